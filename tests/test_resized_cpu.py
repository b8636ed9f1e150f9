"""CPU: bamCoverage of reads resized to the fragment (fragLength / frag_len) -- the expected side itself
(tests/resized_expected.py: the column transform against a per-base brute force, and its identities under the existing
oracle), what bamCoverage and the file-level C calls refuse before any I/O, and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import resized_expected as rx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAM = "/nonexistent/dir/file.bam"
ARG, IO = -1, -2
FRAG_LEN_MAX = 1 << 24
SPAN = 36


def toy(seed=11, n=200, span=None):
    """about 200 reads on two references of 600 and 900 bp, both strands, spans 1 .. 80 (or all `span`), sorted"""
    rng = np.random.default_rng(seed)
    ref_len = np.asarray([600, 900], np.int32)
    rid = np.sort(rng.integers(0, 2, n))
    pos = rng.integers(0, ref_len[rid] - 80)
    order = np.lexsort((pos, rid))
    rid, pos = rid[order], pos[order]
    sp = np.full(n, span) if span else rng.integers(1, 81, n)
    flag = np.where(rng.random(n) < 0.5, 16, 0)
    return dict(ref_len=ref_len, ref_off=np.concatenate([[0], np.cumsum(np.bincount(rid, minlength=2))]).astype(np.int64),
                pos=pos.astype(np.int32), end=(pos + sp - 1).astype(np.int32), flag=flag.astype(np.uint16),
                mapq=rng.integers(0, 61, n).astype(np.uint8), tlen=np.zeros(n, np.int32))


def whole_refs(cols, pad=0):
    n = len(cols["ref_len"])
    return dict(rid=np.arange(n, dtype=np.int32), loc=np.zeros(n, np.int32), len=(cols["ref_len"] + pad).astype(np.int32),
                strand=np.ones(n, np.int32))


# ---- the transform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5, SPAN - 1, SPAN, SPAN + 1, 80, 81, 200, 700])
def test_transform_is_the_brute_force(L):
    """below, at and above the reads' spans, past a reference's last base (the ranges overhang it by 300) and below 0"""
    cols = toy()
    rg = whole_refs(cols, pad=300)
    got, off = rx.coverage(rx.resize_columns(cols, L), rg)
    ss, _ = rx.coverage(rx.resize_columns(cols, L), rg, ss=True)
    for r in range(2):
        hi = int(rg["len"][r])
        assert np.array_equal(got[off[r]:off[r + 1]], rx.brute_force(cols, r, 0, hi, L)), (L, r)
        rows = ss[2 * off[r]:2 * off[r + 1]].reshape(-1, 2)
        assert np.array_equal(rows[:, 0], rx.brute_force(cols, r, 0, hi, L, reverse=False))
        assert np.array_equal(rows[:, 1], rx.brute_force(cols, r, 0, hi, L, reverse=True))
    assert got.sum() > 0
    if L >= 200:
        assert got[off[0] + 600:off[1]].sum() > 0            # the overhang of forward fragments is seen


def test_transform_keeps_the_other_columns_and_sorts_stably():
    cols = toy()
    cols["tlen"] = np.arange(len(cols["pos"]), dtype=np.int32)       # a row's identity
    out = rx.resize_columns(cols, 50)
    rid = np.repeat(np.arange(2), np.diff(cols["ref_off"]))
    assert np.all(np.diff(out["pos"].astype(np.int64) + (rid.astype(np.int64) << 32)) >= 0)
    back = out["tlen"]
    assert np.array_equal(np.sort(back), cols["tlen"])
    assert np.array_equal(out["flag"], cols["flag"][back]) and np.array_equal(out["mapq"], cols["mapq"][back])
    rev = (cols["flag"][back] & 16) != 0
    assert np.array_equal(out["end"][rev], cols["end"][back][rev]) and np.array_equal(out["pos"][~rev], cols["pos"][back][~rev])
    assert np.all(out["end"][~rev] - out["pos"][~rev] == 49)
    assert out["pos"].min() >= 0 and np.all(out["end"][rev] - out["pos"][rev] <= 49)
    same = np.flatnonzero(np.diff(out["pos"]) == 0)                  # ties keep the order they had
    same = same[rid[same] == rid[same + 1]]
    assert len(same) and np.all(back[same] < back[same + 1])
    assert np.array_equal(cols["pos"], toy()["pos"])                 # the input is not written to


def test_length_one_is_the_stranded_pileup():
    """coverage of the 5' ends alone is bamProfile(binsize 1, shift 0, ss), cell by cell -- '-' ranges included"""
    from oracle import oracle_c
    cols = toy(seed=5)
    rng = np.random.default_rng(1)
    n = 40
    rid = rng.integers(0, 2, n)
    rg = dict(rid=rid.astype(np.int32), loc=rng.integers(-5, 500, n).astype(np.int32), len=rng.integers(0, 300, n).astype(np.int32),
              strand=rng.choice(np.asarray([1, -1, 0], np.int32), n))
    got, off = rx.expected(cols, rg, 1, ss=True)
    want, woff = oracle_c.pileup_core(rx.oracle_reads(cols), rg, binsize=1, shift=0, ss=True)
    assert np.array_equal(off, woff) and np.array_equal(got, want) and want.any()


def test_reads_of_that_length_are_left_alone():
    cols = toy(span=SPAN)
    out = rx.resize_columns(cols, SPAN)
    for k in rx.COLUMNS:
        assert np.array_equal(out[k], cols[k]), k
    rg = whole_refs(cols)
    assert np.array_equal(rx.expected(cols, rg, SPAN, binsize=7, ss=True)[0], rx.coverage(cols, rg, 7, True)[0])


# ---- bamCoverage(fragLength=...) -------------------------------------------------------------------------------------
def test_wrapper_refuses_before_any_io():
    """on a path that does not exist: a ValueError, not the open's error"""
    from bamsignals_amd import GRanges, bamCoverage
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    for bad in (0, -1, 2.5, True, 2 ** 24 + 1):
        for form in (dict(), dict(aggregate=True), dict(runs=True)):
            with pytest.raises(ValueError, match="fragLength"):
                bamCoverage(BAM, gr, fragLength=bad, verbose=False, **form)
    with pytest.raises(ValueError, match="fragLength.*already has its length"):
        bamCoverage(BAM, gr, fragLength=200, paired_end="extend", verbose=False)
    with pytest.raises(TypeError):
        bamCoverage(BAM, gr, 0, "ignore", None, -1, False, 200)      # keyword-only


def test_wrapper_passes_the_length_down(monkeypatch):
    from bamsignals_amd import GRanges, bamCoverage, wrappers
    seen = []
    for name in ("coverage_core", "coverage_sum", "coverage_runs"):
        monkeypatch.setattr(wrappers, name, lambda *a, _n=name, **k: seen.append((_n, a[2:], k)) or [np.zeros(1, np.int32)])
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    bamCoverage("x.bam", gr, verbose=False)
    bamCoverage("x.bam", gr, verbose=False, fragLength=None)
    bamCoverage("x.bam", gr, verbose=False, fragLength=200.0, binsize=5, ss=True)
    bamCoverage("x.bam", gr, verbose=False, fragLength=np.int64(1), aggregate=True)
    bamCoverage("x.bam", gr, verbose=False, fragLength=2 ** 24, runs=True, paired_end="ignore")
    head = ((), 0, 0, -1, False)
    assert seen == [("coverage_core", head, dict(binsize=1, ss=False, frag_len=0)),
                    ("coverage_core", head, dict(binsize=1, ss=False, frag_len=0)),
                    ("coverage_core", head, dict(binsize=5, ss=True, frag_len=200)),
                    ("coverage_sum", head, dict(binsize=1, ss=False, frag_len=1)),
                    ("coverage_runs", head, dict(binsize=1, ss=False, frag_len=2 ** 24))]


def test_cores_refuse_a_length_beside_tspan():
    from bamsignals_amd import GRanges, wrappers
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    for core in (wrappers.coverage_core, wrappers.coverage_sum, wrappers.coverage_runs):
        with pytest.raises(ValueError, match="frag_len excludes tspan"):
            core(BAM, gr, (0, 1000), tspan=True, frag_len=200)


# ---- the file-level C calls ------------------------------------------------------------------------------------------
def _call(which, frag_len, tlen_filter=(), binsize=1, ss=0, widths=(100, 100)):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray(widths, np.int32)
    n = len(width)
    codes, start, strand = np.zeros(n, np.int32), np.full(n, 1000, np.int32), np.ones(n, np.int32)
    levels = (C.c_char_p * 1)(b"chr1")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    head = (BAM.encode(), n, codes.ctypes.data, 1, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
            tf.ctypes.data, len(tlen_filter), 0, 0, -1, frag_len, 16385, -1, binsize, ss)
    handle = C.c_void_p()
    if which == "core":
        out, off = np.zeros(4 * int(np.abs(width).sum()) + 4, np.int32), np.zeros(n + 1, np.int64)
        lib.bsig_layout(n, width.ctypes.data, binsize, ss, off.ctypes.data)
        rc = lib.bsig_coverage_core_resized(*head, out.ctypes.data, off.ctypes.data)
    elif which == "sum":
        out = np.zeros(4 * int(np.abs(width).max()) + 4, np.int64)
        rc = lib.bsig_coverage_sum_resized(*head, out.ctypes.data)
    else:
        rc = lib.bsig_coverage_runs_resized(*head, C.byref(handle))
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route(), handle.value


RANGE_MSG = "the fragment length must be between 1 and 16777216 (%d given)"


@pytest.mark.parametrize("which", ["core", "sum", "runs"])
@pytest.mark.parametrize("a,message", [
    (dict(frag_len=0), RANGE_MSG % 0),
    (dict(frag_len=-7), RANGE_MSG % -7),
    (dict(frag_len=FRAG_LEN_MAX + 1), RANGE_MSG % (FRAG_LEN_MAX + 1)),
    (dict(frag_len=200, tlen_filter=(50,)), "tlen_filter must have 0 or 2 elements"),
    (dict(frag_len=200, binsize=0), "provide a binsize greater or equal to 1"),
    (dict(frag_len=200, binsize=65537), "coverage bins are at most 65536 bases wide (bamProfile / bamCount count at that scale)"),
])
def test_file_level_calls_judge_their_parameters_before_the_open(which, a, message):
    """a length of 0 (tspan's "off", which is no length), any other length out of range, and the plan's own rule"""
    rc, msg, route, handle = _call(which, **a)
    assert (rc, msg) == (ARG, message)
    assert route == b"" and not handle


@pytest.mark.parametrize("which", ["core", "sum", "runs"])
def test_file_level_calls_then_fail_at_the_open(which):
    for frag_len in (1, 200, FRAG_LEN_MAX):
        rc, msg, _, handle = _call(which, frag_len, tlen_filter=(0, 1000), binsize=5, ss=1)
        assert rc == IO and "Fail to open BAM file" in msg and not handle


def _params(mode, **a):
    from bamsignals_amd.device import make_params
    return make_params(mode, **a)


@pytest.mark.parametrize("creator", ["bsig_plan_create_resized", "bsig_plan_create_sum_resized"])
def test_plan_creators_judge_their_parameters_without_a_device(creator):
    """as bsig_plan_create does: two zeroed blocks stand in for the handles, which a refused call never looks into"""
    from bamsignals_amd import _lib
    lib = _lib.load()
    ctx, reads = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 16)
    rid, loc, ln, strand = (np.zeros(2, np.int32), np.full(2, 1000, np.int32), np.full(2, 100, np.int32), np.ones(2, np.int32))

    def call(p, frag_len):
        h = C.c_void_p()
        rc = getattr(lib, creator)(C.cast(ctx, C.c_void_p), C.cast(reads, C.c_void_p), 2, rid.ctypes.data, loc.ctypes.data,
                                   ln.ctypes.data, strand.ctypes.data, C.byref(p), frag_len, C.byref(h))
        assert not h.value
        return rc, lib.bsig_last_error().decode()
    for mode in (_lib.MODE_PROFILE, _lib.MODE_COUNT, _lib.MODE_OVERLAP_ANY, _lib.MODE_OVERLAP_WITHIN, 6, 7):
        assert call(_params(mode), 200) == (ARG, "reads are resized to the fragment for bamCoverage only (mode %d given)" % mode)
    for mode in (_lib.MODE_COVERAGE, _lib.MODE_COVERAGE_EX):
        assert call(_params(mode, tspan=True, tlen_filter=(0, 1000)), 200) == \
            (ARG, "a paired-end fragment already has its length: tspan must be 0 with a fragment length")
        for bad in (0, -1, FRAG_LEN_MAX + 1, 2 ** 31 - 1):
            assert call(_params(mode), bad) == (ARG, RANGE_MSG % bad)
        assert call(_params(mode, threads=96), 200) == (ARG, "threads must be 64, 128 or 256")
    assert call(_params(_lib.MODE_COVERAGE_EX, binsize=0), 200) == (ARG, "provide a binsize greater or equal to 1")


# ---- the ABI ---------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("bsig_plan_create_resized", "bsig_plan_create_sum_resized", "bsig_coverage_core_resized",
               "bsig_coverage_sum_resized", "bsig_coverage_runs_resized")


def test_abi():
    from bamsignals_amd import _lib, wrappers
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+BSIG_FRAG_LEN_MAX\s+\(1 << 24\)", code)
    assert wrappers.MAX_FRAG_LENGTH == FRAG_LEN_MAX
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", code).group(1)) == 4 and lib.bsig_abi_version() == 4
    assert C.sizeof(_lib.Params) == 56
    # the length is an argument: the struct has no field for it
    fields = re.search(r"typedef struct \{([^}]*)\}\s*bsig_params;", code).group(1)
    assert "frag" not in fields and len(re.findall(r"\bint32_t\b", fields)) == 13
