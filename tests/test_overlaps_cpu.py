"""CPU: bamOverlaps' expected side (tests/overlaps_expected.py) -- the numpy restatement of the definition against the
identity built from the C oracle's coverage and bamCount --, the ABI's declaration, the parameter rule without a device,
and bamOverlaps' own argument errors.  The first five tests are about the helper alone and need nothing of the library's;
the header, parameter-rule and wrapper tests are the ones that fail without bamOverlaps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import overlaps_expected as oe

BAM = os.path.join(GOLDEN, "randomBam.bam")
# (what the oracle identity can express: type "any", minoverlap 1, filteredF -1)
PARAMS = (dict(), dict(requiredF=66, tlen_filter=(0, 1000)), dict(requiredF=66, tlen_filter=(0, 1000), tspan=True),
          dict(mapqual=30))


@pytest.fixture(scope="module")
def synth():
    from bamsignals_amd.synth import synth_reads
    cols = synth_reads(400_000, [2_000_000, 700_017], seed=92, paired=True, with_cigar=False)
    return cols, oe.oracle_reads(cols), oe.mixed_ranges(cols["ref_len"], 93)


def test_restatement_is_the_oracle_identity_on_synthetic_pairs(synth):
    cols, orc, rg = synth
    totals = []
    for kw in PARAMS:
        for ss in (False, True):
            want = oe.from_oracle(orc, rg, ss=ss, **kw)
            got = oe.restated(cols, rg, ss=ss, **kw)
            assert got.dtype == np.int32 and len(got) == len(rg["len"]) * (2 if ss else 1)
            assert np.array_equal(got, want), (kw, ss)
        totals.append(int(got.sum()))
    assert min(totals) > 100_000                         # (not vacuous)
    assert totals[1] != totals[2]                        # extend counts fragments the reads alone do not reach
    assert not oe.restated(cols, rg)[np.asarray(rg["len"]) == 0].any()


def test_restatement_is_the_oracle_identity_on_the_fixture(fixture_reads, fixture_regions):
    _, rg = fixture_regions
    fixture_reads = oe.fixture_columns(fixture_reads)
    orc = oe.oracle_reads(fixture_reads)
    total = 0
    for kw in PARAMS:
        for ss in (False, True):
            got = oe.restated(fixture_reads, rg, ss=ss, **kw)
            assert np.array_equal(got, oe.from_oracle(orc, rg, ss=ss, **kw)), (kw, ss)
        total += int(got.sum())
    assert total > 1000


def test_minoverlap_and_within_change_the_answer(synth):
    cols, _, rg = synth
    base = oe.restated(cols, rg)
    m50, inside = oe.restated(cols, rg, m=50), oe.restated(cols, rg, within=True)
    assert np.all(m50 <= base) and np.all(inside <= base)
    assert 0 < int(m50.sum()) < int(base.sum()) and 0 < int(inside.sum()) < int(base.sum())
    # strands: the two rows add up to the unstranded count, and a '-' range swaps them
    two = oe.restated(cols, rg, ss=True).reshape(-1, 2)
    assert np.array_equal(two.sum(axis=1), base)
    flipped = dict(rg, strand=-np.where(np.asarray(rg["strand"]) == 0, 1, rg["strand"]))
    assert np.array_equal(oe.restated(cols, flipped, ss=True).reshape(-1, 2), two[:, ::-1])


def test_width_one_range_is_the_coverage_cell(synth):
    from oracle import oracle_c
    cols, orc, _ = synth
    rng = np.random.default_rng(7)
    n = 300
    rid = rng.integers(0, 2, n).astype(np.int32)
    rg = dict(rid=rid, loc=rng.integers(0, cols["ref_len"][rid]).astype(np.int32), len=np.ones(n, np.int32),
              strand=np.ones(n, np.int32))
    for kw in (dict(), dict(requiredF=66, tlen_filter=(0, 1000), tspan=True)):
        cov, _ = oracle_c.coverage_core(orc, rg, **kw)
        assert np.array_equal(oe.restated(cols, rg, **kw), cov) and cov.sum() > 0


def test_planted_reads_have_a_known_answer():
    lo, w = 1000, 200
    rg = dict(rid=[0], loc=[lo], len=[w], strand=[1])
    hi = lo + w
    # (first base, span) -> any m=1, any m=10, within m=1
    for pos, span, want in (((lo - 50), 50, (0, 0, 0)), ((lo - 50), 51, (1, 0, 0)), ((lo - 50), 60, (1, 1, 0)),
                            (hi - 1, 30, (1, 0, 0)), (hi, 30, (0, 0, 0)), (lo, w, (1, 1, 1)), (lo - 1, w + 1, (1, 1, 0)),
                            (lo, w + 1, (1, 1, 0)), (lo - 100, w + 200, (1, 1, 0)), (lo + 5, 9, (1, 0, 1))):
        for reverse in (False, True):
            cols = oe.merge_sorted([oe.planted(pos, span, reverse=reverse)], 1)
            got = (int(oe.restated(cols, rg)[0]), int(oe.restated(cols, rg, m=10)[0]), int(oe.restated(cols, rg, within=True)[0]))
            assert got == want, (pos, span, reverse)
            assert oe.restated(cols, rg, ss=True).tolist() == ([0, want[0]] if reverse else [want[0], 0])


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_the_library_exports_it():
    from bamsignals_amd import _lib
    txt = open(os.path.join(ROOT, "include", "bamsignals_abi.h")).read()
    assert re.search(r"\bint\s+bsig_overlap_core\s*\(", txt)
    assert re.search(r"BSIG_MODE_OVERLAP_ANY\s*=\s*4\b", txt) and re.search(r"BSIG_MODE_OVERLAP_WITHIN\s*=\s*5\b", txt)
    assert int(re.search(r"#define\s+BSIG_ABI_VERSION\s+(\d+)", txt).group(1)) == 4
    lib = _lib.load()
    assert hasattr(lib, "bsig_overlap_core") and lib.bsig_abi_version() == 4
    assert (_lib.MODE_OVERLAP_ANY, _lib.MODE_OVERLAP_WITHIN) == (4, 5)
    assert C.sizeof(_lib.Params) == 14 * 4                # bsig_params did not grow: minoverlap rides in binsize


# (what differs from a good call, code, message): test_overlaps_gpu.py runs the same table through Plan
ARG, EXT = -1, -5
PARAM_RULE = [
    (dict(binsize=0), ARG, "minoverlap must be at least 1"),
    (dict(binsize=-1), ARG, "minoverlap must be at least 1"),
    (dict(shift=1), ARG, "bamOverlaps takes no shift: a read overlaps where it lies"),
    (dict(pe_mid=1, tlen_filter=(0, 1000)), ARG, "bamOverlaps has no midpoint rule: a fragment overlaps as a whole (extend)"),
    (dict(tspan=1), ARG, "paired-end midpoint/extend needs a 2-element tlen_filter"),
    (dict(tlen_filter=(50,)), ARG, "tlen_filter must have 0 or 2 elements"),
    (dict(tspan=1, tlen_filter=(0, -5)), EXT, "negative 'ext' values don't make sense"),
    (dict(tspan=1, tlen_filter=(0, 2 ** 30 + 1)), ARG, "shift / tlen filter too large"),
    (dict(threads=96), ARG, "threads must be 64, 128 or 256"),
]


def overlap_params(mode, a):
    from bamsignals_amd import _lib
    a = dict(dict(mapqual=0, binsize=1, shift=0, ss=0, requiredF=0, filteredF=-1, pe_mid=0, tspan=0, tlen_filter=(),
                  threads=0), **a)
    p = _lib.Params()
    p.mode = mode
    for k in ("mapqual", "binsize", "shift", "ss", "requiredF", "filteredF", "pe_mid", "tspan", "threads"):
        setattr(p, k, a[k])
    p.n_tlen_filter = len(a["tlen_filter"])
    for i, v in enumerate(a["tlen_filter"][:2]):
        p.tlen_filter[i] = v
    return p


@pytest.mark.parametrize("mode", [4, 5])
@pytest.mark.parametrize("a,code,message", PARAM_RULE)
def test_parameter_rule_of_a_plan_needs_no_device(a, code, message, mode):
    """bsig_plan_create judges the parameters before it reads its context or its reads: two zeroed blocks stand in for
    the handles, which a refused call never looks into"""
    from bamsignals_amd import _lib
    lib = _lib.load()
    ctx, reads = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 16)
    rid, loc, ln, strand = (np.zeros(2, np.int32), np.full(2, 1000, np.int32), np.full(2, 100, np.int32), np.ones(2, np.int32))
    h = C.c_void_p()
    rc = lib.bsig_plan_create(C.cast(ctx, C.c_void_p), C.cast(reads, C.c_void_p), 2, rid.ctypes.data, loc.ctypes.data,
                              ln.ctypes.data, strand.ctypes.data, C.byref(overlap_params(mode, a)), C.byref(h))
    assert (rc, lib.bsig_last_error().decode()) == (code, message)
    assert not h.value


def _call_overlap(overlap_type=0, min_overlap=1, tspan=0, tlen_filter=(), widths=(100, 100)):
    from bamsignals_amd import _lib
    lib = _lib.load()
    width = np.asarray(widths, np.int32)
    n = len(width)
    codes, start, strand = np.arange(n, dtype=np.int32) % 2, np.full(n, 1000, np.int32), np.ones(n, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(tlen_filter or (0,), np.int32)
    out, off = np.zeros(2 * n, np.int32), np.zeros(n + 1, np.int64)
    lib.bsig_layout(n, width.ctypes.data, -1, 0, off.ctypes.data)
    rc = lib.bsig_overlap_core(BAM.encode(), n, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data,
                               strand.ctypes.data, tf.ctypes.data, len(tlen_filter), 0, overlap_type, min_overlap, 0, 0, -1,
                               tspan, 16385, -1, out.ctypes.data, off.ctypes.data)
    return rc, lib.bsig_last_error().decode(), lib.bsig_last_call_route()


@pytest.mark.parametrize("a,code,message", [
    (dict(min_overlap=0), ARG, "minoverlap must be at least 1"),
    (dict(overlap_type=2), ARG, "overlap type must be 0 (any) or 1 (within)"),
    (dict(tspan=1), ARG, "paired-end midpoint/extend needs a 2-element tlen_filter"),
    (dict(tlen_filter=(50,)), ARG, "tlen_filter must have 0 or 2 elements"),
    (dict(tspan=1, tlen_filter=(0, -5)), EXT, "negative 'ext' values don't make sense"),
    (dict(tspan=1, tlen_filter=(0, 2 ** 30 + 1)), ARG, "shift / tlen filter too large"),
    (dict(widths=(100, -1)), ARG, "range 1 has a negative width"),
])
def test_parameter_rule_at_file_level(a, code, message):
    rc, msg, route = _call_overlap(**a)
    assert (rc, msg) == (code, message)
    assert route == b""                          # refused before the BAM is opened


# ---- bamOverlaps' own errors -----------------------------------------------------------------------------------------
def test_wrapper_refuses_before_any_native_call(monkeypatch):
    from bamsignals_amd import GRanges, bamOverlaps, wrappers
    def boom(*a, **k):  # noqa: E306
        raise AssertionError("native call made")
    monkeypatch.setattr(wrappers, "overlap_core", boom)
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    for bad in (0, -3, 2.5, "7", True, None, 2 ** 31):
        with pytest.raises(ValueError, match="minoverlap"):
            bamOverlaps("/nonexistent/file.bam", gr, minoverlap=bad, verbose=False)
    with pytest.raises(ValueError, match="'type' should be one of"):
        bamOverlaps("/nonexistent/file.bam", gr, type="start", verbose=False)
    with pytest.raises(ValueError, match="'paired.end' should be one of"):
        bamOverlaps("/nonexistent/file.bam", gr, paired_end="midpoint", verbose=False)
    with pytest.raises(ValueError, match="tlenFilter"):
        bamOverlaps("/nonexistent/file.bam", gr, paired_end="extend", tlenFilter=(300, 100), verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamOverlaps("/nonexistent/file.bam", [("chr1", 1, 100)], verbose=False)
    for good in (dict(), dict(type="within", minoverlap=30.0), dict(type="w", paired_end="extend", ss=True),
                 dict(paired_end="filter", tlenFilter=(50, 200))):
        with pytest.raises(AssertionError, match="native call made"):       # ... and a good call does get there
            bamOverlaps("/nonexistent/file.bam", gr, verbose=False, **good)


def test_wrapper_passes_the_reference_style_arguments(monkeypatch):
    from bamsignals_amd import GRanges, bamOverlaps, wrappers
    seen = []
    monkeypatch.setattr(wrappers, "overlap_core", lambda *a: seen.append(a[2:]) or np.zeros(1, np.int32))
    gr = GRanges(["chr1"], [1], width=[100], strand=["+"])
    bamOverlaps("x.bam", gr, verbose=False)
    bamOverlaps("x.bam", gr, mapqual=20, type="within", minoverlap=30, ss=True, paired_end="filter", filteredFlag=1024, verbose=False)
    bamOverlaps("x.bam", gr, paired_end="extend", tlenFilter=(50, 400), verbose=False)
    assert seen == [((), 0, False, 1, False, 0, -1, False), ((0, 1000), 20, True, 30, True, 66, 1024, False),
                    ((50, 400), 0, False, 1, False, 66, -1, True)]
