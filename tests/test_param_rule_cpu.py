"""CPU: one rule for a plan's parameters.  Every file-level entry point refuses a bad parameter with the code and message
bsig_plan_create / bsig_plan_create_sum give (test_gpu_parity.py::test_error_paths runs the same table through Plan and
SumPlan), and does so before the BAM is decoded -- so before any device is needed."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

from bamsignals_amd import _lib

BAM = os.path.join(GOLDEN, "randomBam.bam")
ARG, EXT = -1, -5
TOO_FAR = 2 ** 30 + 1
TOO_LARGE = "shift / tlen filter too large"
NO_FILTER = "paired-end midpoint/extend needs a 2-element tlen_filter"
NO_COUNT_SUM = "bamCount has no sum over ranges (its sum is one number per strand)"
UNEQUAL = "all signals must have the same length"

# (family, what differs from the defaults, "all" entry points or the "sum"s only, code, message).  The family picks the
# entry points: pileup = bsig_pileup_core[_into] / bsig_pileup_sum, coverage = bsig_coverage_core_ex[_into] /
# bsig_coverage_sum; `widths` are the ranges' widths (default two of 100).
CASES = [
    ("pileup", dict(tlen_filter=(50,)), "all", ARG, "tlen_filter must have 0 or 2 elements"),
    ("pileup", dict(pe_mid=1), "all", ARG, NO_FILTER),
    ("pileup", dict(shift=TOO_FAR), "all", ARG, TOO_LARGE),
    ("pileup", dict(shift=-TOO_FAR), "all", ARG, TOO_LARGE),
    ("pileup", dict(pe_mid=1, shift=2 ** 29 + 1, tlen_filter=(0, 2 ** 29)), "all", ARG, TOO_LARGE),
    ("pileup", dict(binsize=0), "sum", ARG, NO_COUNT_SUM),
    ("pileup", dict(binsize=-1), "sum", ARG, NO_COUNT_SUM),
    ("pileup", dict(widths=(100, 101)), "sum", ARG, UNEQUAL),
    ("coverage", dict(tlen_filter=(50,)), "all", ARG, "tlen_filter must have 0 or 2 elements"),
    ("coverage", dict(tspan=1), "all", ARG, NO_FILTER),
    ("coverage", dict(tspan=1, tlen_filter=(0, -5)), "all", EXT, "negative 'ext' values don't make sense"),
    ("coverage", dict(binsize=0), "all", ARG, "provide a binsize greater or equal to 1"),
    ("coverage", dict(binsize=65537), "all", ARG,
     "coverage bins are at most 65536 bases wide (bamProfile / bamCount count at that scale)"),
    ("coverage", dict(widths=(100, 101)), "sum", ARG, UNEQUAL),
]
ENTRY = {"pileup": ("bsig_pileup_core", "bsig_pileup_core_into", "bsig_pileup_sum"),
         "coverage": ("bsig_coverage_core_ex", "bsig_coverage_core_ex_into", "bsig_coverage_sum")}


def args(a):
    """a case's arguments with the defaults filled in"""
    return dict(dict(mapqual=0, binsize=1, shift=0, ss=0, requiredF=0, filteredF=-1, pe_mid=0, tspan=0, tlen_filter=(),
                     widths=(100, 100)), **a)


def params(family, a):
    """the case as bsig_params, built by hand (make_params refuses a filter of one value itself)"""
    a = args(a)
    p = _lib.Params()
    p.mode = (_lib.MODE_COUNT if a["binsize"] <= 0 else _lib.MODE_PROFILE) if family == "pileup" else _lib.MODE_COVERAGE_EX
    for k in ("mapqual", "binsize", "shift", "ss", "requiredF", "filteredF", "pe_mid", "tspan"):
        setattr(p, k, a[k])
    p.n_tlen_filter = len(a["tlen_filter"])
    for i, v in enumerate(a["tlen_filter"][:2]):
        p.tlen_filter[i] = v
    return p


def call_file_level(name, family, a):
    """one call of a file-level entry point on the fixture BAM, ranges on chr1 and chr2; (code, message)"""
    a = args(a)
    lib = _lib.load()
    width = np.asarray(a["widths"], np.int32)
    n = len(width)
    codes, start, strand = np.arange(n, dtype=np.int32) % 2, np.full(n, 1000, np.int32), np.ones(n, np.int32)
    levels = (C.c_char_p * 2)(b"chr1", b"chr2")
    tf = np.asarray(a["tlen_filter"] or (0,), np.int32)
    head = (BAM.encode(), n, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
            tf.ctypes.data, len(a["tlen_filter"]))
    cells = int(width.max()) * 2 * n
    out, off, sums = np.zeros(cells, np.int32), np.zeros(n + 1, np.int64), np.zeros(cells, np.int64)
    lib.bsig_layout(n, width.ctypes.data, max(a["binsize"], 1), a["ss"], off.ctypes.data)
    vs = [np.zeros(cells, np.int32) for _ in range(n)]
    dst = (C.c_void_p * n)(*[v.ctypes.data for v in vs])
    if family == "pileup":
        mid = (a["mapqual"], a["binsize"], a["shift"], a["ss"], a["requiredF"], a["filteredF"], a["pe_mid"], 16385, -1)
    else:
        mid = (a["mapqual"], a["requiredF"], a["filteredF"], a["tspan"], 16385, -1, a["binsize"], a["ss"])
    tail = {"core": (out.ctypes.data, off.ctypes.data), "into": (dst,), "sum": (sums.ctypes.data,)}
    kind = "sum" if name.endswith("_sum") else "into" if name.endswith("_into") else "core"
    rc = getattr(lib, name)(*head, *mid, *tail[kind])
    return rc, lib.bsig_last_error().decode()


@pytest.mark.parametrize("family,a,which,code,message", CASES)
def test_one_bad_parameter_fails_every_entry_point_alike(family, a, which, code, message):
    names = ENTRY[family] if which == "all" else ENTRY[family][2:]
    for name in names:
        assert call_file_level(name, family, a) == (code, message), name
        if "shift" in a:
            # refused before the decode: the call never got as far as saying how it was carried out
            assert _lib.load().bsig_last_call_route() == b"", name
