"""CPU: which refusal wins.  Every file-level entry point of the ABI is called with one fault, and with two at once, on
the fixture BAM; the code, the text of bsig_last_error() and the (empty) route are compared with a table RECORDED from
the library as it was before the file-level path was cut into stages.  Some entry points judge a parameter before they
open the BAM and others after: that order is part of the interface, and cases e, f and g pin it.

The faults:  a  the output argument missing (out / off, dst, sum or result NULL)
             b  a one-element tlen_filter
             c  a bampath that does not exist
             d  a chromosome that the fixture BAM does not have
             e  b and c        f  b and d
             g  the call's own parameter (views: lower > upper; overlaps: a type that is neither 0 nor 1; the resized
                calls: a fragment length of 0) together with c
`python tests/test_file_level_refusals_cpu.py` prints the table of the library that BSIG_LIB_PATH names."""
import ctypes as C
import os
import pprint

import numpy as np
import pytest

from conftest import GOLDEN

from bamsignals_amd import _lib

BAM = os.path.join(GOLDEN, "randomBam.bam")
MISSING = os.path.join(GOLDEN, "no_such_file.bam")

# the int32 arguments between n_tlen_filter and the output, by family (None: the thresholds pointer, NULL with 0 of them)
PILEUP = dict(mapqual=0, binsize=1, shift=0, ss=0, requiredF=0, filteredF=-1, pe_mid=0, maxgap=16385, device=-1)
COVERAGE = dict(mapqual=0, requiredF=0, filteredF=-1, tspan=0, maxgap=16385, device=-1)
COVERAGE_EX = dict(COVERAGE, binsize=1, ss=0)
RESIZED = dict(mapqual=0, requiredF=0, filteredF=-1, frag_len=150, maxgap=16385, device=-1, binsize=1, ss=0)
BAND = dict(lower=1, upper=5)
# name: (arguments, kind of output, tlen_filter of a good call)
ENTRIES = {
    "bsig_pileup_core": (PILEUP, "flat", ()),
    "bsig_pileup_core_into": (PILEUP, "into", ()),
    "bsig_overlap_core": (dict(mapqual=0, overlap_type=0, min_overlap=1, ss=0, requiredF=0, filteredF=-1, tspan=0, maxgap=16385,
                               device=-1), "flat", ()),
    "bsig_coverage_core": (COVERAGE, "flat", ()),
    "bsig_coverage_core_into": (COVERAGE, "into", ()),
    "bsig_coverage_core_ex": (COVERAGE_EX, "flat", ()),
    "bsig_coverage_core_ex_into": (COVERAGE_EX, "into", ()),
    "bsig_pileup_sum": (PILEUP, "int64", ()),
    "bsig_coverage_sum": (COVERAGE_EX, "int64", ()),
    "bsig_pileup_xcorr": (dict(mapqual=0, requiredF=0, filteredF=-1, max_lag=10, maxgap=16385, device=-1), "int64", ()),
    "bsig_pileup_frag": (dict(mapqual=0, requiredF=0, filteredF=-1, pe_mid=0, len_bin=10, maxgap=16385, device=-1), "int64", (0, 500)),
    "bsig_pileup_hist": (dict(mapqual=0, ss=0, requiredF=0, filteredF=-1, pe_mid=0, max_value=10, maxgap=16385, device=-1), "int64", ()),
    "bsig_coverage_hist": (dict(mapqual=0, requiredF=0, filteredF=-1, tspan=0, max_value=10, maxgap=16385, device=-1), "int64", ()),
    "bsig_pileup_summary": (dict(mapqual=0, ss=0, requiredF=0, filteredF=-1, pe_mid=0, n_thresholds=0, thresholds=None, maxgap=16385,
                                 device=-1), "int64", ()),
    "bsig_coverage_summary": (dict(mapqual=0, requiredF=0, filteredF=-1, tspan=0, n_thresholds=0, thresholds=None, maxgap=16385,
                                   device=-1), "int64", ()),
    "bsig_pileup_scaled": (dict(mapqual=0, ss=0, requiredF=0, filteredF=-1, pe_mid=0, n_bins=4, maxgap=16385, device=-1), "int64", ()),
    "bsig_coverage_scaled": (dict(mapqual=0, requiredF=0, filteredF=-1, tspan=0, n_bins=4, maxgap=16385, device=-1), "int64", ()),
    "bsig_pileup_runs": (PILEUP, "handle", ()),
    "bsig_coverage_runs": (COVERAGE_EX, "handle", ()),
    "bsig_coverage_core_resized": (RESIZED, "flat", ()),
    "bsig_coverage_sum_resized": (RESIZED, "int64", ()),
    "bsig_coverage_runs_resized": (RESIZED, "handle", ()),
    "bsig_pileup_views": (dict(PILEUP, **BAND), "handle", ()),
    "bsig_coverage_views": (dict(COVERAGE_EX, **BAND), "handle", ()),
    "bsig_coverage_views_resized": (dict(RESIZED, **BAND), "handle", ()),
}
# a call's own bad parameter (case g)
OWN = {"band": dict(lower=5, upper=1), "type": dict(overlap_type=7), "length": dict(frag_len=0)}
FAULTS = {"a": {"output"}, "b": {"filter"}, "c": {"file"}, "d": {"chrom"}, "e": {"filter", "file"}, "f": {"filter", "chrom"}}


def cases(name):
    """the cases of an entry point: a .. f, and one g per parameter of its own"""
    mid = ENTRIES[name][0]
    own = [k for k, v in OWN.items() if set(v) <= set(mid)]
    return list(FAULTS) + ["g:" + k for k in own]


def call(name, case):
    """one call of the entry point on two ranges of width 100 with the case's faults; (code, message, route)"""
    lib = _lib.load()
    mid, kind, good_filter = ENTRIES[name]
    faults = FAULTS[case] if case in FAULTS else {"file", case[2:]}
    mid = dict(mid, **OWN.get(case[2:], {}))
    n = 2
    width, start, strand = np.full(n, 100, np.int32), np.full(n, 1000, np.int32), np.ones(n, np.int32)
    codes = np.arange(n, dtype=np.int32) % 2
    levels = (C.c_char_p * 2)(b"chr1", b"chrNone" if "chrom" in faults else b"chr2")
    tf = np.asarray((50,) if "filter" in faults else good_filter or (0,), np.int32)
    n_tf = 1 if "filter" in faults else len(good_filter)
    path = MISSING if "file" in faults else BAM
    head = (path.encode(), n, codes.ctypes.data, 2, levels, start.ctypes.data, width.ctypes.data, strand.ctypes.data,
            tf.ctypes.data, n_tf)
    cells = 4096
    out, off, wide = np.zeros(cells, np.int32), np.zeros(n + 1, np.int64), np.zeros(cells, np.int64)
    lib.bsig_layout(n, width.ctypes.data, mid.get("binsize", 1), mid.get("ss", 0), off.ctypes.data)
    vs = [np.zeros(cells, np.int32) for _ in range(n)]
    dst = (C.c_void_p * n)(*[v.ctypes.data for v in vs])
    handle = C.c_void_p()
    missing = "output" in faults
    tail = {"flat": (None, None) if missing else (out.ctypes.data, off.ctypes.data),
            "into": (None if missing else dst,),
            "int64": (None if missing else wide.ctypes.data,),
            "handle": (None if missing else C.byref(handle),)}[kind]
    rc = getattr(lib, name)(*head, *mid.values(), *tail)
    assert handle.value is None, "a refused call hands out no result"
    return rc, lib.bsig_last_error().decode().replace(MISSING, "<missing>"), lib.bsig_last_call_route()


# ---- recorded from the library of the commit before the stages (see the module's docstring); not derived from the code under test
NO_FILE = (-2, "Fail to open BAM file <missing>")
NO_CHROM = (-4, "chromosome chrNone not present in the bam file")
ONE_VALUE = (-1, "tlen_filter must have 0 or 2 elements")
NO_RESULT = (-1, "result is NULL")
NO_OUT = (-1, "out is NULL")
NO_LENGTH = (-1, "the fragment length must be between 1 and 16777216 (0 given)")
BAD_BAND = (-1, "lower (5) is above upper (1)")
FRAG_FILTER = (-1, "the fragment-length histogram needs a 2-element tlen_filter")
EXPECTED = {
    "bsig_pileup_core": {"a": (-1, "offsets missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_pileup_core_into": {"a": (-1, "destinations missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_overlap_core": {"a": (-1, "offsets missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE,
                          "g:type": (-1, "overlap type must be 0 (any) or 1 (within)")},
    "bsig_coverage_core": {"a": (-1, "offsets missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_coverage_core_into": {"a": (-1, "destinations missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_coverage_core_ex": {"a": (-1, "offsets missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_coverage_core_ex_into": {"a": (-1, "destinations missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_pileup_sum": {"a": (-1, "sum is NULL"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_coverage_sum": {"a": (-1, "sum is NULL"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_pileup_xcorr": {"a": NO_OUT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": NO_FILE, "f": NO_CHROM},
    "bsig_pileup_frag": {"a": NO_OUT, "b": FRAG_FILTER, "c": NO_FILE, "d": NO_CHROM, "e": FRAG_FILTER, "f": FRAG_FILTER},
    "bsig_pileup_hist": {"a": NO_OUT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_coverage_hist": {"a": NO_OUT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_pileup_summary": {"a": NO_OUT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_coverage_summary": {"a": NO_OUT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_pileup_scaled": {"a": NO_OUT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_coverage_scaled": {"a": NO_OUT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_pileup_runs": {"a": NO_RESULT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_coverage_runs": {"a": NO_RESULT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE},
    "bsig_coverage_core_resized": {"a": (-1, "offsets missing"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE,
                                   "g:length": NO_LENGTH},
    "bsig_coverage_sum_resized": {"a": (-1, "sum is NULL"), "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE,
                                  "g:length": NO_LENGTH},
    "bsig_coverage_runs_resized": {"a": NO_RESULT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE,
                                   "g:length": NO_LENGTH},
    "bsig_pileup_views": {"a": NO_RESULT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE, "g:band": BAD_BAND},
    "bsig_coverage_views": {"a": NO_RESULT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE, "g:band": BAD_BAND},
    "bsig_coverage_views_resized": {"a": NO_RESULT, "b": ONE_VALUE, "c": NO_FILE, "d": NO_CHROM, "e": ONE_VALUE, "f": ONE_VALUE, "g:band": BAD_BAND,
                                    "g:length": NO_LENGTH},
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_refusals_are_the_recorded_ones(name):
    assert set(EXPECTED[name]) == set(cases(name))
    for case in cases(name):
        code, message, route = call(name, case)
        assert (code, message) == EXPECTED[name][case], (name, case)
        assert route == b"", (name, case)


def test_every_file_level_entry_point_of_the_abi_is_in_the_table():
    import re
    abi = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bamsignals_abi.h")).read()
    named = set(re.findall(r"^int (bsig_\w+)\(const char \*bampath, int64_t n_ranges", abi, re.M))
    assert named == set(ENTRIES)


if __name__ == "__main__":
    pprint.pprint({name: {case: call(name, case)[:2] for case in cases(name)} for name in ENTRIES}, width=150, sort_dicts=False)
