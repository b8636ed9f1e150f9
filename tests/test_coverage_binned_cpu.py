"""CPU: bamCoverage's binsize / ss arguments -- the checks, the warning and which native entry point a call
reaches -- everything that happens before a GPU is needed."""
import os
import warnings

import pytest

from conftest import GOLDEN

from bamsignals_amd import GRanges, _lib, bamCoverage, wrappers

bampath = os.path.join(GOLDEN, "randomBam.bam")


def test_binsize_errors_before_any_io():
    gr = GRanges("chr1", [1, 50], width=[10, 13])
    for bad in (0, -5):
        with pytest.raises(ValueError, match="provide a binsize greater or equal to 1"):
            bamCoverage("nope.bam", gr, binsize=bad, verbose=False)
    with pytest.raises(ValueError, match="65536"):
        bamCoverage("nope.bam", gr, binsize=65537, verbose=False)
    for bad in (2.5, "7", None, True):
        with pytest.raises(ValueError, match="whole number"):
            bamCoverage("nope.bam", gr, binsize=bad, verbose=False)
    with pytest.raises(TypeError, match="must provide a GRanges object"):
        bamCoverage("nope.bam", {"chr1": 1}, binsize=5, verbose=False)


def test_warning_for_widths_not_a_multiple_of_binsize():
    gr = GRanges("chr1", [1, 50], width=[10, 13])
    with pytest.warns(UserWarning, match="not a multiple of the selected"):
        with pytest.raises(_lib.BsigError):                 # (the file does not exist: the warning comes first)
            bamCoverage("nope.bam", gr, binsize=5, verbose=False)
    even = GRanges("chr1", [1, 50], width=[10, 20])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for b in (1, 5, 10.0):
            with pytest.raises(_lib.BsigError):
                bamCoverage("nope.bam", even, binsize=b, verbose=False)


class _Recorder:
    """The real library, with the two coverage entry points replaced by recorders."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith("bsig_coverage_core"):
            return lambda *a: self.calls.append((name, a)) or 0
        return getattr(self._lib, name)


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


def test_defaults_reach_the_reference_entry_point(recorder):
    gr = GRanges("chr1", [1, 50], width=[10, 13], strand=["+", "-"])
    sig = bamCoverage("x.bam", gr, verbose=False)
    sig2 = bamCoverage("x.bam", gr, binsize=1, ss=False, verbose=False)
    wrappers.coverage_core_into("x.bam", gr, ())
    assert [c[0] for c in recorder.calls] == ["bsig_coverage_core", "bsig_coverage_core", "bsig_coverage_core_into"]
    assert not sig.ss and [s.shape for s in sig.as_list()] == [(10,), (13,)]
    assert not sig2.ss


def test_bins_and_strands_reach_the_ex_entry_point(recorder):
    gr = GRanges("chr1", [1, 50], width=[10, 13], strand=["+", "*"])
    with pytest.warns(UserWarning):
        sig = bamCoverage("x.bam", gr, binsize=4, ss=True, paired_end="extend", verbose=False)
    name, args = recorder.calls[-1]
    assert name == "bsig_coverage_core_ex"
    # ... (mapqual, requiredF, filteredF, tspan, maxgap, device, binsize, ss, out, off)
    assert args[-10:-2] == (0, 66, -1, 1, 16385, -1, 4, 1)
    assert sig.ss and [s.shape for s in sig.as_list()] == [(2, 3), (2, 4)]
    sig = bamCoverage("x.bam", gr, ss=True, verbose=False)               # binsize 1 with strands: the new kernel too
    assert recorder.calls[-1][0] == "bsig_coverage_core_ex" and recorder.calls[-1][1][-4:-2] == (1, 1)
    assert [s.shape for s in sig.as_list()] == [(2, 10), (2, 13)]
    out = wrappers.coverage_core_into("x.bam", gr, (), binsize=5, ss=False)
    assert recorder.calls[-1][0] == "bsig_coverage_core_ex_into" and [v.shape for v in out] == [(2,), (3,)]


def test_native_binsize_checks_without_a_gpu():
    """bsig_coverage_core_ex rejects a binsize outside 1 .. 65,536 before it needs a device."""
    gr = GRanges("chr1", [1000], width=[100])
    for bad in (0, 65537):
        with pytest.raises(_lib.BsigError) as e:
            wrappers.coverage_core(bampath, gr, (), binsize=bad, ss=True)
        assert e.value.code_name == "BSIG_ERR_ARG"


def test_mode_constant():
    assert _lib.MODE_COVERAGE_EX == 3
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bamsignals_abi.h")).read()
    assert "BSIG_MODE_COVERAGE_EX = 3" in hdr
