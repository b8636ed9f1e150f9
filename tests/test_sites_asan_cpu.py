"""CPU: the site decision (csrc/sitemath.h: the parameter rule and site_classify, the very function the kernel runs) under
AddressSanitizer + UndefinedBehaviorSanitizer.  `make -C bamsignals_amd/csrc sites` builds it with tests/asan/sites_driver.cpp
into a stand-alone program; the dense cells of the decks and their reference codes go through it in files this test writes, and
the sites it prints are compared with tests/sites_expected.py.  (A CPU build of host code only.)"""
import os
import subprocess

import numpy as np

import sites_expected as sx
from conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "asan", "sites_driver")


def write_input(path, cells, ref, p):
    ss = len(cells) > 0 and cells[0].ndim == 3
    head = np.asarray([p["min_depth"], p["min_alt"], p["num"], p["den"], p["alt_mask"], 2 if ss else 1, 0 if ref is None else 1, len(cells)], dtype="<i4")
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.asarray([c.shape[-1] for c in cells], dtype="<i4").tobytes())
        for c in cells:
            f.write(np.ascontiguousarray(c, dtype="<i4").tobytes())
        for r in ref or ():
            f.write(np.ascontiguousarray(r, dtype=np.uint8).tobytes())


def parse(text, ss):
    """the driver's lines of one file -> the dict sites_expected gives"""
    lines = text.splitlines()
    assert lines[0] == "rule ok" and lines[-1] == f"end {len(lines) - 2}"
    rows = np.asarray([[int(v) for v in ln.split()] for ln in lines[1:-1]], dtype=np.int64).reshape(len(lines) - 2, 3 + (12 if ss else 6))
    return rows


def test_sites_of_the_decks(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bamsignals_amd", "csrc"), "sites"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
    cases = []
    for deck, ss in (("sites", False), ("sites", True), ("random", True), ("hand", False)):
        cells = sx.dense(deck, ss)
        for ref, p in ((sx.ref_of(deck), sx.NAMED), (None, sx.prm(1, 1, 0, 1)), (sx.ref_of(deck), sx.prm(3, 2, 1, 4, sx.MASK_BASES)),
                       (None, sx.prm(2**31 - 1, 2**31 - 1, 1 << 20, 1 << 20))):
            cases.append((str(tmp_path / f"case{len(cases)}.bin"), cells, ref, p, ss))
            write_input(cases[-1][0], cells, ref, p)
    total = 0
    for path, cells, ref, p, ss in cases:
        run = subprocess.run([DRIVER, path], capture_output=True, text=True, env=env, timeout=300)
        assert run.returncode == 0, (run.returncode, run.stdout[-400:], run.stderr[-3000:])
        rows = parse(run.stdout, ss)
        want = sx.expected_sites(cells, ref, p)
        n = len(cells)
        assert np.array_equal(np.searchsorted(rows[:, 0], np.arange(n + 1)), want["seg_off"])
        assert np.array_equal(rows[:, 1], want["pos"]) and np.array_equal(rows[:, 2], want["alleles"])
        assert np.array_equal(rows[:, 3:].reshape(want["counts"].shape), want["counts"])
        total += len(rows)
    assert total > 0


def test_the_rule_sentences(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bamsignals_amd", "csrc"), "sites"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
    said = []
    for k, p in enumerate((sx.prm(0, 1, 0, 1), sx.prm(1, 0, 0, 1), sx.prm(1, 1, 0, 0), sx.prm(1, 1, 0, (1 << 20) + 1), sx.prm(1, 1, 2, 1),
                           sx.prm(1, 1, -1, 1), sx.prm(1, 1, 0, 1, 0), sx.prm(1, 1, 0, 1, 0x40), sx.prm(-2**31, 1, 0, 1))):
        path = str(tmp_path / f"rule{k}.bin")
        write_input(path, [], None, p)
        run = subprocess.run([DRIVER, path], capture_output=True, text=True, env=env, timeout=60)
        assert run.returncode == 0 and run.stdout.startswith("rule ") and run.stdout.strip() != "rule ok", (p, run.stdout, run.stderr[-2000:])
        said.append(run.stdout.strip())
    assert len(set(said)) == 5, said
