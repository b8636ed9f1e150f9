"""CPU: the range arithmetic of the file-level calls (csrc/rangemath.h) under AddressSanitizer + UndefinedBehaviorSanitizer.

`make -C bamsignals_amd/csrc rangemath` builds tests/asan/rangemath_driver.cpp, a program of its own that includes that
header and nothing else of the library.  Seeded cases go through it; its answers are compared with a restatement in numpy
written here, and checked for what must hold whatever the restatement says: every range dealt exactly once, the runs of a
shard partition it and are maximal, the blocks tile every slot's share inside the budget."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "asan", "rangemath_driver")


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bamsignals_amd", "csrc"), "rangemath"])

    def run(text):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([DRIVER], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        return [np.asarray(line.split()[line.startswith(("w", "r")):], np.int64) for line in p.stdout.splitlines()]
    return run


def caller_order(rng, n):
    """order[k] = the caller's index of the k-th sorted range: stretches where the two orders agree, stretches that are
    reversed, and a shuffled rest -- so that runs of every length occur"""
    order = np.arange(n, dtype=np.int64)
    for _ in range(4):
        if n < 2:
            break
        a, b = sorted(rng.integers(0, n + 1, 2))
        order[a:b] = order[a:b][::-1] if rng.integers(2) else rng.permutation(order[a:b])
    return order


def restated_deal(n, order, nd, block):
    which = [order[(np.arange(n) // block) % nd == k] for k in range(nd)]
    runs = []
    for w in which:
        cut = np.flatnonzero(np.diff(w) != 1) + 1
        edges = np.concatenate([[0], cut, [len(w)]]) if len(w) else np.zeros(1, np.int64)
        runs.append(np.stack([edges[:-1], edges[1:]], 1).reshape(-1))
    return which, runs


@pytest.mark.parametrize("nd", [1, 2, 3, 8])
def test_shard_dealer_and_run_finder(driver, nd):
    rng = np.random.default_rng(100 + nd)
    cases = [(n, block, caller_order(rng, n)) for n in (0, 1, 7, 8 * nd - 1, 8 * nd, 4096 * nd * 8 + 1) for block in (1, 0)]
    lines = driver("".join(f"deal {n} {nd} {block}\n{' '.join(map(str, order))}\n" for n, block, order in cases))
    assert len(lines) == len(cases) * (1 + 2 * nd)
    for c, (n, block, order) in enumerate(cases):
        head, rest = lines[c * (1 + 2 * nd)], lines[c * (1 + 2 * nd) + 1:(c + 1) * (1 + 2 * nd)]
        want_block = block or max(1, min(n // (nd * 8), 4096))
        assert head[0] == want_block, (n, block)
        which, runs = rest[0::2], rest[1::2]
        want_which, want_runs = restated_deal(n, order, nd, want_block)
        for k in range(nd):
            assert np.array_equal(which[k], want_which[k]), (n, block, k)
            assert np.array_equal(runs[k], want_runs[k]), (n, block, k)
            # the runs partition the shard, each is consecutive in the caller's order, and none could be longer: a run
            # begins exactly where the caller's index does not follow its neighbour's
            r, w = runs[k].reshape(-1, 2), which[k]
            assert (len(r) == 0) == (len(w) == 0)
            if len(w):
                assert r[0, 0] == 0 and r[-1, 1] == len(w) and np.array_equal(r[1:, 0], r[:-1, 1])
                assert np.array_equal(r[1:, 0], np.flatnonzero(w[1:] != w[:-1] + 1) + 1)
        assert head[1] == sum(len(r) // 2 for r in runs)
        # every range dealt exactly once
        assert np.array_equal(np.sort(np.concatenate(which)), np.arange(n))


def restated_cut(cells, nd, budget):
    n, blocks = len(cells), []
    for k in range(nd):
        a, b = n * k // nd, n * (k + 1) // nd
        i = a
        while i < b:
            start, total = i, int(cells[i])
            i += 1
            while i < b and total + cells[i] <= budget:
                total += int(cells[i])
                i += 1
            blocks.append((k, start, i, total))
    return np.asarray(blocks, np.int64).reshape(-1, 4)


@pytest.mark.parametrize("nd", [1, 2, 3, 8])
def test_block_cutter(driver, nd):
    rng = np.random.default_rng(200 + nd)
    cells = rng.integers(0, 400, 61).astype(np.int64) * rng.integers(0, 2, 61)        # (ranges without width have no cells)
    one = int(cells.max())
    cases = [(budget, c) for budget in (one - 1, one, int(cells.sum()) + 1, 1) for c in (cells, cells[:nd - 1], cells[:0])]
    lines = driver("".join(f"cut {nd} {budget} {len(c)}\n{' '.join(map(str, c))}\n" for budget, c in cases))
    at = 0
    for budget, c in cases:
        count = int(lines[at][0])
        got = np.asarray(lines[at + 1:at + 1 + count], np.int64).reshape(-1, 4)
        shares = np.asarray(lines[at + 1 + count:at + 1 + count + nd], np.int64).reshape(nd, 2)
        at += 1 + count + nd
        assert np.array_equal(got, restated_cut(c, nd, budget)), (budget, len(c))
        assert np.array_equal(shares, [(len(c) * k // nd, len(c) * (k + 1) // nd) for k in range(nd)])
        for k in range(nd):
            mine = got[got[:, 0] == k]
            # the blocks tile the slot's share, in order
            assert (len(mine) == 0) == (shares[k, 0] == shares[k, 1])
            if len(mine):
                assert mine[0, 1] == shares[k, 0] and mine[-1, 2] == shares[k, 1] and np.array_equal(mine[1:, 1], mine[:-1, 2])
                assert np.all(mine[:, 2] > mine[:, 1])
            for _, a, b, total in mine:
                assert total == c[a:b].sum()
                assert total <= budget or b == a + 1                    # (a single larger range is a block of its own)
                assert b == shares[k, 1] or total + c[b] > budget       # (and no block could take one more range)
    assert at == len(lines)


def restated_cover(iv, queries):
    merged = []
    for rid, beg, end in sorted((t for t in iv if t[2] > t[1]), key=lambda t: t[:2]):
        if merged and merged[-1][0] == rid and beg <= merged[-1][2]:
            merged[-1][2] = max(merged[-1][2], end)
        else:
            merged.append([rid, beg, end])
    each = [int(end <= beg or any(m[0] == rid and m[1] <= beg and end <= m[2] for m in merged)) for rid, beg, end in queries]
    return merged, each


# touching intervals merge; a nested one adds nothing; an empty one covers nothing; the same coordinates on another
# reference are another place; negative starts occur (a range at the start of a reference, minus ext)
COVER_CASES = [
    ([(0, 100, 200), (0, 200, 300)], [(0, 100, 300), (0, 150, 250), (0, 99, 200), (0, 100, 301), (1, 100, 200)]),
    ([(0, 100, 500), (0, 200, 300), (0, 600, 700)], [(0, 200, 300), (0, 450, 500), (0, 450, 650), (0, 500, 600), (0, 600, 700)]),
    ([(0, 300, 300), (0, 400, 350)], [(0, 300, 300), (0, 300, 301), (0, 340, 360), (2, 5, 5)]),
    ([(1, 100, 200), (0, 100, 200), (2, -50, 80), (0, 150, 400)], [(0, 100, 400), (1, 100, 200), (1, 150, 400), (2, -50, 80), (2, -51, 0), (3, 0, 1)]),
    ([], [(0, 0, 1), (0, 5, 5)]),
    ([(0, 10, 20)], []),
]


def test_regions_covered(driver):
    rng = np.random.default_rng(300)
    cases = list(COVER_CASES)
    for _ in range(20):       # seeded: short intervals on three references, so that they touch, nest and miss by one
        m, q = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        draw = lambda k: [(int(r), int(b), int(b + w)) for r, b, w in zip(rng.integers(0, 3, k), rng.integers(-5, 60, k), rng.integers(-2, 25, k))]
        cases.append((draw(m), draw(q)))
    flat = lambda ts: " ".join(str(v) for t in ts for v in t)
    lines = driver("".join(f"cover {len(iv)} {flat(iv)}\n{len(qs)} {flat(qs)}\n" for iv, qs in cases))
    assert len(lines) == 2 * len(cases)
    for c, (iv, qs) in enumerate(cases):
        merged, each = restated_cover(iv, qs)
        assert lines[2 * c].tolist() == [len(merged)] + [v for m in merged for v in m], c
        assert lines[2 * c + 1].tolist() == each + [int(all(each))], c
    # the hand-written cases say what they were written for
    assert restated_cover(*COVER_CASES[0]) == ([[0, 100, 300]], [1, 1, 0, 0, 0])
    assert restated_cover(*COVER_CASES[1])[1] == [1, 1, 0, 0, 1]
    assert restated_cover(*COVER_CASES[2]) == ([], [1, 0, 0, 1])
