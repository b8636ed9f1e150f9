"""CPU: the arithmetic of plan creation (csrc/planmath.h) under AddressSanitizer + UndefinedBehaviorSanitizer.

`make -C bamsignals_amd/csrc planmath` builds tests/asan/planmath_driver.cpp, a program of its own that includes that
header and nothing else of the library.  Cases go through it on standard input; its answers are compared with a
restatement in numpy / plain Python written here, and checked for what must hold whatever the restatement says: tiles
partition their ranges, a parameter rule is true at its limit and false one past it, slices partition the windows of a
heavy tile, runs partition the tiles inside their bounds."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import test_short_half_cpu as short_half

DRIVER = os.path.join(ROOT, "tests", "asan", "planmath_driver")
PROFILE, COUNT, COVERAGE = 0, 1, 2
HEAVY, NEG, ATOMIC, UNITS = 1 << 29, 1 << 30, 1 << 31, 0x0FFFFFFF
LIMIT = (1 << 15) - 256         # 32,512: what a tile's window may span for the 16-bit columns


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bamsignals_amd", "csrc"), "planmath"])

    def run(text):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([DRIVER], input=text, capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        return [[int(v) for v in line.split()] for line in p.stdout.splitlines()]
    return run


def rule(mode, cov_ex=0, binsize=1, ss=0, mid=0, tspan=0, frag_len=0, ext=0, overlap=0, minoverlap=0):
    return dict(mode=mode, cov_ex=cov_ex, binsize=binsize, ss=ss, mid=mid, tspan=tspan, frag_len=frag_len, ext=ext,
                lay_binsize=-1 if mode == COUNT else binsize, overlap=overlap, minoverlap=minoverlap)


def kind(sum=0, xcorr=0, body=0, lag=0, frag=0, len_bin=0, own=0, row=0):
    return dict(sum=sum, xcorr=xcorr, body=body, lag=lag, frag=frag, len_bin=len_bin, own=own, row=row)


def words(*parts):
    out = []
    for p in parts:
        out += [int(v) for v in (p.values() if isinstance(p, dict) else np.ravel(p))]
    return " ".join(map(str, out))


# ---------------------------------------------------------------------------------------------------------------
# tile size
# ---------------------------------------------------------------------------------------------------------------
def restated_tile(r, k, caller, lens):
    widest = 64 if r["mode"] == COUNT else max([64] + [(w + r["binsize"] - 1) // r["binsize"] for w in lens])
    binned = r["mode"] == PROFILE or r["cov_ex"]
    split = binned and r["ss"]
    cells, floor = caller if caller > 0 else min(widest, 1024 if split else 2048), 64
    if binned and r["binsize"] > 1 and caller <= 0:
        cells, floor = min(cells, max(4, -(-16384 // r["binsize"]))), 4
    cells = (min(max(cells, floor), 4096 if split else 8192) + 3) & ~3
    xbody = min(k["body"], widest) if k["xcorr"] else 0
    if k["xcorr"]:
        cells = (xbody + k["lag"] + 3) & ~3
    if k["own"]:
        cells = (k["own"] + 3) & ~3
    return cells, xbody


# (rule, kind, caller's tile_cells, widths, the tile size): one case on each side of every rule
TILE_CASES = [
    (rule(PROFILE), kind(), 0, [10, 63], 64), (rule(PROFILE), kind(), 0, [65], 68),              # the widest range, from 64 cells on
    (rule(PROFILE), kind(), 0, [2048], 2048), (rule(PROFILE), kind(), 0, [2049, 5], 2048),       # ... up to 2,048
    (rule(PROFILE, ss=1), kind(), 0, [1024], 1024), (rule(PROFILE, ss=1), kind(), 0, [1025], 1024),   # ... 1,024 with strands
    (rule(COVERAGE), kind(), 0, [3000], 2048), (rule(COVERAGE, cov_ex=1, ss=1), kind(), 0, [3000], 1024),
    (rule(COUNT, ss=1), kind(), 0, [40_000], 64),                                                # bamCount: no cells to size
    (rule(PROFILE), kind(), 100, [5000], 100), (rule(PROFILE), kind(), 10, [5000], 64),          # the caller's value, its floor
    (rule(PROFILE), kind(), 8192, [5], 8192), (rule(PROFILE), kind(), 9000, [5], 8192),          # ... its cap
    (rule(PROFILE, ss=1), kind(), 4096, [5], 4096), (rule(PROFILE, ss=1), kind(), 4097, [5], 4096),   # ... with strands
    (rule(PROFILE), kind(), 101, [5], 104),                                                      # rounded up to 4
    (rule(PROFILE, binsize=2), kind(), 0, [100_000], 2048), (rule(PROFILE, binsize=8), kind(), 0, [100_000], 2048),
    (rule(PROFILE, binsize=9), kind(), 0, [100_000], 1824),                                      # 16 kbp a tile: ceil(16384 / 9) = 1821
    (rule(COVERAGE, cov_ex=1, binsize=274, ss=1), kind(), 0, [100_000], 60),
    (rule(PROFILE, binsize=5461), kind(), 0, [100_000], 4), (rule(PROFILE, binsize=5462), kind(), 0, [100_000], 4),   # ... 4 at least
    (rule(PROFILE, binsize=4096), kind(), 0, [100_000], 4), (rule(PROFILE, binsize=4095), kind(), 0, [1_000_000], 8),
    (rule(PROFILE, binsize=7), kind(), 0, [100], 64),                                            # the floor of 4 is no floor of 64 ...
    (rule(PROFILE, binsize=300), kind(), 0, [3000], 56), (rule(PROFILE, binsize=300), kind(), 10, [3000], 64),   # ... but a caller's has it
    (rule(COVERAGE, binsize=1), kind(), 0, [100], 100),
    (rule(PROFILE, ss=1), kind(xcorr=1, body=2048, lag=200), 2048, [4099], 2248),                # body + halo
    (rule(PROFILE, ss=1), kind(xcorr=1, body=2048, lag=200), 2048, [100, 7], 300),               # ... a body no wider than the widest
    (rule(PROFILE, ss=1), kind(xcorr=1, body=16, lag=0), 16, [4099], 16), (rule(PROFILE, ss=1), kind(xcorr=1, body=16, lag=31), 16, [9], 48),
    (rule(PROFILE, ss=1), kind(own=18), 18, [4099], 20), (rule(COVERAGE), kind(own=2048), 2048, [5], 2048),   # hist
    (rule(COVERAGE), kind(own=16, row=1), 16, [4099], 16), (rule(PROFILE), kind(own=257, row=1), 257, [9], 260),   # summary, scaled
]


def test_tile_size(driver):
    got = driver("".join(f"tilesize {words(r, k, [caller, len(w)], w)}\n" for r, k, caller, w, _ in TILE_CASES))
    assert len(got) == len(TILE_CASES)
    for (r, k, caller, w, want), g in zip(TILE_CASES, got):
        assert tuple(g) == restated_tile(r, k, caller, w), (r, k, caller, w)
        assert g[0] == want and g[0] % 4 == 0, (r, k, caller, w, g)
    assert got[-8][1] == 2048 and got[-7][1] == 100          # the xcorr bodies


# ---------------------------------------------------------------------------------------------------------------
# kernel parameters
# ---------------------------------------------------------------------------------------------------------------
def layout(c0=(1000, 256, 9, 1, 4096), c1=(500, 4096, 11, 1, 8192), packed=(50_000, 256, 9, 1, 0)):
    """(n, maxspan, kshift, has a 16-bit column, its offset) per class"""
    return [c0, c1, (10, 65_536, 13, 0, 0), (1, 70_000, 14, 0, 0), packed]


def kparams_line(r, k=None, caller=0, tile=2048, quad_off=0, mapqual=0, requiredF=0, filteredF=-1, tf=(), shift=0, lay=None, codes=(0, 16)):
    tf2 = list(tf) + [0] * (2 - len(tf))
    return "kparams " + words(r, k or kind(), [caller, tile, quad_off, mapqual, requiredF, filteredF, len(tf)], tf2, [shift],
                              lay or layout(), [len(codes)], codes) + "\n"


FIELDS = ("rel24", "packed_half", "short_half", "off0", "off1", "win0", "win1", "div_magic", "div_shift", "div_m15", "div_s15", "use_tlen",
          "shift", "overlap_wide")


def kparams(driver, **kw):
    r = kw.pop("r", None) or rule(PROFILE, ext=abs(kw.get("shift", 0)))
    (line,) = driver(kparams_line(r, **kw))
    return dict(zip(FIELDS, line))


def test_rel24_is_true_at_its_limit_and_false_one_past_it(driver):
    for sign in (1, -1):
        assert kparams(driver, shift=sign * 4_177_791)["rel24"] == 1
        assert kparams(driver, shift=sign * 4_177_792)["rel24"] == 0
    # with the midpoint rule: 2 |shift| + tlen_filter[1] / 2 at 8,355,583 and 8,355,584
    mid = rule(PROFILE, mid=1)
    for shift, tf1, want in ((1000, 16_707_167, 1), (1000, 16_707_168, 0), (-1000, 16_707_166, 1), (0, 16_711_167, 1), (0, 16_711_168, 0)):
        assert 2 * abs(shift) + tf1 // 2 == (8_355_583 if want else 8_355_584)
        assert kparams(driver, r=mid, shift=shift, tf=(0, tf1))["rel24"] == want, (shift, tf1)
    # no midpoint rule: the filter's upper end does not count; a negative one counts as 0
    assert kparams(driver, shift=4_177_791, tf=(0, 1 << 30))["rel24"] == 1
    assert kparams(driver, r=mid, shift=4_177_791, tf=(-10, -5))["rel24"] == 1
    # coverage has no shift
    got = kparams(driver, r=rule(COVERAGE), shift=4_177_792)
    assert got["rel24"] == 1 and got["shift"] == 0


def test_packed_half_rule(driver):
    span, k = 256, 9
    room = LIMIT - span - 2 * (1 << k)          # tile + 2 ext at the limit
    lay = layout(c0=(0, 0, 0, 0, 0), c1=(0, 0, 0, 0, 0))
    for tile, ext, want in ((room, 0, 1), (room + 1, 0, 0), (room - 150, 75, 1), (room - 149, 75, 0)):
        assert tile + 2 * ext + span + 2 * (1 << k) == (LIMIT if want else LIMIT + 1)
        assert kparams(driver, r=rule(PROFILE, ext=ext), tile=tile, lay=lay)["packed_half"] == want, (tile, ext)
    ok = dict(tile=2048, lay=lay)
    assert kparams(driver, **ok)["packed_half"] == 1
    # one rejected code among the table's: by mapq, by a required flag, by a filtered flag
    assert kparams(driver, mapqual=10, codes=(0 | 30 << 16, 16 | 30 << 16), **ok)["packed_half"] == 1
    assert kparams(driver, mapqual=10, codes=(0 | 30 << 16, 16 | 9 << 16, 99 | 30 << 16), **ok)["packed_half"] == 0
    assert kparams(driver, requiredF=2, codes=(99, 83), **ok)["packed_half"] == 1
    assert kparams(driver, requiredF=2, codes=(99, 83, 16), **ok)["packed_half"] == 0
    assert kparams(driver, filteredF=0x400, codes=(0, 16), **ok)["packed_half"] == 1
    assert kparams(driver, filteredF=0x400, codes=(0, 0x400), **ok)["packed_half"] == 0
    assert kparams(driver, codes=(), **ok)["packed_half"] == 1
    # bins of two bases, a template-length rule, another mode, no column
    assert kparams(driver, r=rule(PROFILE, binsize=2), **ok)["packed_half"] == 0
    assert kparams(driver, tf=(0, 500), **ok)["packed_half"] == 0
    assert kparams(driver, r=rule(PROFILE, mid=1), **ok)["packed_half"] == 0
    assert kparams(driver, r=rule(COVERAGE), **ok)["packed_half"] == 0
    assert kparams(driver, tile=2048, lay=layout(c0=(0, 0, 0, 0, 0), c1=(0, 0, 0, 0, 0), packed=(50_000, 256, 9, 0, 0)))["packed_half"] == 0


def test_short_half_rule(driver):
    def got(tile, ext, c0, c1, **kw):
        return kparams(driver, r=rule(PROFILE, ext=ext), tile=tile, lay=layout(c0=c0, c1=c1, packed=(50_000, 1, 4, 1, 0)), **kw)
    # either class at 32,512 and 32,513, against tests/test_short_half_cpu.py's rule
    for cls in (0, 1):
        span, k = (256, 9) if cls == 0 else (4096, 11)
        other = (7, 5, 4, 1, 64)
        for ext in (0, 75):
            room = LIMIT - 2 * ext - 2 * (span - 1) - 2 * (1 << k)
            for tile, want in ((room, 1), (room + 1, 0)):
                assert short_half.rule(tile, ext, span, k) == bool(want)
                mine = (1000, span, k, 1, 4096)
                g = got(tile, ext, mine if cls == 0 else other, other if cls == 0 else mine)
                assert g["packed_half"] == 1 and g["short_half"] == want, (cls, ext, tile)
                wins = [g["win0"], g["win1"]]
                if want:
                    assert wins[cls] == (ext + span - 1) << 5 | k and wins[1 - cls] == (ext + 4) << 5 | 4
                    assert [g["off0"], g["off1"]][cls] == 4096 and [g["off0"], g["off1"]][1 - cls] == 64
                else:
                    assert wins == [0, 0] and g["off0"] == g["off1"] == 0
    # seeded cases: the C++ rule and the numpy one agree
    rng = np.random.default_rng(11)
    cases = [(int(rng.choice([64, 500, 2048, 8192, 20_000])), int(rng.choice([0, 75, 5000, 11_000])), int(rng.choice([1, 100, 256])),
              int(rng.integers(4, 14)), int(rng.choice([257, 2100, 4096])), int(rng.integers(4, 14))) for _ in range(200)]
    lines = driver("".join(kparams_line(rule(PROFILE, ext=ext), tile=tile, lay=layout((9, s0, k0, 1, 8), (9, s1, k1, 1, 16), (9, 1, 4, 1, 0)))
                           for tile, ext, s0, k0, s1, k1 in cases))
    seen = set()
    for (tile, ext, s0, k0, s1, k1), line in zip(cases, lines):
        g = dict(zip(FIELDS, line))
        assert g["packed_half"] == int(tile + 2 * ext + 1 + 32 <= LIMIT)
        want = bool(g["packed_half"]) and short_half.rule(tile, ext, s0, k0) and short_half.rule(tile, ext, s1, k1)
        assert g["short_half"] == int(want)
        assert (g["win1"] != 0) == want and (g["win0"] != 0) == want
        seen.add(want)
    assert seen == {False, True}
    # an empty class is skipped, whatever it says of itself, and its window word is not 0
    g = got(2048, 0, (1000, 256, 9, 1, 4096), (0, 1 << 20, 20, 0, 0))
    assert g["short_half"] == 1 and g["win1"] == 4 and g["off1"] == 0 and g["win0"] == 255 << 5 | 9
    g = got(2048, 0, (0, 0, 0, 0, 0), (0, 0, 0, 0, 0))
    assert g["short_half"] == 1 and g["win0"] == g["win1"] == 4
    # a class with reads and no column
    assert got(2048, 0, (1000, 256, 9, 0, 0), (0, 0, 0, 0, 0))["short_half"] == 0
    # a filter that could reject a read: the packed column still serves (no code is rejected), the classes' do not
    full = ((1000, 256, 9, 1, 4096), (500, 4096, 11, 1, 8192))
    assert got(2048, 0, *full)["short_half"] == 1
    for kw in (dict(mapqual=1, codes=(30 << 16,)), dict(requiredF=1, codes=(99, 83)), dict(filteredF=0xFFFF), dict(filteredF=0x400)):
        g = got(2048, 0, *full, **kw)
        assert g["packed_half"] == 1 and g["short_half"] == 0 and g["win1"] == 0, kw
    assert got(2048, 0, *full, filteredF=0x10000)["short_half"] == 1


def restated_magic(d):
    if d < 2:
        return 0, 0
    s = (d - 1).bit_length()
    return -(-(1 << (31 + s)) // d), s - 1


def test_division_multipliers(driver):
    assert driver("div15\n") == [[1]]           # every binsize 2 .. 8192 at every multiple below 2^15, checked in the driver
    for b in (-1, 1, 2, 3, 7, 274, 4096, 8191, 8192, 8193, 65_536):
        g = kparams(driver, r=rule(PROFILE, binsize=b))
        s = 15 + (b - 1).bit_length()
        assert (g["div_m15"], g["div_s15"]) == ((-(-(1 << s) // b), s) if 2 <= b <= 8192 else (0, 0)), b
        assert (g["div_magic"], g["div_shift"]) == restated_magic(b), b
    # a frag plan's tiles divide by the row width
    g = kparams(driver, r=rule(COUNT), k=kind(frag=1, len_bin=7))
    assert (g["div_magic"], g["div_shift"]) == restated_magic(7) and g["div_m15"] == 0


def test_the_other_parameters(driver):
    assert kparams(driver)["use_tlen"] == 0 and kparams(driver, tf=(0, 9))["use_tlen"] == 1
    assert kparams(driver, r=rule(COVERAGE, tspan=1))["use_tlen"] == 1 and kparams(driver, r=rule(PROFILE, mid=1))["use_tlen"] == 1
    assert kparams(driver, r=rule(COVERAGE, frag_len=150, ext=149))["use_tlen"] == 0
    ov = rule(COUNT, overlap=1, minoverlap=1)
    assert kparams(driver, r=ov, quad_off=1)["overlap_wide"] == 1 and kparams(driver, r=ov)["overlap_wide"] == 0
    assert kparams(driver, r=rule(COUNT), quad_off=1)["overlap_wide"] == 0


# ---------------------------------------------------------------------------------------------------------------
# tiles
# ---------------------------------------------------------------------------------------------------------------
REF_LEN = (300_000, 65_536, 65_537)
REF_UNITS = [(n + 65_535) >> 16 for n in REF_LEN]
REF_UNIT0 = [0, 5, 6]


def layout_offsets(r, lens):
    mult = 2 if r["ss"] else 1
    per = [mult if r["lay_binsize"] <= 0 else (mult * -(-w // r["lay_binsize"]) if w > 0 else 0) for w in lens]
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def some_ranges(widths, seed):
    """every width three times, once per strand, in a seeded order on three references, with duplicates"""
    rng = np.random.default_rng(seed)
    w = rng.permutation(np.repeat(np.asarray(widths, np.int64), 3))
    n = len(w)
    rid = rng.integers(0, 3, n)
    loc = (rng.random(n) * np.maximum(np.asarray(REF_LEN)[rid] - w, 1)).astype(np.int64) - 3
    strand = np.asarray([1, -1, 0])[np.arange(n) % 3]
    rid[-2:], loc[-2:], w[-2:] = rid[:2], loc[:2], w[:2]                 # two duplicates, other strands
    return dict(rid=rid, loc=loc, len=w, strand=strand)


def restated_tiles(r, k, caller, rg, off):
    cells_t, xbody = restated_tile(r, k, caller, rg["len"].tolist())
    mult, whole = (2 if r["ss"] else 1), 1 << 14
    split = min(max(caller, 16), whole) if (k["frag"] or r["overlap"]) and caller > 0 else whole
    wide = r["mode"] == PROFILE and caller <= 0 and r["binsize"] > split // 2
    items, zero = [], False
    for i in sorted(range(len(rg["len"])), key=lambda i: (rg["rid"][i], rg["loc"][i], i)):
        w, neg = int(rg["len"][i]), rg["strand"][i] < 0
        if w <= 0:
            zero |= bool(off[i + 1] > off[i])
            continue
        head = (int(rg["loc"][i]), w)
        tail = (REF_UNIT0[rg["rid"][i]], REF_UNITS[rg["rid"][i]] | (NEG if neg else 0))
        cells = int(off[i + 1] - off[i]) // mult
        if wide:
            zero = True
            for c in range(cells):
                ra, rb = c * r["binsize"], min(w, (c + 1) * r["binsize"])
                g0, g1 = (w - rb, w - ra) if neg else (ra, rb)
                items += [head + (a, min(split, g1 - a), int(off[i]) + c * mult, tail[0], tail[1] | ATOMIC) for a in range(g0, g1, split)]
        elif r["mode"] == COUNT:
            zero |= w > split
            items += [head + (a, min(split, w - a), int(off[i]), tail[0], tail[1] | (ATOMIC if w > split else 0)) for a in range(0, w, split)]
        elif k["xcorr"]:
            for c0 in range(0, w, xbody):
                nb = min(xbody, w - c0)
                items.append(head + (c0, nb + min(k["lag"], w - c0 - nb), nb) + tail)
        else:
            items += [head + (c0, min(cells_t, cells - c0), i * mult if k["row"] else int(off[i]) + c0 * mult) + tail
                      for c0 in range(0, cells, cells_t)]
    if k["sum"]:
        items.sort(key=lambda it: it[2])
    return [cells_t, xbody, COUNT if wide else r["mode"], int(zero), len(items)], items


def cut(driver, r, k, caller, rg):
    off = layout_offsets(r, rg["len"].tolist())
    n = len(rg["len"])
    text = "tiles " + words(r, k, [caller, 3], np.stack([REF_UNIT0, REF_UNITS], 1), [n],
                            np.stack([rg["rid"], rg["loc"], rg["len"], rg["strand"]], 1), off) + "\n"
    got = driver(text)
    head, items = got[0], [tuple(g) for g in got[1:]]
    want_head, want_items = restated_tiles(r, k, caller, rg, off)
    assert head == want_head and head[4] == len(items)
    assert items == want_items
    for loc, w, c0, nc, out_off, unit0, flags in items:
        assert nc > 0 and c0 >= 0 and flags & HEAVY == 0
    return head, items, off


def owner_of(off, out_off):
    """the range a cell of the flat layout belongs to (ranges without cells own none)"""
    return int(np.searchsorted(off, out_off, side="right")) - 1


def widths_for(t):
    return [0, 1, t - 1, t, t + 1, 2 * t + 3]


@pytest.mark.parametrize("t,r,k,caller", [
    (4, rule(PROFILE, binsize=4096), kind(), 0), (4, rule(COVERAGE, cov_ex=1, binsize=5000, ss=1), kind(), 0),
    (64, rule(PROFILE, ss=1), kind(), 64), (64, rule(COVERAGE), kind(), 64), (64, rule(PROFILE, binsize=3), kind(), 64),
    (2048, rule(PROFILE), kind(), 0), (2048, rule(COVERAGE), kind(), 2048), (2048, rule(PROFILE, ss=1), kind(own=2048), 2048),
    (64, rule(PROFILE, ss=1), kind(own=64, row=1), 64), (2048, rule(COVERAGE), kind(own=2048, row=1), 2048), (4, rule(COVERAGE), kind(own=4, row=1), 4)])
def test_cell_tiles_partition_every_range(driver, t, r, k, caller):
    b = r["binsize"]
    rg = some_ranges([max(c * b - (b // 2), min(c, 1)) for c in widths_for(t)], seed=t + b)      # (c cells: the last bin a part of one)
    head, items, off = cut(driver, r, k, caller, rg)
    S = 2 if r["ss"] else 1
    assert head[0] == t and head[2] == r["mode"] and head[3] == 0        # no zeroing: every cell is written, a range without width has none
    seen = np.zeros(int(off[-1]) // S, np.int64)
    for loc, w, c0, nc, out_off, unit0, flags in items:
        i = out_off // S if k["row"] else owner_of(off, out_off)
        assert out_off == (i * S if k["row"] else off[i] + c0 * S)
        assert (loc, w) == (rg["loc"][i], rg["len"][i]) and unit0 == REF_UNIT0[rg["rid"][i]] and flags & UNITS == REF_UNITS[rg["rid"][i]]
        assert bool(flags & NEG) == (rg["strand"][i] < 0) and not flags & ATOMIC
        assert nc <= t and c0 % t == 0
        seen[off[i] // S + c0:off[i] // S + c0 + nc] += 1
    assert np.all(seen == 1) and len(seen) == sum(-(-int(w) // b) for w in rg["len"])
    assert {it[3] for it in items} >= {1, t - 1, t, 3}                    # part tiles and whole ones occurred


@pytest.mark.parametrize("ss", [0, 1])
def test_count_tiles_partition_every_range(driver, ss):
    rg = some_ranges([0, 1, 16_383, 16_384, 16_385, 40_000], seed=3)
    head, items, off = cut(driver, rule(COUNT, ss=ss), kind(), 0, rg)
    S = ss + 1
    covered = {}
    for loc, w, c0, nc, out_off, unit0, flags in items:
        i = out_off // S
        assert out_off == off[i] and (loc, w) == (rg["loc"][i], rg["len"][i]) and bool(flags & NEG) == (rg["strand"][i] < 0)
        assert bool(flags & ATOMIC) == (w > 16_384) and nc <= 16_384
        covered.setdefault(i, []).append((c0, c0 + nc))
    for i, w in enumerate(rg["len"]):
        parts = sorted(covered.get(i, []))
        assert (len(parts) > 1) == (w > 16_384) and (len(parts) == 0) == (w == 0)
        if parts:
            assert parts[0][0] == 0 and parts[-1][1] == w and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert head[3] == 1                                                   # split ranges, and ranges without width that own cells
    # needs_zero exactly when a range is split or has no width
    for widths, want in (([1, 16_384], 0), ([1, 16_385], 1), ([0, 5], 1)):
        one = dict(rid=np.zeros(2, np.int64), loc=np.asarray([5, 9]), len=np.asarray(widths), strand=np.ones(2, np.int64))
        assert cut(driver, rule(COUNT, ss=ss), kind(), 0, one)[0][3] == want, widths
    # a zero-width range of a profile owns no cell: nothing to zero, no tile
    one = dict(rid=np.zeros(1, np.int64), loc=np.asarray([5]), len=np.asarray([0]), strand=np.ones(1, np.int64))
    assert cut(driver, rule(PROFILE), kind(), 0, one)[0][3:] == [0, 0] and cut(driver, rule(COUNT), kind(), 0, one)[0][3:] == [1, 0]
    # an overlap plan's and a frag plan's tile_cells: bases per tile, 16 at least; anybody else's does not count
    long = dict(rid=np.zeros(1, np.int64), loc=np.asarray([5]), len=np.asarray([1000]), strand=np.ones(1, np.int64))
    assert cut(driver, rule(COUNT, overlap=1, minoverlap=1), kind(), 100, long)[0][4] == 10
    assert cut(driver, rule(COUNT), kind(frag=1, len_bin=1), 7, long)[0][4] == 63
    assert cut(driver, rule(COUNT), kind(), 100, long)[0][4] == 1


def test_wide_bins_become_count_tiles(driver):
    rg = some_ranges([0, 1, 8193, 40_000, 100_000], seed=9)
    head, _, _ = cut(driver, rule(PROFILE, binsize=8192, ss=1), kind(), 0, rg)
    assert head[2] == PROFILE and head[3] == 0
    assert cut(driver, rule(PROFILE, binsize=8193, ss=1), kind(), 8, rg)[0][2] == PROFILE          # a caller's tile_cells keeps the profile
    for b in (8193, 20_000, 40_000):
        head, items, off = cut(driver, rule(PROFILE, binsize=b, ss=1), kind(), 0, rg)
        assert head[2] == COUNT and head[3] == 1
        covered = {}
        for loc, w, c0, nc, out_off, unit0, flags in items:
            i = owner_of(off, out_off)
            assert (out_off - off[i]) % 2 == 0 and flags & ATOMIC and nc <= 16_384
            assert (loc, w) == (rg["loc"][i], rg["len"][i]) and bool(flags & NEG) == (rg["strand"][i] < 0)
            covered.setdefault((i, (out_off - off[i]) // 2), []).append((c0, c0 + nc))
        bins = 0
        for i, w in enumerate(rg["len"]):
            for c in range(-(-int(w) // b)):
                ra, rb = c * b, min(w, (c + 1) * b)
                g0, g1 = (w - rb, w - ra) if rg["strand"][i] < 0 else (ra, rb)         # mirrored on the '-' strand
                parts = sorted(covered[(i, c)])
                assert parts[0][0] == g0 and parts[-1][1] == g1 and all(x[1] == y[0] for x, y in zip(parts, parts[1:]))
                bins += 1
        assert bins == len(covered)
        assert (max(len(v) for v in covered.values()) > 1) == (b > 16_384)


@pytest.mark.parametrize("body,lag", [(64, 0), (64, 31), (64, 200), (2048, 200), (16, 2047)])
def test_xcorr_tiles(driver, body, lag):
    rg = some_ranges(widths_for(body) + [9], seed=body + lag)
    head, items, off = cut(driver, rule(PROFILE, ss=1), kind(xcorr=1, body=body, lag=lag), body, rg)
    assert head[:2] == [(body + lag + 3) & ~3, body]
    order = [i for i in sorted(range(len(rg["len"])), key=lambda i: (rg["rid"][i], rg["loc"][i], i)) if rg["len"][i] > 0]
    it = iter(items)
    for i in order:
        at, w = 0, int(rg["len"][i])
        while at < w:                                                       # the bodies partition the range ...
            loc, wi, c0, nc, nb, unit0, flags = next(it)
            assert (loc, wi, c0) == (rg["loc"][i], w, at) and nb == min(body, w - at)
            assert nc == nb + min(lag, w - at - nb) and nc <= head[0]      # ... and the halo is what the range still has
            at += nb
    assert next(it, None) is None


def test_sum_tiles_are_ordered_by_c0_then_genomic(driver):
    rng = np.random.default_rng(5)
    n = 40
    rid = rng.integers(0, 3, n)
    rg = dict(rid=rid, loc=rng.integers(-5, 60_000, n), len=np.full(n, 2048 + 2048 + 5), strand=rng.choice([1, -1, 0], n))
    rg["loc"][-3:], rg["rid"][-3:] = rg["loc"][:3], rg["rid"][:3]
    for r, t in ((rule(PROFILE, ss=1), 1024), (rule(COVERAGE), 2048)):
        head, items, off = cut(driver, r, kind(sum=1), 0, rg)
        assert head[0] == t
        keys = [(c0, unit0, loc) for loc, w, c0, nc, out_off, unit0, flags in items]
        assert keys == sorted(keys) and len(items) == n * -(-4101 // t)
        for c0 in {k[0] for k in keys}:
            assert len({it[3] for it in items if it[2] == c0}) == 1          # one nc per c0
        # ... and the order among tiles of one c0 and one place is the caller's (a stable sort): out_off tells them apart
        same = {}
        for loc, w, c0, nc, out_off, unit0, flags in items:
            same.setdefault((c0, unit0, loc), []).append(out_off)
        assert all(v == sorted(v) for v in same.values()) and any(len(v) > 1 for v in same.values())


# ---------------------------------------------------------------------------------------------------------------
# tile loads, the depth bound, the heavy split
# ---------------------------------------------------------------------------------------------------------------
def windows_with(rng, total):
    """five class windows that hold `total` reads between them, some of them empty"""
    cut = np.sort(rng.integers(0, total + 1, 4))
    size = np.diff(np.concatenate([[0], cut, [total]]))
    lo = rng.integers(0, 1 << 20, 5)
    return np.stack([lo, lo + size], 1)


@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("count_mode", [0, 1])
@pytest.mark.parametrize("heavy_reads", [4, 64, 32_768])
def test_heavy_split(driver, heavy_reads, count_mode, policy):
    rng = np.random.default_rng(heavy_reads + policy)
    slice_reads = max(4, heavy_reads // 4) if heavy_reads < 32_768 else 8192
    totals = [0, 1, heavy_reads - 1, heavy_reads, heavy_reads + 1, heavy_reads, 3 * heavy_reads + 2, heavy_reads + 1, 10 * heavy_reads]
    win = [windows_with(rng, t) for t in totals]
    win[4] = np.asarray([[7, 7], [0, 0], [100, 100 + heavy_reads + 1], [5, 5], [9, 9]])          # all of it in one class
    nc = rng.integers(1, 2049, len(totals))
    for coverage in (0, 1):
        got = driver("heavy " + words([heavy_reads, slice_reads, policy, count_mode, coverage, len(totals)],
                                      np.concatenate([nc[:, None], np.asarray(win).reshape(len(totals), 10)], 1)) + "\n")
        assert got[0] == totals
        assert got[1] == [int(sum(t * c for t, c in zip(totals, nc))) if coverage else sum(totals)]
    heavy = [t for t, total in enumerate(totals) if total > heavy_reads]              # exactly at the threshold: not heavy
    assert got[2][0] == len(heavy) == 4 and got[2][1] == sum(totals[t] ** 2 for t in heavy)
    assert got[3] == [HEAVY if t in heavy else 0 for t in range(len(totals))]
    hitems = got[4:]
    assert got[2][2] == len(hitems)
    if policy == 1:                                                                     # walked whole: the item, no windows
        assert hitems == [[t, 0] for t in heavy]
        return
    want = []
    for t in heavy:
        for c in range(5):
            for j0 in range(int(win[t][c][0]), int(win[t][c][1]), slice_reads):
                row = [0] * 10
                row[2 * c:2 * c + 2] = [j0, min(j0 + slice_reads, int(win[t][c][1]))]
                want.append([t, ATOMIC if count_mode else 0] + row)
    assert hitems == want
    for t in heavy:                                                                     # whatever the restatement says:
        mine = [np.asarray(h[2:]).reshape(5, 2) for h in hitems if h[0] == t]
        for c in range(5):
            parts = [tuple(m[c]) for m in mine if m[c][1] > m[c][0]]
            lo, hi = win[t][c]
            assert (len(parts) == 0) == (hi == lo)                                      # the slices partition every class window ...
            if parts:
                assert parts[0][0] == lo and parts[-1][1] == hi and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
                assert all(b - a == slice_reads for a, b in parts[:-1]) and 0 < parts[-1][1] - parts[-1][0] <= slice_reads
        assert all(sum(m[c][1] > m[c][0] for c in range(5)) == 1 for m in mine)         # ... one non-empty window a slice
        assert all(m[c][0] == m[c][1] == 0 for m in mine for c in range(5) if m[c][1] <= m[c][0])


# ---------------------------------------------------------------------------------------------------------------
# run cutters
# ---------------------------------------------------------------------------------------------------------------
def restated_runs(weight, per, ceiling):
    runs, a, total = [], 0, 0
    for t, w in enumerate(weight):
        if t > a and (t - a >= per or total + w > ceiling):
            runs.append((a, t))
            a, total = t, 0
        total += w
    return runs + ([(a, len(weight))] if a < len(weight) else [])


def test_cut_runs(driver):
    rng = np.random.default_rng(21)
    cases = []
    for n in (0, 1, 7, 200):
        weight = rng.integers(0, 50, n)
        weight[n // 2:n // 2 + 2] = 1000                                                # above every ceiling but the last
        for per in (1, 3, 1 << 40):
            for ceiling in (0, 1, 120, 4294967295):
                cases.append((weight.tolist(), per, ceiling, int(rng.integers(0, 4))))
    got = driver("".join(f"runs {per} {ceiling} {n_wide} {len(w)} {words(w)}\n" for w, per, ceiling, n_wide in cases))
    for (w, per, ceiling, n_wide), g in zip(cases, got):
        runs = [tuple(p) for p in np.asarray(g, np.int64).reshape(-1, 2)]
        main, wide = runs[:len(runs) - n_wide], runs[len(runs) - n_wide:]
        assert main == restated_runs(w, per, ceiling), (per, ceiling)
        assert wide == [(k, k + 1) for k in range(n_wide)]                              # the wide tiles: runs of one
        assert (len(main) == 0) == (len(w) == 0)
        if main:                                                                        # the runs partition the tiles
            assert main[0][0] == 0 and main[-1][1] == len(w) and all(a[1] == b[0] for a, b in zip(main, main[1:]))
        for a, b in main:
            assert 0 < b - a <= per                                                     # no run longer than per
            assert sum(w[a:b]) <= ceiling or b == a + 1                                 # none over the ceiling unless one tile is
        for t, x in enumerate(w):
            if x > ceiling:
                assert (t, t + 1) in main                                               # a tile above the ceiling stands alone


def restated_sum_runs(parts, per, S):
    runs, chunks, most, n_main = [], [], 0, 0
    for part in parts:
        last, a = None, 0
        while a < len(part):
            b = a
            while b < len(part) and part[b][0] == part[a][0]:
                b += 1
            for r in range(a, b, per):
                runs.append((r, min(b, r + per)))
                if last != part[a][0] or chunks[-1][1] - chunks[-1][0] >= 32:
                    chunks.append([len(runs) - 1, len(runs) - 1, part[a][0] * S, part[a][1] * S])
                    last = part[a][0]
                chunks[-1][1] = len(runs)
                most = max(most, part[a][1] * S)
            a = b
        n_main = n_main or len(runs)
    return n_main, runs, [tuple(c) for c in chunks], most


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("per", [1, 4, 65_536])
def test_cut_sum_runs(driver, per, S):
    main = [(c0, 1024 if c0 < 2048 else 5) for c0 in (0, 1024, 2048) for _ in range({0: 70, 1024: 3, 2048: 133}[c0])]
    heavy = [(c0, 1024) for c0 in (0, 0, 0, 1024)]
    (n_main,), runs, chunks, (most,) = driver(f"sumruns {per} {S} {len(main)} {words(main)} {len(heavy)} {words(heavy)}\n")
    runs = [tuple(p) for p in np.asarray(runs, np.int64).reshape(-1, 2)]
    chunks = [tuple(c) for c in np.asarray(chunks, np.int64).reshape(-1, 4)]
    assert (n_main, runs, chunks, most) == restated_sum_runs([main, heavy], per, S)
    assert most == 1024 * S
    for part, mine in ((main, runs[:n_main]), (heavy, runs[n_main:])):
        assert mine[0][0] == 0 and mine[-1][1] == len(part) and all(a[1] == b[0] for a, b in zip(mine, mine[1:]))
        for a, b in mine:
            assert 0 < b - a <= per and len({part[t][0] for t in range(a, b)}) == 1    # never two c0 in a run
    # the chunks partition the runs' slabs; each holds at most 32 slabs, all of one c0 and one part
    assert chunks[0][0] == 0 and chunks[-1][1] == len(runs) and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    for lo, hi, cell0, nvals in chunks:
        assert 0 < hi - lo <= 32 and (hi <= n_main or lo >= n_main)
        part = main if hi <= n_main else heavy
        tiles = [part[t] for a, b in runs[lo:hi] for t in range(a, b)]
        assert {c0 * S for c0, _ in tiles} == {cell0} and {nc * S for _, nc in tiles} == {nvals}
    if per == 1:
        assert max(hi - lo for lo, hi, _, _ in chunks) == 32
