"""tests/layout_expected.py checked against itself, without a GPU: a restated layout decodes back into the reads it
was made of, its indexes file every read under the bucket of its coordinate, its classes are the forms deck's own, the
checksum and the CIGAR walk agree with sums done by hand in Python integers, and the file reader reads back what a
writer of the same format wrote and refuses what is not such a file.  The inputs are tests/test_layout_gpu.py's."""
import struct

import numpy as np
import pytest

import forms_deck as deck
import layout_expected as le
import test_layout_gpu as tg


def _inputs():
    d = deck.reads()
    return {
        "mixed": tg.mixed_reads(6145, 7145),
        "many_references": tg.many_references(),
        "edges": tg.edge_reads(tg.EDGE_SPANS),
        "deck": {k: d[k] for k in ("ref_len", "ref_off", "pos", "end", "flag", "mapq", "tlen")},
    }


@pytest.fixture(scope="module")
def layouts():
    return {name: (cols, tg.want_layout(cols)) for name, cols in _inputs().items()}


@pytest.mark.parametrize("name", ["mixed", "many_references", "edges", "deck"])
def test_a_layout_decodes_back_into_its_reads(layouts, name):
    cols, L = layouts[name]
    cls = L["read_class"]
    span = cols["end"].astype(np.int64) - cols["pos"] + 1
    assert sum(C["n"] for C in L["cls"]) == len(cls) == L["n_reads"]
    assert L["n_classes"] == sum(C["n"] > 0 for C in L["cls"]) == 5
    for c in range(le.N_CLASSES):
        m = cls == c                                        # boolean mask: input order
        C = L["cls"][c]
        pos, sp, flag, mapq, tlen = le.decode_class(L, c)
        for what, got, want in (("pos", pos, cols["pos"][m]), ("span", sp, span[m]), ("flag", flag, cols["flag"][m]),
                                ("mapq", mapq, cols["mapq"][m]), ("tlen", tlen, cols["tlen"][m])):
            assert np.array_equal(got, want.astype(np.int64)), (c, what)
        assert C["maxspan"] == span[m].max() and C["col_cap"] == (C["n"] + 3) // 4 * 4 + 4 and 4 <= C["col_cap"] - C["n"] <= 7
        for col in le.COLUMNS:
            assert (C[col] is not None) == le.class_has(c, col)
            if C[col] is not None:
                assert len(C[col]) == C["col_cap"] and not C[col][C["n"]:].any()


@pytest.mark.parametrize("name", ["mixed", "many_references", "edges", "deck"])
def test_every_index_files_every_read_under_its_bucket(layouts, name):
    cols, L = layouts[name]
    n = len(cols["pos"])
    rid = np.searchsorted(cols["ref_off"][1:], np.arange(n), side="right")
    unit0, units = L["ref_unit0"].astype(np.int64), L["ref_units"].astype(np.int64)
    assert np.array_equal(units, (cols["ref_len"].astype(np.int64) >> 16) + 1)
    assert np.array_equal(unit0, np.cumsum(units) - units)
    total_bp = int(units.sum()) << 16
    g = (unit0[rid] << 16) + np.clip(cols["pos"].astype(np.int64), 0, (units[rid] << 16) - 1)
    for c in range(le.N_CLASSES):
        C = L["cls"][c]
        idx = C["idx"].astype(np.int64)
        assert C["idx_entries"] == (total_bp >> C["kshift"]) + 2 and len(idx) == C["idx_entries"] - 1
        assert idx[0] == 0 and np.all(np.diff(idx) >= 0) and idx[-1] == C["n"]
        assert 4 <= C["kshift"] <= (15 if c == le.PACKED else 16)
        assert np.array_equal(le.read_buckets(L, c), g[L["read_class"] == c] >> C["kshift"])


def test_the_classes_are_the_forms_decks_own(layouts):
    cols, L = layouts["deck"]
    assert np.array_equal(L["read_class"], deck.read_classes(True))
    unpacked = tg.want_layout(cols, pack=False)
    assert np.array_equal(unpacked["read_class"], deck.read_classes(False))
    assert unpacked["n_codes"] == 0 and unpacked["fmtab"] is None and unpacked["cls"][4]["n"] == 0 and unpacked["n_classes"] == 4
    assert L["n_codes"] == 512                   # the deck has more pairs than codes: some short reads stay in class 0
    short = (cols["end"].astype(np.int64) - cols["pos"] + 1 <= 256) & (cols["flag"] < 4096)
    assert np.any(L["read_class"][short] == 0)


def test_the_pair_table_orders_by_count_then_key():
    pos = np.arange(10) * 10
    flag = np.asarray([16, 0, 16, 99, 0, 4095, 99, 5000, 0, 7])
    mapq = np.asarray([3, 3, 3, 0, 3, 255, 0, 1, 2, 9])
    end = pos + np.asarray([0, 255, 9, 9, 9, 9, 9, 9, 9, 256])            # the last read is 257 long: not counted
    keys, counts = le.pair_table(pos, end, flag, mapq)
    k = lambda f, q: f | q << 12
    assert keys.tolist() == [k(99, 0), k(0, 3), k(16, 3), k(0, 2), k(4095, 255)] and counts.tolist() == [2, 2, 2, 1, 1]
    assert le.sample_stride(2047 * 2048) == 1 and le.sample_stride(2047 * 2048 + 1) == 2 and le.sample_stride(3072 * 2048) == 3


def test_bucket_shift_follows_the_loop():
    # 16 reads a bucket: the largest power of two <= 16 * total_bp / n, between 16 bp and 64 kbp (32 kbp packed)
    assert le.bucket_shift(1 << 16, 1 << 20, False) == 8 and le.bucket_shift((1 << 16) + 1, 1 << 20, False) == 7
    assert le.bucket_shift(1 << 30, 1 << 20, False) == 4 and le.bucket_shift(1, 1 << 20, False) == 16
    assert le.bucket_shift(1, 1 << 20, True) == 15 and le.bucket_shift(100, 1 << 20, True, 1e12) == 15
    assert le.bucket_shift(1 << 16, 1 << 20, False, 1.0) == 4 and le.bucket_shift(1 << 16, 1 << 20, False, 0.001) == 4
    assert le.bucket_shift(3, 3 << 16, False, 1.0) == 16 and le.bucket_shift(3, (3 << 16) - (1 << 16), False, 1.0) == 15


def test_cigar_end_by_hand():
    op = dict(M=0, I=1, D=2, N=3, S=4, H=5, P=6, EQ=7, X=8)
    reads = [
        (100, 0, [(10, "M")], 109),
        (100, 0, [(3, "S"), (10, "M"), (2, "I"), (5, "D"), (100, "N"), (4, "EQ"), (1, "X"), (2, "P"), (9, "H")], 100 + 120 - 1),
        (100, 4, [(10, "M")], 100),                                    # unmapped: one base
        (100, 0, [], 100),                                             # no CIGAR: one base
        (100, 0, [(5, "S"), (7, "I"), (2, "H"), (1, "P")], 100),       # nothing on the reference: one base
        (-5, 0, [(10, "M")], 4),
        (100, 0, [(10, "M"), (50, 9), (50, 15), (1, "M")], 110),       # op codes 9 .. 15 consume nothing
        (0, 0, [((1 << 28) - 1, "N")], (1 << 28) - 2),
    ]
    off, cg = [0], []
    for _, _, ops, _ in reads:
        cg += [ln << 4 | (op[o] if isinstance(o, str) else o) for ln, o in ops]
        off.append(len(cg))
    got = le.cigar_end([r[0] for r in reads], [r[1] for r in reads], off, np.asarray(cg, np.uint32))
    assert got.tolist() == [r[3] for r in reads]


def test_cigars_for_keeps_the_spans():
    cols = tg.mixed_reads(2049, 3049)
    flag, off, cg, shape = tg.cigars_for(cols, 4049)
    end = le.cigar_end(cols["pos"], flag, off, cg)
    one = np.isin(shape, (3, 4, 5))
    assert np.array_equal(end[~one], cols["end"][~one]) and np.array_equal(end[one], cols["pos"][one])
    assert set(shape.tolist()) == set(range(8)) and set((cg & 15).tolist()) == set(range(16))


def _mix_by_hand(word, i, salt):
    M, mask = 0xD6E8FEB86659FD93, (1 << 64) - 1
    x = ((word << 32) | ((i * 0x9E3779B1) & 0xFFFFFFFF)) ^ (((i + salt) * M) & mask)
    x ^= x >> 32
    x = (x * M) & mask
    return x ^ (x >> 29)


def test_checksum_by_hand(layouts):
    words = np.asarray([0, 1, 0xFFFFFFFF, 0x80000000, 12345], np.uint32)
    for salt in (1, 0x100000002, 25 * 0x100000001 + 1):
        want = sum(_mix_by_hand(int(w), i, salt) for i, w in enumerate(words)) & ((1 << 64) - 1)
        assert le.words_checksum(words, salt) == want
    assert le.words_checksum(np.asarray([-1, -2], np.int32), 1) == le.words_checksum(np.asarray([0xFFFFFFFF, 0xFFFFFFFE], np.uint32), 1)
    assert le.words_checksum(np.zeros(0, np.uint32), 1) == 0
    # the salts: + 0x100000001 per column slot of a non-empty class, with or without the column, and per index; none for
    # an empty class; the pair table last
    step, mask = 0x100000001, (1 << 64) - 1
    alone = tg.want_layout(tg.edge_reads((4097, 5000), with_high_flags=False))
    assert [c for c in range(5) if alone["cls"][c]["n"]] == [2]
    C = alone["cls"][2]
    want = sum(le.words_checksum(C[col], 1 + j * step) for j, col in enumerate(("pos", "end", "fm", "tlen", "idx")))
    assert le.expected_checksum(alone) == want & mask
    packed = tg.want_layout(tg.edge_reads((1, 256), with_high_flags=False))
    assert [c for c in range(5) if packed["cls"][c]["n"]] == [4]
    C = packed["cls"][4]
    want = le.words_checksum(C["fm"], 1 + 2 * step) + le.words_checksum(C["tlen"], 1 + 3 * step) + le.words_checksum(C["idx"], 1 + 4 * step) \
        + le.words_checksum(packed["fmtab"], 1 + 5 * step)
    assert le.expected_checksum(packed) == want & mask
    _, L = layouts["mixed"]
    total, slot = 0, 0
    for c in range(5):
        for col in ("pos", "end", "fm", "tlen", "idx"):
            if L["cls"][c][col] is not None:
                total += le.words_checksum(L["cls"][c][col], 1 + slot * step)
            slot += 1
    assert le.expected_checksum(L) == (total + le.words_checksum(L["fmtab"], 1 + 25 * step)) & mask


def test_read_layout_round_trip(layouts, tmp_path):
    assert le.HEADER_BYTES == 216
    for name in ("mixed", "edges"):
        _, L = layouts[name]
        path = str(tmp_path / (name + ".bsig"))
        le.write_layout(path, L, stamp="a stamp of 24 characters", checksum=le.expected_checksum(L), spare=0xDEADBEEF)
        back = le.read_layout(path)
        assert back["stamp"] == "a stamp of 24 characters" and back["checksum"] == le.expected_checksum(L)
        assert le.layout_differences(back, L) == []
        raw = open(path, "rb").read()
        # every piece padded to 64 bytes: header, stamp, three reference arrays, the pair table, then the classes
        size = 256 + 64 + 3 * le.pad64(4 * L["n_ref"]) + 2048
        for c, C in enumerate(L["cls"]):
            size += (4 if c in (2, 3) else 2 if c == 4 else 3) * le.pad64(4 * C["col_cap"]) + le.pad64(4 * C["idx_entries"])
        assert len(raw) == size and struct.unpack_from("<Q", raw, 32)[0] == size
        # the spare last entry of an index is in the file and not in what the reader returns
        assert raw.count(struct.pack("<I", 0xDEADBEEF)) >= 5 and all(0xDEADBEEF not in C["idx"][-1:] for C in back["cls"])
    # one changed word is named, not printed
    other = le.read_layout(path)
    other["cls"][1]["fm"][3] ^= 1
    other["cls"][4]["idx"][7:9] += 1
    diff = le.layout_differences(other, L)
    assert len(diff) == 2 and diff[0].startswith("class 1 fm: 1 of") and "first at 3" in diff[0]
    assert diff[1].startswith("class 4 idx: 2 of") and "first at 7" in diff[1]
    other["checksum"] ^= 1 << 63                 # the header's checksum is held to the restatement's
    assert le.layout_differences(other, L)[2].startswith("checksum")
    assert all(len(line) < 200 for line in diff)


def test_read_layout_refuses_what_is_no_reads_file(layouts, tmp_path):
    _, L = layouts["edges"]
    path = str(tmp_path / "ok.bsig")
    le.write_layout(path, L)
    raw = open(path, "rb").read()
    for name, data, message in (("truncated", raw[:-64], "header says"), ("longer", raw + bytes(64), "header says"),
                                ("magic", b"BSIGRDS2" + raw[8:], "magic"), ("version", raw[:8] + struct.pack("<I", 3) + raw[12:], "version"),
                                ("stub", raw[:100], "shorter")):
        p = str(tmp_path / (name + ".bsig"))
        open(p, "wb").write(data)
        with pytest.raises(AssertionError, match=message):
            le.read_layout(p)
