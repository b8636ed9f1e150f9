"""CPU: the DEFLATE streams zlib's compressor never writes (tests/deflate_writer.py) against zlib's inflate -- the reference: it
must accept every valid case and give the expected bytes -- and against the host build of csrc/inflate_lane.h, the decoder
behind the GPU inflate kernel.  Then what the cases claim to exercise, computed from their own code lengths and tokens, not
from their names; and the writer's own parts against brute force.  tests/test_inflate_foreign_gpu.py sends the same cases
through the kernel, whose table construction (coop_tables) no host test runs."""
import itertools
import zlib

import numpy as np
import pytest

import deflate_writer as dw
from test_inflate_lane import lane  # noqa: F401  (the fixture: inflate_lane_host.cpp compiled for the host)


@pytest.fixture(scope="module")
def corpus():
    return dw.corpus()


@pytest.fixture(scope="module")
def blocks():
    return dw.corpus_blocks()


def test_families_and_order(corpus):
    assert tuple(dict.fromkeys(dw.family_of(n) for n in corpus)) == dw.FAMILIES
    assert list(corpus) == list(dw.corpus())                                   # deterministic
    assert sum(len(d) for _, d in corpus.values()) < 4 << 20


def test_valid_cases_against_zlib_and_the_host_lane(corpus, lane):  # noqa: F811
    for name, (raw, data) in corpus.items():
        d = zlib.decompressobj(-15)
        got = d.decompress(raw)
        assert got == data and d.eof and d.unused_data == b"", name
        rc, out = lane(raw, len(data))
        assert rc == 0 and out == data, (name, rc)


def test_invalid_cases_fail_in_zlib_and_in_the_host_lane(lane):  # noqa: F811
    inv = dw.invalid()
    assert set(dw.LANE_ACCEPTS) <= set(inv) and set(dw.TABLE_LEVEL) <= set(inv)
    for name, (raw, n) in inv.items():
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(raw)
            refused = not (d.eof and len(got) == n)
        except zlib.error:
            refused = True
        assert refused, name
        rc, out = lane(raw, n)
        # (the one documented difference: an incomplete set whose missing codes nobody uses decodes)
        assert (rc == 0) == (name in dw.LANE_ACCEPTS), (name, rc)


def _sorted_syms(lens):
    return sorted((s for s, l in enumerate(lens) if l), key=lambda s: (lens[s], s))


def _used(block):
    lf, df = dw.token_freq(block["tokens"])
    return {s for s, f in enumerate(lf) if f}, {s for s, f in enumerate(df) if f}


def _cold(block):
    """sorted position -> symbol for the literal/length symbols the decoder keeps in its cold table: codes longer than the
    8-bit first-level table, from the 129th of them on"""
    ll = block["ll_lens"]
    order = _sorted_syms(ll)
    base = sum(1 for s in order if ll[s] <= 8)
    return {i: s for i, s in enumerate(order) if i - base >= 128}


def test_flat_long_reads_cold_length_symbols_that_differ_between_blocks(blocks):
    for name in ("flat_long/one", "flat_long/twice", "flat_long/six"):
        per_block = []
        for b in blocks[name]:
            used, dused = _used(b)
            assert used == set(range(286)) and dused == set(range(30)), name      # every symbol of both codes
            cold = _cold(b)
            assert len(cold) == 157
            n = sum(1 for i, s in cold.items() if s >= 256 and s in used)
            assert n >= 20, (name, n)
            assert {i >> 5 for i in cold} == {4, 5, 6, 7, 8}                       # every word of the ninth bits that can be cold
            per_block.append(cold)
        for a, b in zip(per_block, per_block[1:]):
            differ = sum(1 for i in a if i in b and a[i] != b[i])
            ninth = sum(1 for i in a if i in b and (a[i] >> 8) != (b[i] >> 8))
            print(name, "cold positions: symbols differ at", differ, "ninth bits at", ninth)
            assert differ >= 20 and ninth >= 20, (name, differ, ninth)
    assert len(blocks["flat_long/twice"]) == 2 and len(blocks["flat_long/six"]) == 6


def _match_bits(b, t):
    ls, le, _ = dw.length_symbol(t[0], t[2] if len(t) > 2 else None)
    ds, de, _ = dw.dist_symbol(t[1])
    return b["ll_lens"][ls] + le + b["d_lens"][ds] + de


def test_deep_has_48_bit_turns_behind_one_to_six_literals(blocks):
    b, = blocks["deep/deep"]
    ll, toks = b["ll_lens"], b["tokens"]
    assert sorted(l for l in ll if l) == list(range(1, 16)) + [15] and ll[284] == ll[285] == 15 and ll[256] and ll[257]
    assert sorted(l for l in b["d_lens"] if l) == list(range(1, 16)) + [15] and b["d_lens"][28] == b["d_lens"][29] == 15
    first = next(k for k, t in enumerate(toks) if not isinstance(t, int))
    assert first >= 32768 and toks[first][:2] == (258, 32768)                     # dist == op: back to the block's first byte
    behind = set()
    for k, t in enumerate(toks):
        if not isinstance(t, int) and _match_bits(b, t) == 48:
            q = 0
            while isinstance(toks[k - 1 - q], int) and ll[toks[k - 1 - q]] <= 8:
                q += 1
            behind.add(q)
    assert behind >= {0, 1, 2, 3, 4, 5, 6}, behind
    for want in ((258, 32768, 284), (257, 32767), (227, 24577), (3, 1), (258, 16385)):
        assert want in toks


def test_dsyms_long_reads_both_word_borders(blocks):
    b, = blocks["dsyms_long/dsyms_long"]
    d = b["d_lens"]
    order = _sorted_syms(d)
    _, dused = _used(b)
    assert len(order) == 30 and dused == set(range(30)) and sum(1 for l in d if l > 6) >= 26
    for pos in (11, 12, 23, 24):
        assert d[order[pos]] > 6 and order[pos] in dused


def _fills(toks):
    op = 0
    for t in toks:
        if isinstance(t, int):
            op += 1
        else:
            yield op % 16, t
            op += t[0]


def test_dist_edges_every_fill_with_every_distance_and_length(blocks):
    seen_d, seen_l = set(), set()
    for name in ("dist_edges/near", "dist_edges/lengths", "dist_edges/far"):
        for b in blocks[name]:
            for fill, t in _fills(b["tokens"]):
                seen_d.add((fill, t[1]))
                seen_l.add((fill,) + (t[0],) + tuple(t[2:]))
    assert seen_d >= set(itertools.product(range(16), dw.DIST_EDGES))
    assert seen_l >= {(f,) + le for f in range(16) for le in dw.LEN_EDGES}
    toks = blocks["dist_edges/near"][0]["tokens"]
    assert toks[5] == (10, 5) and all(isinstance(t, int) for t in toks[:5])      # dist == op
    corpus = dw.corpus()
    for rest in (161, 160, 159, 0):
        toks = blocks["dist_edges/ends_%d_before_end" % rest][0]["tokens"]
        assert toks[300][0] == 258 and len(toks) - 301 == rest
    for rest in (161, 160, 159):
        toks = blocks["dist_edges/starts_%d_before_end" % rest][0]["tokens"]
        assert toks[-1][0] == rest and len(corpus["dist_edges/starts_%d_before_end" % rest][1]) == 558 + rest


def test_few_distance_codes_header_forms_block_mix_many_blocks_and_sizes(corpus, blocks):
    got = {n.split("/")[1]: [l for l in blocks[n][0]["d_lens"] if l] for n in blocks if n.startswith("few_distance_codes/")}
    assert got == {"none": [], "one_at_symbol_0": [1], "one_at_symbol_1": [1], "two_of_length_1": [1, 1]}
    assert blocks["few_distance_codes/one_at_symbol_1"][0]["d_lens"] == [0, 1] and blocks["few_distance_codes/none"][0]["hdist"] == 1
    hf = [b for n in blocks if n.startswith("header_forms/") for b in blocks[n]]
    assert {b["hclen"] for b in hf} >= {5, 8, 19} and {b["hlit"] for b in hf} >= {257, 286} and {b["hdist"] for b in hf} >= {1, 30}
    assert max(max(b["cl_lens"]) for b in hf) == 7
    items = {it for b in hf for it in b["cl_items"] if it[0] >= 16}
    assert items >= {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)}
    b = blocks["header_forms/repeats_hclen_19"][0]
    at, crosses, after18 = 0, False, False
    for k, (s, rep) in enumerate(b["cl_items"]):
        n = rep if s >= 16 else 1
        crosses |= s == 16 and at < b["hlit"] < at + n
        after18 |= s == 16 and b["cl_items"][k - 1][0] == 18
        at += n
    assert crosses and after18
    assert blocks["header_forms/first_symbol_eob"][0]["tokens"] == [] and len(blocks["header_forms/first_symbol_eob"]) == 2
    mix = blocks["block_mix/all_kinds"]
    assert [(b["kind"], b.get("n", len(b.get("tokens", [])) and -1)) for b in mix[:4]] == [("stored", 0), ("fixed", -1), ("stored", 768), ("fixed", 0)]
    assert mix[4]["kind"] == "dynamic" and (mix[-1]["kind"], mix[-1]["tokens"]) == ("fixed", [])
    for kind in ("fixed", "dynamic"):
        assert {b["at"] % 8 for b in mix if b["kind"] == kind} == set(range(8)), kind
    assert blocks["block_mix/stored_65535"][0]["n"] == 65535
    many = blocks["many_blocks/many_blocks"]
    sizes = [sum(1 if isinstance(t, int) else t[0] for t in b["tokens"]) for b in many]
    assert len(many) == 48 and all(b["kind"] == "dynamic" for b in many) and sum(sizes) == 65280
    assert min(sizes) >= 40 and max(sizes) <= 4000 and len(set(sizes)) > 40, sizes
    for k, b in enumerate(many):
        assert max(b["ll_lens"]) <= (15, 11, 9, 8)[k % 4]
    assert len({tuple(b["ll_lens"]) for b in many}) == 48
    assert 8 in {max(b["ll_lens"]) for b in many[3::4]} and 9 in {max(b["ll_lens"]) for b in many[2::4]}
    assert sorted({len(d) for n, (_, d) in corpus.items() if n.startswith("isize_edges/")}) == [0, 1, 15, 16, 17, 159, 160, 161, 65535, 65536]


def test_bam_foreign_is_what_zlib_never_writes(corpus, blocks):
    names = [n for n in blocks if n.startswith("bam_foreign/")]
    far = far3 = most_long = 0
    headers = set()
    for n in names:
        b, = blocks[n]
        for t in b["tokens"]:
            if not isinstance(t, int):
                far += t[1] > 32506
                far3 += t[0] == 3 and t[1] > 4096
        most_long = max(most_long, sum(1 for l in b["ll_lens"] if l > 8))
        headers.add((tuple(b["ll_lens"]), tuple(b["d_lens"])))
    print("bam_foreign: blocks", len(names), "matches beyond 32,506:", far, "3-byte matches beyond 4,096:", far3,
          "most long symbols in a block:", most_long)
    assert far >= 1 and far3 >= 1 and most_long > 128 and len(headers) == len(names)
    stream = b"".join(corpus[n][1] for n in names)
    assert stream == dw.bam_stream() and stream[:4] == b"BAM\x01"
    sizes = {len(corpus[n][1]) for n in names}
    assert {65280, 65536, 65535, 60001, 3} <= sizes
    # the container: empty blocks in the middle, another subfield in front of BC, and gzip reads it all
    import gzip
    f, n_blocks, total = dw.family_file("bam_foreign")
    assert gzip.decompress(f) == stream and total == len(stream) and n_blocks == len(names) + (len(names) - 1) // 8
    assert f.count(b"ZZ\x04\x00bsigBC\x02\x00") == len(names) // 5


def test_lengths_from_freq_against_brute_force():
    rng = np.random.default_rng(8)
    for trial in range(60):
        n = int(rng.integers(2, 9))
        limit = int(rng.integers(max(1, int(np.ceil(np.log2(n)))), 6))
        freq = [int(x) for x in rng.integers(1, 50, n)] if trial % 3 else [int(x) for x in 2 ** rng.integers(0, 12, n)]
        lens = dw.lengths_from_freq(freq, limit)
        cost = sum(f * l for f, l in zip(freq, lens))
        best = min(sum(f * l for f, l in zip(freq, c)) for c in itertools.product(range(1, limit + 1), repeat=n)
                   if sum(2.0 ** -l for l in c) <= 1.0)
        assert cost == best and max(lens) <= limit and dw.kraft(lens) == 1 << 15, (freq, limit, lens)
    assert dw.lengths_from_freq([0, 5, 0], 7) == [0, 1, 0] and dw.lengths_from_freq([0, 0], 7) == [0, 0]


def test_tokenizer_round_trip_and_knobs():
    rng = np.random.default_rng(9)
    stream = dw.bam_stream()
    for k, data in enumerate((stream[5000:45000], bytes(rng.integers(0, 3, 5000).astype(np.uint8)), b"", b"ab", b"x" * 1000,
                              (bytes(rng.integers(0, 256, 33000).astype(np.uint8)) * 2)[:65536])):
        for far3, full in ((True, True), (False, False)):
            toks = dw.tokenize(data, far3=far3, full_window=full)
            assert dw.expand(toks) == data, k
            m = [t for t in toks if not isinstance(t, int)]
            assert all(3 <= t[0] <= 258 and 1 <= t[1] <= (32768 if full else 32506) for t in m)
            if not far3:
                assert not any(t[0] == 3 and t[1] > 4096 for t in m)
    assert dw.expand([1, 2, 3, (7, 2)], b"\x09") == bytes([1, 2, 3, 2, 3, 2, 3, 2, 3, 2])
    assert dw.expand([(4, 1)], b"\x09") == b"\x09" * 4
    # the writer's blocks re-read by zlib: a tokenized stream through each emitter
    data = stream[5000:9000]
    toks = dw.tokenize(data)
    for emit in ("fixed", "auto"):
        w = dw.Deflate()
        getattr(w, emit)(toks, True)
        assert zlib.decompress(w.getvalue(), -15) == data
