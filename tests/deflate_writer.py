"""A DEFLATE (RFC 1951) and BGZF writer for tests: the streams zlib's compressor never produces.

Every DEFLATE stream the inflate kernel met before came out of zlib (or, once, htslib).  RFC 1951 allows far more: matches
at the full 32,768 bytes, 3-byte matches at any distance, one distance code or none, 15-bit codes, code-length headers run-length
coded in any legal way, dozens of tiny blocks.  This module writes such streams bit by bit, from the RFC alone:

  * BitWriter: bits LSB first, Huffman codes MSB first;
  * Deflate: stored / fixed / dynamic block emitters that take the code lengths, the tokens and (optionally) the exact
    code-length item stream, and choose HLIT / HDIST / HCLEN themselves unless told otherwise;
  * lengths_from_freq: an optimal length-limited Huffman code (package-merge), complete whenever two symbols are used;
  * tokenize: a greedy LZ77 tokenizer over the whole 32,768-byte window with 3-byte matches at any distance;
  * bgzf_block: the BGZF container, with other gzip subfields in front of BC if asked;
  * corpus() / invalid(): the seeded, deterministic cases of tests/test_deflate_writer_cpu.py, tests/test_inflate_foreign_gpu.py
    and the sanitizer driver's test.

A token is a literal byte (int) or a match (length, distance) -- or (length, distance, length symbol) where the length symbol is
to be chosen (258 as symbol 284 + extra 31).  The invalid cases also use ("ll", symbol), ("d", symbol) and ("raw", value, bits).
"""
import bisect
import functools
import gzip
import os
import struct
import tempfile
import zlib
from collections import OrderedDict

import numpy as np

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)       # RFC 1951, 3.2.7
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _len_table():
    base, extra = [], []
    for s in range(28):                              # symbols 257..284: 3..10 one each, then four symbols per extra bit
        e = 0 if s < 8 else (s >> 2) - 1
        base.append(3 + s if s < 8 else 3 + ((4 + (s & 3)) << e))
        extra.append(e)
    return base + [258], extra + [0]                 # symbol 285: 258, no extra bits


def _dist_table():
    base, extra = [], []
    for s in range(30):                              # 1..4 one each, then two symbols per extra bit
        e = 0 if s < 4 else (s >> 1) - 1
        base.append(1 + s if s < 4 else 1 + ((2 + (s & 1)) << e))
        extra.append(e)
    return base, extra


LEN_BASE, LEN_EXTRA = _len_table()
DIST_BASE, DIST_EXTRA = _dist_table()
assert LEN_BASE[27] == 227 and LEN_EXTRA[27] == 5 and DIST_BASE[29] == 24577 and DIST_EXTRA[29] == 13


def length_symbol(length, lsym=None):
    """(symbol 257..285, extra bits, extra value) of a match length; lsym picks the symbol (258 as 284 + 31)"""
    assert 3 <= length <= 258
    if lsym is None:
        lsym = 285 if length == 258 else 257 + bisect.bisect_right(LEN_BASE, length, 0, 28) - 1
    s = lsym - 257
    v = length - LEN_BASE[s]
    assert 0 <= v < (1 << LEN_EXTRA[s]) or (v == 0 and LEN_EXTRA[s] == 0), (length, lsym)
    return lsym, LEN_EXTRA[s], v


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    s = bisect.bisect_right(DIST_BASE, dist) - 1
    return s, DIST_EXTRA[s], dist - DIST_BASE[s]


def _rev(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def canonical_codes(lengths):
    """the canonical Huffman codes (RFC 1951, 3.2.2) of a list of lengths, as the bit-reversed values a LSB-first writer emits"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l:
            out.append(_rev(nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append(0)
    return out


def kraft(lengths):
    """sum of 2^-l over the used symbols, in units of 2^-15"""
    return sum(1 << (15 - l) for l in lengths if l)


def lengths_from_freq(freq, limit):
    """An optimal Huffman code with no length above `limit` (package-merge).  One used symbol gets length 1; with two or more
    the code is complete, which is asserted here."""
    used = [s for s, f in enumerate(freq) if f > 0]
    lens = [0] * len(freq)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    assert len(used) <= (1 << limit), (len(used), limit)
    leaves = sorted(((freq[s], (s,)) for s in used), key=lambda t: t[0])
    cur = leaves
    for _ in range(limit - 1):
        packs = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packs, key=lambda t: t[0])
    for _, syms in cur[:2 * len(used) - 2]:
        for s in syms:
            lens[s] += 1
    assert kraft(lens) == 1 << 15 and max(lens) <= limit, (kraft(lens), max(lens))
    return lens


def rle_items(seq):
    """a run-length coding of the code lengths as (symbol, repeat) items: the longest legal repeats"""
    items, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                items.append((18, r))
                run -= r
            if run >= 3:
                items.append((17, run))
                run = 0
        else:
            items.append((v, 1))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                items.append((16, r))
                run -= r
        items += [(v, 1)] * run
        i = j
    return items


def expand_items(items):
    out = []
    for s, rep in items:
        if s < 16:
            out.append(s)
        elif s == 16:
            assert out and 3 <= rep <= 6
            out += [out[-1]] * rep
        elif s == 17:
            assert 3 <= rep <= 10
            out += [0] * rep
        else:
            assert 11 <= rep <= 138
            out += [0] * rep
    return out


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):                            # n bits of v, least significant first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 4096:
            self._spill()

    def _spill(self):
        k = self.n >> 3
        self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    def code(self, c, n):                            # a Huffman code, most significant bit first
        self.bits(_rev(c, n), n)

    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def align(self):
        self.bits(0, -self.bitpos() % 8)

    def raw(self, data):
        self.align()
        self._spill()
        self.buf += data

    def getvalue(self):
        k = (self.n + 7) >> 3
        return bytes(self.buf) + self.acc.to_bytes(k, "little")


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class Deflate(BitWriter):
    """block emitters; .blocks logs what was written (kind, code lengths, tokens, header fields, first bit) for the
    tests' non-vacuity figures"""

    def __init__(self):
        super().__init__()
        self.blocks = []

    def stored(self, data, last, nlen=None):
        at = self.bitpos()
        self.bits(int(last), 1)
        self.bits(0, 2)
        self.align()
        assert len(data) <= 65535
        self.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + bytes(data))
        self.blocks.append(dict(kind="stored", at=at, n=len(data)))

    def _emit(self, tokens, ll_lens, d_lens, eob=True):
        llc, dc = canonical_codes(ll_lens), canonical_codes(d_lens)
        bits = self.bits
        for t in tokens:
            if isinstance(t, int):
                assert ll_lens[t], ("literal without a code", t)
                bits(llc[t], ll_lens[t])
            elif isinstance(t[0], str):
                if t[0] == "ll":
                    bits(llc[t[1]], ll_lens[t[1]])
                elif t[0] == "d":
                    bits(dc[t[1]], d_lens[t[1]])
                else:
                    bits(t[1], t[2])
            else:
                ls, le, lv = length_symbol(t[0], t[2] if len(t) > 2 else None)
                ds, de, dv = dist_symbol(t[1])
                assert ll_lens[ls] and d_lens[ds], ("match without a code", t)
                bits(llc[ls], ll_lens[ls])
                bits(lv, le)
                bits(dc[ds], d_lens[ds])
                bits(dv, de)
        if eob:
            bits(llc[256], ll_lens[256])

    def fixed(self, tokens, last):
        at = self.bitpos()
        self.bits(int(last), 1)
        self.bits(1, 2)
        self._emit(tokens, FIXED_LL, FIXED_D)
        self.blocks.append(dict(kind="fixed", at=at, ll_lens=FIXED_LL, d_lens=FIXED_D, tokens=list(tokens)))

    def dynamic(self, ll_lens, d_lens, tokens, last, cl_items=None, hlit=None, hdist=None, hclen=None, cl_lens=None,
                check=True, eob=True):
        """hlit / hdist / hclen: the COUNTS (257..286, 1..30, 4..19) to write instead of the smallest that hold the lengths;
        cl_lens: the code-length code's 19 lengths instead of lengths_from_freq(items, 7); check=False: write it even if
        it is not a valid stream"""
        at = self.bitpos()
        ll, d = list(ll_lens), list(d_lens)
        if hlit is None:
            hlit = max([257] + [k + 1 for k, l in enumerate(ll) if l])
        if hdist is None:
            hdist = max([1] + [k + 1 for k, l in enumerate(d) if l])
        ll = (ll + [0] * hlit)[:hlit]
        d = (d + [0] * hdist)[:hdist]
        seq = ll + d
        if cl_items is None:
            cl_items = rle_items(seq)
        if check:
            assert 257 <= hlit <= 286 and 1 <= hdist <= 30
            assert expand_items(cl_items) == seq, "the code-length items do not spell the code lengths"
        if cl_lens is None:
            freq = [0] * 19
            for s, _ in cl_items:
                freq[s] += 1
            cl_lens = lengths_from_freq(freq, 7)
            if sum(1 for l in cl_lens if l) == 1:          # zlib wants this code complete: a second 1-bit code nobody uses
                cl_lens[[s for s in (0, 8, 16) if not cl_lens[s]][0]] = 1
        need = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
        if hclen is None:
            hclen = need
        assert not check or hclen >= need
        self.bits(int(last), 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for k in range(hclen):
            self.bits(cl_lens[CL_ORDER[k]], 3)
        clc = canonical_codes(cl_lens)
        for s, rep in cl_items:
            assert cl_lens[s] or not check
            self.bits(clc[s], cl_lens[s])
            if s == 16:
                self.bits(rep - 3, 2)
            elif s == 17:
                self.bits(rep - 3, 3)
            elif s == 18:
                self.bits(rep - 11, 7)
        self._emit(tokens, ll + [0] * (288 - len(ll)), d + [0] * (32 - len(d)), eob)
        self.blocks.append(dict(kind="dynamic", at=at, ll_lens=ll, d_lens=d, tokens=list(tokens), hlit=hlit, hdist=hdist,
                                hclen=hclen, cl_lens=list(cl_lens), cl_items=list(cl_items)))

    def auto(self, tokens, last, limit=15, **kw):
        """a dynamic block whose codes are lengths_from_freq of the tokens' own symbols"""
        lf, df = token_freq(tokens)
        self.dynamic(lengths_from_freq(lf, limit), lengths_from_freq(df, min(limit, 15)), tokens, last, **kw)


def token_freq(tokens):
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[length_symbol(t[0], t[2] if len(t) > 2 else None)[0]] += 1
            df[dist_symbol(t[1])[0]] += 1
    return lf, df


def expand(tokens, history=b""):
    """the bytes the tokens mean, behind `history`"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            l, dist = t[0], t[1]
            start = len(out) - dist
            assert start >= 0, "a match reaches in front of the output"
            if dist >= l:
                out += out[start:start + l]
            else:
                out += (bytes(out[start:]) * (l // dist + 1))[:l]
    return bytes(out[len(history):])


def tokenize(data, far3=True, full_window=True, chain=4):
    """Greedy LZ77: the longest match among the latest `chain` positions with the same three bytes, the FARTHEST of equals.
    far3: 3-byte matches at any distance (zlib: within 4,096); full_window: distances up to 32,768 (zlib: 32,506)."""
    n, toks, table, i = len(data), [], {}, 0
    maxd = 32768 if full_window else 32506

    def insert(a, b):
        for j in range(a, min(b, n - 2)):
            lst = table.setdefault(data[j:j + 3], [])
            lst.append(j)
            if len(lst) > chain:
                del lst[0]

    while i < n:
        best_l = best_d = 0
        cands = table.get(data[i:i + 3]) if i + 3 <= n else None
        if cands:
            maxl = min(258, n - i)
            for p in reversed(cands):
                dist = i - p
                if dist > maxd:
                    break
                if data[p:p + maxl] == data[i:i + maxl]:
                    l = maxl
                else:
                    lo, hi = 3, maxl                      # the first lo bytes match, the first hi do not
                    while hi - lo > 1:
                        mid = (lo + hi) >> 1
                        if data[p + lo:p + mid] == data[i + lo:i + mid]:
                            lo = mid
                        else:
                            hi = mid
                    l = lo
                if l == 3 and dist > 4096 and not far3:
                    continue
                if l >= best_l:
                    best_l, best_d = l, dist
        if best_l >= 3:
            toks.append((best_l, best_d))
            insert(i, i + best_l)
            i += best_l
        else:
            toks.append(data[i])
            insert(i, i + 1)
            i += 1
    return toks


def bgzf_block(raw_deflate, data, extra=b"", crc=None, isize=None):
    """one BGZF block: gzip header with the BC subfield (other subfields, `extra`, in front of it), the DEFLATE data, CRC32, ISIZE"""
    xlen = len(extra) + 6
    total = 12 + xlen + len(raw_deflate) + 8
    assert total <= 65536 and len(data) <= 65536, (total, len(data))
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\x00" + struct.pack("<H", total - 1)
            + raw_deflate + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize))


def fits_bgzf(raw_deflate, data, extra=b""):
    return 12 + len(extra) + 6 + len(raw_deflate) + 8 <= 65536 and len(data) <= 65536


# ---- the corpus --------------------------------------------------------------------------------------------------------

def cover_tokens(rng, ll_lens, d_lens, op, rounds=2, lits=True):
    """tokens that use every literal, every length symbol and every distance symbol the codes hold (a distance symbol only
    once `op`, the bytes out so far, reaches it): the literals in random order, then matches that pair the length symbols
    with the distance symbols"""
    toks = []
    if lits:
        ls = [s for s in range(256) if ll_lens[s]]
        toks += [int(x) for x in rng.permutation(ls)]
        op += len(ls)
    lsyms = [s for s in range(257, min(286, len(ll_lens))) if ll_lens[s]]
    dsyms = [s for s in range(min(30, len(d_lens))) if d_lens[s]]
    if not lsyms or not dsyms:
        return toks
    for k in range(rounds * max(len(lsyms), len(dsyms))):
        lsym, ds = lsyms[k % len(lsyms)], dsyms[(k + k // len(dsyms)) % len(dsyms)]
        if DIST_BASE[ds] > op:
            continue
        length = LEN_BASE[lsym - 257] + (int(rng.integers(0, 1 << LEN_EXTRA[lsym - 257])) if lsym != 285 else 0)
        dist = min(op, DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds])))
        toks.append((length, dist, lsym))
        op += length
    return toks


def _flat_ll(ten_bit_from):
    """'A' in one bit, the other 285 symbols in 9 (227) and 10 (58) bits; the 10-bit ones are the 58 symbols from
    position `ten_bit_from` of the 285 on"""
    others = [s for s in range(286) if s != 65]
    ll = [9] * 286
    ll[65] = 1
    for k in range(58):
        ll[others[(ten_bit_from + k) % 285]] = 10
    assert kraft(ll) == 1 << 15
    return ll


FLAT_D = [4, 4] + [5] * 28


def _flat_long(rng, n_blocks):
    w = Deflate()
    op = 0
    for b in range(n_blocks):
        ll = _flat_ll(227 if b % 2 == 0 else (b // 2) * 31)       # even blocks: the top 58 symbols; odd: low ones
        toks = []
        if b == 0:                                                 # history for the far distance symbols: half of it 'A's
            body = rng.integers(0, 256, 25000)
            body[rng.random(25000) < 0.5] = 65
            toks += [int(x) for x in body]
        toks += cover_tokens(rng, ll, FLAT_D, op + len(toks))
        w.dynamic(ll, FLAT_D, toks, b == n_blocks - 1)
        op = sum(1 if isinstance(t, int) else t[0] for blk in w.blocks for t in blk["tokens"])
    return w


def _deep(rng):
    lits = [0, 32, 48, 65, 67, 71, 84, 97, 101, 110, 116, 255]       # lengths 1..12
    ll = [0] * 286
    for k, s in enumerate(lits):
        ll[s] = k + 1
    ll[256], ll[257], ll[284], ll[285] = 13, 14, 15, 15
    d = [0] * 30
    for s in range(14):
        d[s] = s + 1
    d[28] = d[29] = 15
    assert kraft(ll) == 1 << 15 and kraft(d) == 1 << 15
    p = np.array([2.0 ** -l for l in range(1, 13)])
    body = [lits[k] for k in rng.choice(12, 32768, p=p / p.sum())]
    body[100:112] = lits                                              # every literal at least once
    toks = body + [(258, 32768, 284), (257, 32767), (227, 24577), (3, 1), (258, 16385), (258, 32768)]
    short = lits[:8]                                                  # codes the 8-bit table holds
    for q in range(0, 7):
        toks += [lits[9], lits[10]]                                   # a long literal ends the token before
        toks += [short[(q + k) % 8] for k in range(q)] + [(258, 32768, 284)]
        toks += [lits[11]] + [short[(2 * q + k) % 8] for k in range(q)] + [(257, 32767)]
    for ds in range(14):                                              # the short distance codes too
        toks += [(3, DIST_BASE[ds])]
    w = Deflate()
    w.dynamic(ll, d, toks, True)
    return w


DIST_EDGES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 32768)
LEN_EDGES = ((3,), (4,), (8,), (9,), (15,), (16,), (17,), (63,), (64,), (65,), (257,), (258,), (258, 284))


def _fill_to(rng, toks, op, fill):
    k = (fill - op) % 16
    toks += [int(x) for x in rng.integers(0, 256, k)]
    return op + k


def _dist_edges(rng):
    """near: every distance of DIST_EDGES below 32,768 at every accumulator fill 0..15 (output offset mod 16), the lengths
    cycling; lengths: every length of LEN_EDGES at every fill, the near distances cycling; far: 32,768 at every fill,
    and dist == op"""
    out = OrderedDict()
    toks = [int(x) for x in rng.integers(0, 256, 5)] + [(10, 5)]     # dist == op
    op, k = 15, 0
    body = [int(x) for x in rng.integers(0, 256, 130)]
    toks += body
    op += len(body)
    for dist in DIST_EDGES[:-1]:
        for fill in range(16):
            op = _fill_to(rng, toks, op, fill)
            le = LEN_EDGES[k % len(LEN_EDGES)]
            k += 1
            if le[0] > 65 and k % 3:
                le = LEN_EDGES[k % 10]                                # (not every one 258 bytes: the block must fit)
            toks.append((le[0], dist) + le[1:])
            op += le[0]
    out["dist_edges/near"] = toks
    toks = [int(x) for x in rng.integers(0, 256, 200)]
    op, k = 200, 0
    for le in LEN_EDGES:
        for fill in range(16):
            op = _fill_to(rng, toks, op, fill)
            toks.append((le[0], DIST_EDGES[k % 19]) + le[1:])
            k += 1
            op += le[0]
    out["dist_edges/lengths"] = toks
    toks = [int(x) for x in rng.integers(0, 256, 32768)] + [(258, 32768)]          # dist == op, to the block's first byte
    op = 32768 + 258
    for fill in range(16):
        op = _fill_to(rng, toks, op, fill)
        le = LEN_EDGES[(3 * fill) % len(LEN_EDGES)]
        toks.append((le[0], 32768) + le[1:])
        op += le[0]
    out["dist_edges/far"] = toks
    # the copier writes the last 160 bytes of a block one by one: 258-byte matches that END 161 / 160 / 159 bytes before
    # the end of the output and exactly at it, and matches that START 161 / 160 / 159 bytes before it and run to it
    for rest in (161, 160, 159, 0):
        out["dist_edges/ends_%d_before_end" % rest] = ([int(x) for x in rng.integers(0, 256, 300)] + [(258, 300)]
                                                       + [int(x) for x in rng.integers(0, 256, rest)])
    for rest in (161, 160, 159):
        out["dist_edges/starts_%d_before_end" % rest] = [int(x) for x in rng.integers(0, 256, 300)] + [(258, 37), (rest, 290)]
    return out


DSYMS_LONG = [1, 2, 3, 4] + [7] * 4 + [8] * 6 + [9] * 2 + [10] * 2 + [11] * 2 + [12] * 2 + [13] * 2 + [14] * 2 + [15] * 4


def _dsyms_long(rng):
    assert len(DSYMS_LONG) == 30 and kraft(DSYMS_LONG) == 1 << 15
    d = [DSYMS_LONG[k] for k in rng.permutation(30)]
    toks = [int(x) for x in rng.integers(0, 64, 32768)]
    for _ in range(3):
        for ds in rng.permutation(30):
            toks.append((int(rng.integers(3, 12)), DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds]))))
    lf, _ = token_freq(toks)
    w = Deflate()
    w.dynamic(lengths_from_freq(lf, 15), d, toks, True)
    return w


def _few_distance_codes(rng):
    out = OrderedDict()
    text = [int(x) for x in rng.integers(97, 123, 400)]
    lf, _ = token_freq(text)
    w = Deflate()
    w.dynamic(lengths_from_freq(lf, 15), [0], text, True)
    out["few_distance_codes/none"] = w
    for name, d, dists in (("one_at_symbol_0", [1], (1,)), ("one_at_symbol_1", [0, 1], (2,)), ("two_of_length_1", [1, 0, 0, 1], (1, 4))):
        toks = list(text[:50])
        for k in range(40):
            toks += text[50 + 3 * k:53 + 3 * k] + [(3 + (7 * k) % 256, dists[k % len(dists)])]
        lf, _ = token_freq(toks)
        w = Deflate()
        w.dynamic(lengths_from_freq(lf, 15), d, toks, True)
        out["few_distance_codes/" + name] = w
    return out


def _header_forms(rng):
    out = OrderedDict()
    # every repeat item at its extremes, a 16 behind an 18, a 16 across HLIT; HLIT 286, HDIST 30, HCLEN 19, 7-bit items
    ll = [0] * 3 + [6] * 7 + [0] * 10 + [7] * 4 + [0] * 11 + [7, 7, 7, 7, 6, 7] + [0] * 138 + [0] * 3 + [0] + [7] * 103
    d = [7, 7, 6] + [5] * 23 + [4] * 4
    items = ([(17, 3), (6, 1), (16, 6), (17, 10), (7, 1), (16, 3), (18, 11), (7, 1), (16, 3), (6, 1), (7, 1), (18, 138), (16, 3), (0, 1),
              (7, 1)] + [(16, 6)] * 16 + [(16, 5), (16, 3), (6, 1), (5, 1), (16, 6), (16, 6), (16, 6), (16, 4), (4, 1), (16, 3)])
    cl = [0] * 19
    for s, l in ((7, 1), (16, 2), (17, 3), (18, 4), (5, 5), (6, 6), (0, 7), (4, 7)):
        cl[s] = l
    assert len(ll) == 286 and kraft(ll) == 1 << 15 and kraft(d) == 1 << 15 and kraft(cl) == 1 << 15
    w = Deflate()
    w.dynamic(ll, d, cover_tokens(rng, ll, d, 0, rounds=6), True, cl_items=items, cl_lens=cl, hlit=286, hdist=30, hclen=19)
    out["header_forms/repeats_hclen_19"] = w
    # five code-length codes (16 17 18 0 8: with four no symbol could have a length): HLIT 257, HDIST 1
    ll = [0] + [8] * 256
    items = [(0, 1), (8, 1)] + [(16, 6)] * 42 + [(16, 3), (0, 1)]
    w = Deflate()
    w.dynamic(ll, [0], [int(x) for x in rng.integers(1, 256, 300)], True, cl_items=items)
    assert w.blocks[0]["hclen"] == 5 and w.blocks[0]["hlit"] == 257 and w.blocks[0]["hdist"] == 1
    out["header_forms/hclen_5"] = w
    # the HCLEN FIELD 4: eight codes (16 17 18 0 8 7 9 6)
    ll = [8] * 255 + [9, 9]
    w = Deflate()
    w.dynamic(ll, [0], [int(x) for x in rng.integers(0, 256, 300)], True, hclen=8)
    out["header_forms/hclen_8"] = w
    # the smallest repeats, chosen where longer ones were possible
    ll = [8] * 255 + [9, 9]
    items = []
    for k in range(0, 252, 4):
        items += [(8, 1), (16, 3)]
    items += [(8, 1)] * 3 + [(9, 1), (9, 1), (17, 3), (0, 1), (0, 1)] + [(18, 11), (17, 3), (17, 9), (0, 1)]
    w = Deflate()
    w.dynamic(ll, [0] * 24, [int(x) for x in rng.integers(0, 256, 300)], True, cl_items=items, hlit=262, hdist=24)
    out["header_forms/smallest_repeats"] = w
    # a dynamic block whose first symbol is end-of-block, then one that holds something
    w = Deflate()
    toks = tokenize(bytes(rng.integers(0, 4, 500).astype(np.uint8)))
    lf, df = token_freq(toks)
    w.dynamic(lengths_from_freq(lf, 15), lengths_from_freq(df, 15), [], False)
    w.auto(toks, True)
    out["header_forms/first_symbol_eob"] = w
    return out


def _block_mix(rng, records):
    out = OrderedDict()
    w = Deflate()
    hist = bytearray()

    def toks_of(data):
        t = tokenize(bytes(hist) + data)                              # (matches may reach into the blocks before)
        got, k = 0, 0
        while got < len(hist):
            got += 1 if isinstance(t[k], int) else t[k][0]
            k += 1
        if got != len(hist):                                          # a match across the border: this part as literals
            return list(data)
        return t[k:]

    def add(kind, data, last=False):
        if kind == "stored":
            w.stored(data, last)
        elif kind == "fixed":
            w.fixed(toks_of(data), last)
        else:
            w.auto(toks_of(data), last, limit=int(rng.choice([15, 9])))
        hist.extend(data)

    at = 0
    def take(n):
        nonlocal at
        at += n
        return records[at - n:at]
    add("stored", b"")
    add("fixed", take(700))
    add("stored", take(768))
    add("fixed", b"")
    add("dynamic", take(1500))
    seen, k = 0, 0
    while seen < 16 or k < 24:                                        # fixed and dynamic blocks begin at every bit offset 0..7
        add(("fixed", "dynamic", "fixed", "stored")[k % 4], take(int(rng.integers(1, 90))))
        seen = len({(b["kind"], b["at"] % 8) for b in w.blocks if b["kind"] != "stored"})
        k += 1
        assert k < 400
    add("fixed", b"", last=True)
    out["block_mix/all_kinds"] = (w, bytes(hist))
    for name, n in (("stored_65535", 65535), ("stored_largest_in_bgzf", 65505)):
        w = Deflate()
        data = bytes(rng.integers(0, 256, n).astype(np.uint8))
        w.stored(data, True)
        out["block_mix/" + name] = (w, data)
    return out


def _many_blocks(rng, records):
    data = records[:65280]
    toks = tokenize(data)
    while True:
        sizes = rng.integers(40, 4001, 48)
        sizes = (sizes * (63500.0 / sizes.sum())).astype(int)
        if sizes.min() >= 60 and sizes.max() <= 3900:
            break
    w = Deflate()
    k, blk = 0, 0
    while k < len(toks):
        part, got = [], 0
        while k < len(toks) and (got < sizes[blk] or blk == 47):
            part.append(toks[k])
            got += 1 if isinstance(toks[k], int) else toks[k][0]
            k += 1
        w.auto(part, k == len(toks), limit=(15, 11, 9, 8)[blk % 4])
        blk += 1
    assert blk == 48, blk
    return w, data


def _isize_edges(rng, records):
    out = OrderedDict()
    for n in (0, 1, 15, 16, 17, 159, 160, 161):
        w = Deflate()
        data = records[1000:1000 + n]
        if n == 0:
            w.fixed([], True)
        else:
            w.auto(tokenize(data), True)
        out["isize_edges/%d" % n] = (w, data)
    rec = records[2000:2036]
    for n in (65535, 65536):
        for kind, data in (("run", b"\x5a" * n), ("records", (rec * 2000)[:n])):
            w = Deflate()
            w.auto(tokenize(data), True)
            out["isize_edges/%d_%s" % (n, kind)] = (w, data)
    return out


BAM_FOREIGN_READS = 6000
BAM_FOREIGN_SIZES = (65280, 12345, 65536, 777, 40001, 65280, 3, 60001, 33333, 65535)


@functools.lru_cache(maxsize=None)
def bam_stream():
    """an uncompressed BAM stream made with the package's own tools: real-shaped records (names, 100 bases and qualities)"""
    from bamsignals_amd import write_columns_as_bam
    from bamsignals_amd.synth import synth_reads
    cols = synth_reads(BAM_FOREIGN_READS, [3_000_000, 500_000], seed=1951)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "f.bam")
        write_columns_as_bam(path, ["a", "b"], cols, l_seq=100, seed=7)
        return gzip.decompress(open(path, "rb").read())


def _bam_foreign():
    """the stream re-compressed block by block: tokenized with both knobs on, one dynamic block of lengths_from_freq(15) each"""
    stream = bam_stream()
    out, at, k = OrderedDict(), 0, 0
    while at < len(stream):
        n = BAM_FOREIGN_SIZES[k % len(BAM_FOREIGN_SIZES)]
        data = stream[at:at + n]
        w = Deflate()
        w.auto(tokenize(data), True)
        out["bam_foreign/%04d" % k] = (w, data)
        at += n
        k += 1
    return out


FAMILIES = ("flat_long", "deep", "dist_edges", "dsyms_long", "few_distance_codes", "header_forms", "block_mix", "many_blocks",
            "isize_edges", "bam_foreign")


@functools.lru_cache(maxsize=None)
def _built():
    rng = np.random.default_rng(1951)
    cases = OrderedDict()                                              # name -> (Deflate, expected bytes)

    def put(name, w, data=None):
        if data is None:
            data = expand([t for b in w.blocks for t in b.get("tokens", [])])
        cases[name] = (w, data)

    put("flat_long/one", _flat_long(rng, 1))
    put("flat_long/twice", _flat_long(rng, 2))
    put("flat_long/six", _flat_long(rng, 6))
    put("deep/deep", _deep(rng))
    for name, toks in _dist_edges(rng).items():
        w = Deflate()
        if name.endswith("lengths"):
            w.fixed(toks, True)
        else:
            w.auto(toks, True)
        put(name, w)
    put("dsyms_long/dsyms_long", _dsyms_long(rng))
    for fam in (_few_distance_codes, _header_forms):
        for name, w in fam(rng).items():
            put(name, w)
    records = bam_stream()[4096:]
    for name, (w, data) in _block_mix(rng, records).items():
        put(name, w, data)
    put("many_blocks/many_blocks", *_many_blocks(rng, records[100_000:]))
    for name, (w, data) in _isize_edges(rng, records[200_000:]).items():
        put(name, w, data)
    for name, (w, data) in _bam_foreign().items():
        put(name, w, data)
    return cases


def corpus():
    """name ('family/case') -> (raw DEFLATE stream, the bytes it inflates to), in a fixed order"""
    return OrderedDict((name, (w.getvalue(), data)) for name, (w, data) in _built().items())


def corpus_blocks():
    """name -> the log of the DEFLATE blocks written for it (kind, code lengths, tokens, header fields, first bit)"""
    return OrderedDict((name, w.blocks) for name, (w, _) in _built().items())


def family_of(name):
    return name.split("/")[0]


def family_file(family, names=None):
    """A BGZF file of the family's cases, one block each (cases that fit no BGZF block left out: only a stored block of
    65,535 bytes), and the EOF block -> (bytes, blocks without the EOF block, bytes they inflate to).  bam_foreign: every
    eighth block is followed by an empty block, every fifth carries an 8-byte subfield in front of BC."""
    out, k, empties, total = b"", 0, 0, 0
    for name, (raw, data) in corpus().items():
        if family_of(name) != family or (names is not None and name not in names) or not fits_bgzf(raw, data):
            continue
        if family == "bam_foreign" and k and k % 8 == 0:
            out += EOF_BLOCK
            empties += 1
        out += bgzf_block(raw, data, b"ZZ\x04\x00bsig" if family == "bam_foreign" and k % 5 == 4 else b"")
        k += 1
        total += len(data)
    n = k + empties
    return out + EOF_BLOCK, n, total


# the invalid cases the lane decoder accepts and zlib does not: incomplete code sets whose missing codes are never used
LANE_ACCEPTS = ("incomplete_ll_unused", "incomplete_dist_unused", "incomplete_cl_unused")
# ... and those that fail at the code tables or at a checked symbol, before anything can go wrong behind them
TABLE_LEVEL = ("oversubscribed_ll", "oversubscribed_dist", "oversubscribed_cl", "no_code_for_256", "four_cl_codes_no_lengths",
               "unused_distance_code", "match_without_distance_codes", "fixed_symbol_286", "fixed_symbol_287",
               "fixed_distance_30", "fixed_distance_31", "dist_is_op_plus_1")


@functools.lru_cache(maxsize=None)
def _invalid():
    rng = np.random.default_rng(3)
    text = [int(x) for x in rng.integers(97, 105, 120)]
    toks = text[:60] + [(9, 13), (30, 60)] + text[60:] + [(4, 1)]
    lf, df = token_freq(toks)
    ll, d = lengths_from_freq(lf, 15), lengths_from_freq(df, 15)
    n = len(expand(toks))
    out = OrderedDict()

    def put(name, out_len, build):
        w = Deflate()
        build(w)
        out[name] = (w.getvalue(), out_len)

    put("oversubscribed_ll", n, lambda w: w.dynamic([8] * 257, d, [], True, check=False))
    put("oversubscribed_dist", n, lambda w: w.dynamic(ll, [1, 1, 1], [], True, check=False))
    cl3 = [0] * 19
    cl3[0] = cl3[8] = cl3[16] = 1
    put("oversubscribed_cl", n, lambda w: w.dynamic(ll, d, [], True, cl_items=[(8, 1)] * 258, cl_lens=cl3, check=False))
    put("no_code_for_256", 120, lambda w: w.dynamic([8] * 256, [0], text, True, hlit=257, eob=False))
    put("four_cl_codes_no_lengths", 0, lambda w: w.dynamic([], [0], [], True, cl_items=[(18, 138), (18, 120)], hclen=4, eob=False))
    put("unused_distance_code", 70, lambda w: w.dynamic(ll, [1], text[:60] + [("ll", 258), ("raw", 1, 1)], True))
    put("match_without_distance_codes", 70, lambda w: w.dynamic(ll, [0], text[:60] + [("ll", 258), ("raw", 0, 5)], True))
    for s in (286, 287):
        put("fixed_symbol_%d" % s, 70, lambda w, s=s: w.fixed(text[:60] + [("ll", s), ("raw", 0, 5)], True))
    for s in (30, 31):
        put("fixed_distance_%d" % s, 70, lambda w, s=s: w.fixed(text[:60] + [("ll", 260), ("d", s)], True))

    def bad_dist(w):
        t = text[:3] + [(3, 4)]
        w.auto(t, True)
    put("dist_is_op_plus_1", 6, bad_dist)
    put("match_passes_out_len_by_one", 14, lambda w: w.auto(text[:5] + [(10, 5)], True))
    put("hlit_287", n, lambda w: w.dynamic(ll + [0], d, toks, True, hlit=287, check=False))
    put("hdist_31", n, lambda w: w.dynamic(ll, d + [0] * (31 - len(d)), toks, True, hdist=31, check=False))
    seq = ll[:max(257, max(k + 1 for k, l in enumerate(ll) if l))] + d[:max(k + 1 for k, l in enumerate(d) if l)]
    put("item_16_first", n, lambda w: w.dynamic(ll, d, toks, True, cl_items=[(16, 3)] + rle_items(seq)[1:], check=False))
    put("repeat_past_the_lengths", n, lambda w: w.dynamic(ll, d, toks, True, cl_items=rle_items(seq)[:-1] + [(18, 138)], check=False))
    put("stored_nlen_wrong", 50, lambda w: w.stored(bytes(text[:50]), True, nlen=0x1234))

    def one_bit_early(w):                                              # the end-of-block code's last bit opens the last byte
        for k in range(16):
            w2 = Deflate()
            w2.dynamic(ll, d, toks + text[:k], True)
            if w2.bitpos() % 8 == 1:
                w.dynamic(ll, d, toks + text[:k], True)
                return k
        raise AssertionError("no such stream")
    w = Deflate()
    k = one_bit_early(w)
    out["ends_one_bit_early"] = (w.getvalue()[:-1], n + k)
    put("inflates_to_out_len_minus_1", n + 1, lambda w: w.dynamic(ll, d, toks, True))
    # the documented difference: incomplete sets whose missing codes nobody uses (zlib refuses them at the header)
    ll_inc = [0] * 257
    ll_inc[97] = ll_inc[98] = ll_inc[256] = 2
    put("incomplete_ll_unused", 40, lambda w: w.dynamic(ll_inc, [0], [97, 98] * 20, True))
    assert sum(1 for f in df if f) == 3
    put("incomplete_dist_unused", n, lambda w: w.dynamic(ll, [2 if f else 0 for f in df], toks, True))
    cl_inc = [0] * 19
    for s in set(s for s, _ in rle_items(seq)):
        cl_inc[s] = 5
    put("incomplete_cl_unused", n, lambda w: w.dynamic(ll, d, toks, True, cl_lens=cl_inc))
    return out


def invalid():
    """name -> (raw DEFLATE stream, the output length it is decoded for): each must fail"""
    return OrderedDict(_invalid())
