"""The resident read layout (csrc/bsig_types.h; built by csrc/runtime.hip: layout_from_device) restated in plain numpy
with 64-bit integers, and a reader of the reads file that `Reads.save` writes (csrc/runtime.hip: bsig_reads_save), so
that tests/test_layout_gpu.py can hold every byte of a layout to the restatement.  Nothing here imports the library.

A layout, from the file or restated, is a dict:
  n_ref, n_reads, n_classes, n_codes, ref_len, ref_unit0, ref_units,
  fmtab (uint32[512], or None without a pair table),
  cls: five dicts of n, maxspan, kshift, col_cap, idx_entries and the columns pos / end / fm / tlen / idx -- a column
       the class does not have, and every column of an empty class, is None; a column has col_cap words (zeros from n
       on), idx has idx_entries - 1 (the index's spare last entry is never written, and never compared);
a layout read from a file has `stamp` and `checksum` too, a restated one `read_class`: the class of every input read."""
import struct

import numpy as np

MAGIC, VERSION = b"BSIGRDS1", 4
N_CLASSES, PACKED = 5, 4
PACK_CODES, PACK_POS_BITS, UNIT_SHIFT = 512, 15, 16
CHUNK = 2048                              # reads per workgroup of the layout kernels
HEADER = "<8sIIqIIQ" + "qiiQQ" * N_CLASSES + "QII"
HEADER_BYTES = struct.calcsize(HEADER)    # 216
COLUMNS = ("pos", "end", "fm", "tlen")    # the order of a class's columns in the file and in the checksum
COL_DTYPE = dict(pos=np.int32, end=np.int32, fm=np.uint32, tlen=np.int32, idx=np.uint32)


def class_has(c, col):
    """pos: all but the packed class; end: classes 2 and 3; fm, tlen: all"""
    return c != PACKED if col == "pos" else c in (2, 3) if col == "end" else True


def pad64(v):
    return (int(v) + 63) & ~63


def empty_class():
    return dict(n=0, maxspan=0, kshift=0, col_cap=0, idx_entries=0, pos=None, end=None, fm=None, tlen=None, idx=None)


# ---------------------------------------------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------------------------------------------
def read_layout(path):
    """Parse a reads file.  Refuses a wrong magic or version and a file whose size is not the header's file_bytes."""
    raw = open(path, "rb").read()
    assert len(raw) >= HEADER_BYTES, "%s: shorter than a reads file's header" % path
    h = struct.unpack_from(HEADER, raw, 0)
    magic, version, n_ref, n_reads, stamp_len, n_classes, file_bytes = h[:7]
    assert magic == MAGIC, "%s: not a reads file (magic %r)" % (path, magic)
    assert version == VERSION, "%s: reads file of version %d, not %d" % (path, version, VERSION)
    assert file_bytes == len(raw), "%s: header says %d bytes, the file has %d" % (path, file_bytes, len(raw))
    checksum, n_codes, _reserved = h[7 + 5 * N_CLASSES:]
    at = [pad64(HEADER_BYTES)]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype=dtype, count=int(count), offset=at[0]).copy()
        at[0] += pad64(a.nbytes)
        return a

    out = dict(n_ref=n_ref, n_reads=n_reads, n_classes=n_classes, n_codes=n_codes, checksum=checksum)
    out["stamp"] = take(np.uint8, stamp_len).tobytes().decode()
    out["ref_len"] = take(np.int32, n_ref)
    out["ref_unit0"] = take(np.uint32, n_ref)
    out["ref_units"] = take(np.uint32, n_ref)
    out["fmtab"] = take(np.uint32, PACK_CODES) if n_codes else None
    out["cls"] = []
    for c in range(N_CLASSES):
        n, maxspan, kshift, col_cap, idx_entries = h[7 + 5 * c:12 + 5 * c]
        C = empty_class()
        C.update(n=n, maxspan=maxspan, kshift=kshift, col_cap=col_cap, idx_entries=idx_entries)
        if n:
            for col in COLUMNS:
                if class_has(c, col):
                    C[col] = take(COL_DTYPE[col], col_cap)
            C["idx"] = take(np.uint32, idx_entries)[:idx_entries - 1]
        out["cls"].append(C)
    assert at[0] == len(raw), "%s: %d bytes behind the last column" % (path, len(raw) - at[0])
    return out


def write_layout(path, layout, stamp="", checksum=0, spare=0):
    """The file of a layout, as bsig_reads_save lays it out (`spare`: what every index's unwritten last entry holds)."""
    parts = []

    def put(b):
        parts.append(b + bytes(pad64(len(b)) - len(b)))

    sb = stamp.encode()
    n_ref = int(layout["n_ref"])
    body = [sb, np.asarray(layout["ref_len"], np.int32).tobytes(), np.asarray(layout["ref_unit0"], np.uint32).tobytes(),
            np.asarray(layout["ref_units"], np.uint32).tobytes()]
    if layout["n_codes"]:
        body.append(np.asarray(layout["fmtab"], np.uint32).tobytes())
    recs = []
    for c, C in enumerate(layout["cls"]):
        recs += [C["n"], C["maxspan"], C["kshift"], C["col_cap"], C["idx_entries"]]
        if not C["n"]:
            continue
        for col in COLUMNS:
            if class_has(c, col):
                body.append(np.asarray(C[col], COL_DTYPE[col]).tobytes())
        body.append(np.concatenate([C["idx"], [spare]]).astype(np.uint32).tobytes())
    file_bytes = pad64(HEADER_BYTES) + sum(pad64(len(b)) for b in body)
    put(struct.pack(HEADER, MAGIC, VERSION, n_ref, int(layout["n_reads"]), len(sb), int(layout["n_classes"]), file_bytes,
                    *[int(v) for v in recs], int(checksum), int(layout["n_codes"]), 0))
    for b in body:
        put(b)
    with open(path, "wb") as fp:
        fp.write(b"".join(parts))


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def cigar_end(pos, flag, cigar_off, cigar):
    """bam_endpos - 1 of every read: pos + (bases of the reference its CIGAR consumes: ops M 0, D 2, N 3, = 7, X 8) - 1;
    flag 0x4, a zero sum or an empty CIGAR give one base."""
    pos = np.asarray(pos, np.int64)
    off = np.asarray(cigar_off, np.int64)
    cg = np.asarray(cigar, np.int64)
    op = cg & 0xF
    eats = (op == 0) | (op == 2) | (op == 3) | (op == 7) | (op == 8)
    run = np.concatenate([[0], np.cumsum(np.where(eats, cg >> 4, 0))])
    rlen = run[off[1:]] - run[off[:-1]]
    rlen[(np.asarray(flag, np.int64) & 4) != 0] = 0
    rlen[rlen == 0] = 1
    return pos + rlen - 1


def sample_stride(n):
    """the pair table counts every `stride`-th chunk of 2,048 reads: all of them up to 2,047 chunks"""
    return max(1, ((n + CHUNK - 1) // CHUNK) // 1024)


def pair_table(pos, end, flag, mapq):
    """(keys, counts) of the (flag, mapq) pairs of the sampled short reads, key = flag | mapq << 12, most frequent first,
    equal counts by key ascending: the first 512 get the codes 0 .. 511 (the sample: conftest.expected_packed)."""
    pos, end = np.asarray(pos, np.int64), np.asarray(end, np.int64)
    flag, mapq = np.asarray(flag, np.int64), np.asarray(mapq, np.int64)
    span = end - pos + 1
    cand = (span >= 1) & (span <= 256) & (flag < 4096) & (pos >= 0)
    sampled = (np.arange(len(pos)) // CHUNK) % sample_stride(len(pos)) == 0
    keys, counts = np.unique((flag | mapq << 12)[cand & sampled], return_counts=True)
    order = sorted(range(len(keys)), key=lambda j: (-int(counts[j]), int(keys[j])))
    return keys[order], counts[order]


def bucket_shift(n_class, total_bp, packed, bucket_reads=16.0):
    """layout_from_device's choice of a class's bucket width, operation by operation in double precision"""
    min_shift = 4
    while (total_bp >> min_shift) >= (1 << 32):
        min_shift += 1
    per_bucket = max(1.0, float(bucket_reads))
    bp_per_bucket = per_bucket * float(total_bp) / float(n_class)
    max_shift = PACK_POS_BITS if packed else UNIT_SHIFT
    k = 4
    while k < max_shift and float(1 << (k + 1)) <= bp_per_bucket:
        k += 1
    k = max(k, min_shift)
    assert k <= max_shift, "genome too large for the bucket index"
    return k


def read_classes(pos, end, flag, packed_mask):
    span = np.asarray(end, np.int64) - np.asarray(pos, np.int64) + 1
    flag = np.asarray(flag, np.int64)
    cls = np.where(span <= 256, 0, np.where((span <= 4096) & (flag < 4096), 1, np.where(span <= 65536, 2, 3)))
    cls[packed_mask] = PACKED
    return cls


def expected_layout(ref_len, ref_off, pos, end, flag, mapq, tlen, bucket_reads=16.0, pack=True):
    """The layout of coordinate-sorted columns, from bsig_types.h's header comment."""
    from conftest import expected_packed
    ref_len, ref_off = np.asarray(ref_len, np.int64), np.asarray(ref_off, np.int64)
    pos, end = np.asarray(pos, np.int64), np.asarray(end, np.int64)
    flag, mapq, tlen = np.asarray(flag, np.int64), np.asarray(mapq, np.int64), np.asarray(tlen, np.int64)
    n, n_ref = len(pos), len(ref_len)
    # 1. references back to back in units of 65,536 bp
    units = (ref_len >> UNIT_SHIFT) + 1
    unit0 = np.concatenate([[0], np.cumsum(units)[:-1]]) if n_ref else np.zeros(0, np.int64)
    total_bp = int(units.sum()) << UNIT_SHIFT
    out = dict(n_ref=n_ref, n_reads=n, n_classes=0, n_codes=0, ref_len=ref_len.astype(np.int32),
               ref_unit0=unit0.astype(np.uint32), ref_units=units.astype(np.uint32), fmtab=None,
               cls=[empty_class() for _ in range(N_CLASSES)])
    if n == 0 or n_ref == 0:
        return out
    # 2. the pair table
    key = flag | mapq << 12
    packed_mask = np.zeros(n, bool)
    code = np.zeros(n, np.int64)
    if pack:
        keys, _ = pair_table(pos, end, flag, mapq)
        table = keys[:PACK_CODES]
        if len(table):
            packed_mask, n_codes = expected_packed(pos, end, flag, mapq, ref_off, ref_len)
            assert n_codes == len(table)
            fmtab = np.zeros(PACK_CODES, np.uint32)
            fmtab[:len(table)] = (table & 0xFFF) | (table >> 12) << 16
            out["fmtab"], out["n_codes"] = fmtab, len(table)
            by_key = np.argsort(table)
            at = np.searchsorted(table[by_key], key[packed_mask])
            code[packed_mask] = by_key[at]
            assert np.array_equal(table[code[packed_mask]], key[packed_mask])
    # 3. - 5. classes, the stable partition, the words
    cls = read_classes(pos, end, flag, packed_mask)
    out["read_class"] = cls
    rid = np.searchsorted(ref_off[1:], np.arange(n), side="right")
    ref_bp = units[rid] << UNIT_SHIFT
    g = (unit0[rid] << UNIT_SHIFT) + np.clip(pos, 0, ref_bp - 1)
    span1 = end - pos
    for c in range(N_CLASSES):
        m = np.flatnonzero(cls == c)                    # ascending: BAM order kept
        if not len(m):
            continue
        C = out["cls"][c]
        nc = len(m)
        cap = (nc + 3) // 4 * 4 + 4                     # 6.
        if c == 0:
            fm = flag[m] | mapq[m] << 16 | span1[m] << 24
        elif c == 1:
            fm = flag[m] | mapq[m] << 12 | span1[m] << 20
        elif c == PACKED:
            fm = (pos[m] & 0x7FFF) | span1[m] << PACK_POS_BITS | code[m] << 23
        else:
            fm = flag[m] | mapq[m] << 16

        def column(v, dtype):
            a = np.zeros(cap, dtype)
            a[:nc] = v.astype(dtype)
            return a
        if c != PACKED:
            C["pos"] = column(pos[m], np.int32)
        if c in (2, 3):
            C["end"] = column(end[m], np.int32)
        assert fm.min() >= 0 and fm.max() < 1 << 32
        C["fm"] = column(fm, np.uint32)
        C["tlen"] = column(tlen[m], np.int32)
        k = bucket_shift(nc, total_bp, c == PACKED, bucket_reads)         # 7.
        n_buckets = total_bp >> k                                          # 8.
        gb = g[m] >> k
        assert np.all(np.diff(gb) >= 0), "reads not sorted by position inside every reference"
        C["idx"] = np.searchsorted(gb, np.arange(n_buckets + 1), side="left").astype(np.uint32)
        C.update(n=nc, maxspan=int(span1[m].max()) + 1, kshift=k, col_cap=cap, idx_entries=n_buckets + 2)   # 9.
        out["n_classes"] += 1
    return out


def expected_info(layout):
    """what Reads.info() says of a layout, but for the bytes it holds on the device"""
    return dict(n_reads=layout["n_reads"], n_classes=layout["n_classes"], n_codes=layout["n_codes"],
                class_n=[C["n"] for C in layout["cls"]], class_maxspan=[C["maxspan"] for C in layout["cls"]],
                class_bucket_shift=[C["kshift"] for C in layout["cls"]])


_MIX = np.uint64(0xD6E8FEB86659FD93)


def words_checksum(words, salt):
    """k_checksum: the sum over i of mix(word i, i + salt), modulo 2^64"""
    w = np.ascontiguousarray(words).view(np.uint32).astype(np.uint64)
    i = np.arange(len(w), dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (w << np.uint64(32) | (i * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) ^ (i + np.uint64(salt)) * _MIX
        x ^= x >> np.uint64(32)
        x *= _MIX
        x ^= x >> np.uint64(29)
        return int(np.add.reduce(x, dtype=np.uint64)) if len(x) else 0


def expected_checksum(layout):
    """layout_checksum: every column over its col_cap words and every index over its idx_entries - 1, each under a salt
    of its own -- from 1, + 0x100000001 after each of a non-empty class's four column slots (whether it has the column
    or not) and after its index; an empty class takes no salt; the pair table comes last."""
    total, salt = 0, 1
    for C in layout["cls"]:
        if not C["n"]:
            continue
        for col in COLUMNS:
            if C[col] is not None:
                assert len(C[col]) == C["col_cap"]
                total += words_checksum(C[col], salt)
            salt += 0x100000001
        assert len(C["idx"]) == C["idx_entries"] - 1
        total += words_checksum(C["idx"], salt)
        salt += 0x100000001
    if layout["fmtab"] is not None:
        total += words_checksum(layout["fmtab"], salt)
    return total & (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------
# a layout read back into reads
# ---------------------------------------------------------------------------------------------------------------
def decode_class(layout, c):
    """(pos, span, flag, mapq, tlen) of class c's reads, from its columns alone (the packed class: the position's high
    bits from the bucket the index files the read under, flag and mapq from the pair table)."""
    C = layout["cls"][c]
    n = C["n"]
    fm = C["fm"][:n].astype(np.int64)
    tlen = C["tlen"][:n].astype(np.int64)
    if c == PACKED:
        bucket = np.searchsorted(C["idx"].astype(np.int64), np.arange(n), side="right") - 1     # last b with idx[b] <= j
        gchunk = (bucket << C["kshift"]) >> PACK_POS_BITS                                       # kshift <= 15
        unit = gchunk >> (UNIT_SHIFT - PACK_POS_BITS)
        rid = np.searchsorted(layout["ref_unit0"].astype(np.int64), unit, side="right") - 1
        chunk_in_ref = gchunk - (layout["ref_unit0"].astype(np.int64)[rid] << (UNIT_SHIFT - PACK_POS_BITS))
        pos = chunk_in_ref << PACK_POS_BITS | fm & 0x7FFF
        word = layout["fmtab"].astype(np.int64)[fm >> 23]
        return pos, (fm >> PACK_POS_BITS & 0xFF) + 1, word & 0xFFFF, word >> 16, tlen
    pos = C["pos"][:n].astype(np.int64)
    if c == 0:
        return pos, (fm >> 24) + 1, fm & 0xFFFF, fm >> 16 & 0xFF, tlen
    if c == 1:
        return pos, (fm >> 20) + 1, fm & 0xFFF, fm >> 12 & 0xFF, tlen
    return pos, C["end"][:n].astype(np.int64) - pos + 1, fm & 0xFFFF, fm >> 16, tlen


def read_buckets(layout, c):
    """the bucket every read of class c is filed under: the last b with idx[b] <= j"""
    C = layout["cls"][c]
    return np.searchsorted(C["idx"].astype(np.int64), np.arange(C["n"]), side="right") - 1


# ---------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------
def layout_differences(got, want, checksum=True):
    """Every difference between two layouts as one line each: the class, the column, the first differing entry and how
    many differ -- never the arrays."""
    bad = []
    for k in ("n_ref", "n_reads", "n_classes", "n_codes"):
        if int(got[k]) != int(want[k]):
            bad.append("%s: %d, expected %d" % (k, got[k], want[k]))

    def arrays(name, a, b):
        if (a is None) != (b is None):
            bad.append("%s: %s, expected %s" % (name, "absent" if a is None else "present", "absent" if b is None else "present"))
        elif a is not None:
            if len(a) != len(b):
                bad.append("%s: %d entries, expected %d" % (name, len(a), len(b)))
            else:
                d = np.flatnonzero(np.asarray(a).astype(np.int64) != np.asarray(b).astype(np.int64))
                if len(d):
                    bad.append("%s: %d of %d entries differ, the first at %d: %d, expected %d"
                               % (name, len(d), len(a), d[0], a[d[0]], b[d[0]]))
    for k in ("ref_len", "ref_unit0", "ref_units", "fmtab"):
        arrays(k, got[k], want[k])
    for c in range(N_CLASSES):
        G, W = got["cls"][c], want["cls"][c]
        for k in ("n", "maxspan", "kshift", "col_cap", "idx_entries"):
            if int(G[k]) != int(W[k]):
                bad.append("class %d %s: %d, expected %d" % (c, k, G[k], W[k]))
        for col in COLUMNS + ("idx",):
            arrays("class %d %s" % (c, col), G[col], W[col])
    if checksum and "checksum" in got:
        want_sum = want["checksum"] if "checksum" in want else expected_checksum(want)
        if int(got["checksum"]) != want_sum:
            bad.append("checksum: %#x, expected %#x" % (got["checksum"], want_sum))
    return bad
