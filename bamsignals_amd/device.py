"""Handle-level host API over the C ABI: a device context, reads resident in HBM, plans.

This is plumbing for the reference-shaped entry points in ``wrappers.py`` and for ``bench.py``;
all arithmetic happens in the HIP kernels (csrc/kernels.hip).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class _PinnedBlock:
    """Owner of one bsig_host_alloc() block; freed when the last numpy view of it is collected."""

    def __init__(self, nbytes):
        self._lib = _lib.load()
        p = C.c_void_p()
        _lib.check(self._lib.bsig_host_alloc(int(nbytes), C.byref(p)))
        self.ptr = p.value
        self.buf = (C.c_char * max(int(nbytes), 1)).from_address(self.ptr)

    def __del__(self):
        if getattr(self, "ptr", None):
            self._lib.bsig_host_free(C.c_void_p(self.ptr))
            self.ptr = None


def pinned_empty(n, dtype):
    """numpy array of ``n`` elements in page-locked host memory."""
    dtype = np.dtype(dtype)
    block = _PinnedBlock(n * dtype.itemsize)
    arr = np.frombuffer(block.buf, dtype=dtype, count=n)
    # the ctypes buffer keeps `block` alive through arr.base; tie them explicitly as well
    block.buf._owner = block
    return arr


class Context:
    """One GPU + the HIP stream the kernels are launched on."""

    def __init__(self, device=0, stream=None):
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.bsig_ctx_create(int(device), C.c_void_p(stream or 0), C.byref(h)))
        self._h = h
        self.device = int(device)

    @property
    def stream(self):
        return self._lib.bsig_ctx_stream(self._h)

    def sync(self):
        _lib.check(self._lib.bsig_ctx_sync(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bsig_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class Reads:
    """Read columns resident in HBM (span classes + bucket index, see csrc/bsig_types.h).

    ``end`` may be omitted when ``cigar_off``/``cigar`` (packed ``len<<4|op``) are given: the GPU
    then derives ``bam_endpos - 1`` itself.

    ``spliced=True`` (needs ``cigar_off``/``cigar``): the reads are split at their N gaps and the rows are their aligned
    blocks, each with its read's flag, mapq and tlen (csrc/splice.hip); ``info()["n_reads"]`` then counts blocks.  Such
    reads give plain coverage only: every other plan refuses them.

    ``bases=True`` (needs ``cigar_off``/``cigar`` and ``seq_off``, ``seq``, ``qual``): an ordinary plain set that also keeps
    what the reads say -- read i owns bases ``seq_off[i] .. seq_off[i + 1]``; base g of the whole is nibble g of ``seq``
    (BAM's 4-bit codes, the high half of byte ``g // 2`` where g is even) and byte g of ``qual`` (0xFF: missing) -- as a
    base table beside the reads (csrc/nucleotides.hip).  Every plan works on it as on a plain set; ``nucleotides`` needs it.
    """

    def __init__(self, ctx, ref_len, ref_off, pos, flag, mapq, tlen, end=None, cigar_off=None, cigar=None, *, spliced=False,
                 bases=False, seq_off=None, seq=None, qual=None):
        self._lib = _lib.load()
        self.ctx = ctx
        ref_len = _i32(ref_len)
        ref_off = np.ascontiguousarray(ref_off, dtype=np.int64)
        pos = _i32(pos)
        flag = np.ascontiguousarray(flag, dtype=np.uint16)
        mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
        tlen = _i32(tlen)
        n = len(pos)
        if not (len(flag) == len(mapq) == len(tlen) == n):
            raise ValueError("read columns differ in length")
        cols = _lib.Columns()
        cols.n_reads = n
        cols.n_ref = len(ref_len)
        cols.ref_len = _ptr(ref_len).value
        cols.ref_off = _ptr(ref_off).value
        cols.pos, cols.flag, cols.mapq, cols.tlen = (_ptr(a).value for a in (pos, flag, mapq, tlen))
        keep = [ref_len, ref_off, pos, flag, mapq, tlen]
        if spliced and (cigar_off is None or cigar is None):
            raise ValueError("spliced reads need cigar_off + cigar: an end column does not say where the N gaps lie")
        if bases and spliced:
            raise ValueError("a set is spliced or has bases, not both")
        if bases and (cigar_off is None or cigar is None or seq_off is None or seq is None or qual is None):
            raise ValueError("reads with bases need cigar_off + cigar and seq_off, seq, qual")
        if end is not None and not spliced and not bases:
            end = _i32(end)
            if len(end) != n:
                raise ValueError("end column differs in length")
            cols.end = _ptr(end).value
            keep.append(end)
        if end is None or spliced or bases:
            if cigar_off is None or cigar is None:
                raise ValueError("need either end or cigar_off + cigar")
            cigar_off = np.ascontiguousarray(cigar_off, dtype=np.int64)
            cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
            if len(cigar_off) != n + 1:
                raise ValueError("cigar_off must have n_reads + 1 entries")
            cols.cigar_off = _ptr(cigar_off).value
            cols.cigar = _ptr(cigar).value
            keep += [cigar_off, cigar]
        h = C.c_void_p()
        if bases:
            seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            qual = np.ascontiguousarray(qual, dtype=np.uint8)
            if len(seq_off) != n + 1:
                raise ValueError("seq_off must have n_reads + 1 entries")
            total = int(seq_off[-1])
            if len(qual) < total or 2 * len(seq) < total:
                raise ValueError("seq or qual is shorter than seq_off says")
            bc = _lib.BaseColumns()
            bc.seq_off, bc.seq, bc.qual = (_ptr(a).value for a in (seq_off, seq, qual))
            _lib.check(self._lib.bsig_reads_upload_bases(ctx._h, C.byref(cols), C.byref(bc), C.byref(h)))
        else:
            upload = self._lib.bsig_reads_upload_spliced if spliced else self._lib.bsig_reads_upload
            _lib.check(upload(ctx._h, C.byref(cols), C.byref(h)))
        self._h = h
        self.n_reads = n
        self.n_ref = len(ref_len)

    @classmethod
    def from_bam(cls, ctx, bam, threads=0, *, spliced=False, bases=False):
        """The whole of an open ``bamio.BamFile`` decoded to HBM: BGZF inflate on the CPU thread pool,
        records -> columns on the GPU (csrc/devdecode.hip; CPU decode where the file needs it).  ``spliced``: the reads
        split at their N gaps, the gaps found on the GPU while the stream is resident.  ``bases``: a plain set with its base
        table (bases and qualities are decoded on the host)."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self.ctx = ctx
        h = C.c_void_p()
        if bases and spliced:
            raise ValueError("a set is spliced or has bases, not both")
        decode = self._lib.bsig_reads_from_bam_spliced if spliced else self._lib.bsig_reads_from_bam
        if bases:
            decode = self._lib.bsig_reads_from_bam_bases
        _lib.check(decode(ctx._h, bam._h, int(threads), C.byref(h)))
        self._h = h
        self.n_ref = len(bam.ref_len)
        self.n_reads = self.info()["n_reads"]
        return self

    @classmethod
    def from_bam_multi(cls, ctxs, bam, threads=0):
        """The whole BAM resident on every context's GPU: each GPU decodes one share of the BGZF blocks,
        the column shares are exchanged over xGMI.  Returns (list of Reads, sharded?)."""
        lib = _lib.load()
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c._h for c in ctxs])
        hs = (C.c_void_p * n)()
        sharded = C.c_int32(0)
        _lib.check(lib.bsig_reads_from_bam_multi(arr, n, bam._h, int(threads), hs, C.byref(sharded)))
        out = []
        for k in range(n):
            self = cls.__new__(cls)
            self._lib = lib
            self.ctx = ctxs[k]
            self._h = C.c_void_p(hs[k])
            self.n_ref = len(bam.ref_len)
            self.n_reads = self.info()["n_reads"]
            out.append(self)
        return out, bool(sharded.value)

    @classmethod
    def from_bam_regions(cls, ctx, bam, rid, beg, end, threads=0, *, spliced=False, bases=False):
        """The records the BAI lists for the regions [beg, end) (0-based) decoded to HBM -- a superset
        of the overlapping records, each once, in file order (what ``BamFile.decode(rid, beg, end)``
        returns on the host)."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self.ctx = ctx
        rid = np.ascontiguousarray(rid, dtype=np.int32)
        beg = np.ascontiguousarray(beg, dtype=np.int64)
        end = np.ascontiguousarray(end, dtype=np.int64)
        if not (len(rid) == len(beg) == len(end)):
            raise ValueError("region arrays differ in length")
        h = C.c_void_p()
        if bases and spliced:
            raise ValueError("a set is spliced or has bases, not both")
        decode = self._lib.bsig_reads_from_bam_regions_spliced if spliced else self._lib.bsig_reads_from_bam_regions
        if bases:
            decode = self._lib.bsig_reads_from_bam_regions_bases
        _lib.check(decode(ctx._h, bam._h, len(rid), _ptr(rid), _ptr(beg), _ptr(end), int(threads), C.byref(h)))
        self._h = h
        self.n_ref = len(bam.ref_len)
        self.n_reads = self.info()["n_reads"]
        return self

    def save(self, path, stamp=""):
        """Write the resident layout to ``path`` (bsig_reads_save); ``stamp`` ties it to its source."""
        _lib.check(self._lib.bsig_reads_save(self._h, str(path).encode(), str(stamp).encode()))

    @classmethod
    def load(cls, ctx, path, stamp=""):
        """Resident reads from a file written by ``save`` (fails if ``stamp`` differs)."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self.ctx = ctx
        h = C.c_void_p()
        _lib.check(self._lib.bsig_reads_load(ctx._h, str(path).encode(), str(stamp).encode(), C.byref(h)))
        self._h = h
        self.n_reads = self.info()["n_reads"]
        self.n_ref = None
        return self

    def clone(self, ctx):
        """A copy of these resident reads on ``ctx``'s GPU (device-to-device)."""
        other = type(self).__new__(type(self))
        other._lib = self._lib
        other.ctx = ctx
        h = C.c_void_p()
        _lib.check(self._lib.bsig_reads_clone(self._h, ctx._h, C.byref(h)))
        other._h = h
        other.n_ref, other.n_reads = self.n_ref, self.n_reads
        return other

    @property
    def spliced(self):
        """Are the rows aligned blocks of reads split at their N gaps?"""
        return bool(self._lib.bsig_reads_is_spliced(self._h))

    @property
    def n_junction_rows(self):
        """Rows of a spliced set's junction table: one per N gap of a read (0 for a plain set)."""
        return int(self._lib.bsig_reads_n_junction_rows(self._h))

    def junctions(self, rid, loc, length, strand, mapqual=0, requiredF=0, filteredF=-1, min_anchor=0, ss=False):
        """The distinct junctions of every range with their supporting reads (csrc/junctions.hip), counted on the GPU from
        the set's junction table: ``(seg_off, start, end, count, max_anchor)`` -- range i owns entries ``seg_off[i] ..
        seg_off[i + 1]``, ``start`` / ``end`` are the gap's first and last base (0-based), ``count`` is uint32 of shape
        ``(n,)`` or, with ``ss``, ``(n, 2)`` (sense, antisense).  A junction belongs to a range that contains it whole; a
        row counts if it passes ``mapqual`` / ``requiredF`` / ``filteredF`` and its anchor is at least ``min_anchor``.
        Only a spliced set has a table."""
        rid, loc, length, strand = (_i32(a) for a in (rid, loc, length, strand))
        n = len(rid)
        if not (len(loc) == len(length) == len(strand) == n):
            raise ValueError("range arrays differ in length")
        h = C.c_void_p()
        _lib.check(self._lib.bsig_reads_junctions(self._h, n, _ptr(rid), _ptr(loc), _ptr(length), _ptr(strand), int(mapqual),
                                                  int(requiredF), int(filteredF), int(min_anchor), int(bool(ss)), C.byref(h)))
        return take_junctions(self._lib, h, ss)

    @property
    def has_bases(self):
        """Does the set keep a base table (``bases=True``)?"""
        return bool(self._lib.bsig_reads_has_bases(self._h))

    @property
    def base_table_bytes(self):
        """Bytes of the base table's arrays: 28 a read (and 16 for the closing offsets), 4 an operation, 1.5 a base,
        8 * (n_ref + 1); 0 without a table or with an empty one."""
        return int(self._lib.bsig_reads_base_table_bytes(self._h))

    def nucleotides(self, rid, loc, length, strand, mapqual=0, requiredF=0, filteredF=-1, min_base_qual=0, ss=False):
        """A / C / G / T / N / deletion counts per base of every range (csrc/nucleotides.hip), counted on the GPU from the
        set's base table: a list with one int32 array per range, ``(6, width)`` or with ``ss`` ``(2, 6, width)`` (sense,
        antisense) -- views of one buffer.  include/bamsignals_abi.h says what counts.  Only a set with bases has a table."""
        rid, loc, length, strand = (_i32(a) for a in (rid, loc, length, strand))
        n = len(rid)
        if not (len(loc) == len(length) == len(strand) == n):
            raise ValueError("range arrays differ in length")
        off = np.zeros(n + 1, dtype=np.int64)
        cells = int(self._lib.bsig_nucleotides_cells(n, _ptr(length), int(bool(ss)), _ptr(off)))
        if cells < 0:
            raise ValueError("a range has a negative width")
        out = np.zeros(max(cells, 1), dtype=np.int32)
        _lib.check(self._lib.bsig_reads_nucleotides_host(self._h, n, _ptr(rid), _ptr(loc), _ptr(length), _ptr(strand), int(mapqual),
                                                         int(requiredF), int(filteredF), int(min_base_qual), int(bool(ss)), _ptr(out)))
        return split_nucleotides(out, off, length, ss)

    def sites(self, rid, loc, length, strand, ref=None, min_depth=10, min_alt=2, frac=(1, 5), alt_mask=0x2F, mapqual=0, requiredF=0,
              filteredF=-1, min_base_qual=0, ss=False, timing=None):
        """The variant and mixed-allele sites of every range (csrc/sites.hip): the cells ``nucleotides`` would count, judged on
        the GPU where they are counted; only the sites come back: ``(seg_off, pos, alleles, counts)`` -- range i owns entries
        ``seg_off[i] .. seg_off[i + 1]``, ``pos`` is the cell's index in the range as the range reads, ``alleles`` is
        ``base | alt << 8``, ``counts`` int32 ``(n, 6)`` or with ``ss`` ``(n, 2, 6)``.  ``ref``: uint8 channel codes 0 .. 4,
        ``sum(length)`` of them, range after range in the range's reading direction, or None (the base channel is then the
        first of the largest counts).  ``frac``: ``(num, den)``.  include/bamsignals_abi.h says what a site is.  ``timing``: a
        list that receives the seconds of count + scan, fill and download.  Only a set with bases has a table."""
        from .sites import take_sites
        rid, loc, length, strand = (_i32(a) for a in (rid, loc, length, strand))
        n = len(rid)
        if not (len(loc) == len(length) == len(strand) == n):
            raise ValueError("range arrays differ in length")
        if ref is not None:
            ref = np.ascontiguousarray(ref, dtype=np.uint8)
            if ref.ndim != 1 or len(ref) != int(np.maximum(length, 0).astype(np.int64).sum()):
                raise ValueError("ref must hold one code per base of the ranges")
        h = C.c_void_p()
        _lib.check(self._lib.bsig_reads_sites(self._h, n, _ptr(rid), _ptr(loc), _ptr(length), _ptr(strand), int(mapqual), int(requiredF),
                                              int(filteredF), int(min_base_qual), int(bool(ss)), None if ref is None else _ptr(ref),
                                              int(min_depth), int(min_alt), int(frac[0]), int(frac[1]), int(alt_mask), C.byref(h)))
        if timing is not None:
            t = (C.c_double * 3)()
            self._lib.bsig_sites_result_timing(h, t)
            timing[:] = list(t)
        return take_sites(self._lib, h, bool(ss))

    @property
    def n_source_reads(self):
        """Reads a spliced set was made from, the rows of its read table (``info()["n_reads"]`` counts blocks); 0 for a
        plain set."""
        return int(self._lib.bsig_reads_n_source_reads(self._h))

    def gene_counts(self, model, mapqual=0, requiredF=0, filteredF=-1, strand="unstranded"):
        """Reads per gene (csrc/genecounts.hip): every read of the set's read table classified against ``model`` (a
        ``genecounts.GeneModel`` whose ``n_ref`` is the set's), on the GPU: ``(counts, summary)`` -- int64, one count per
        gene and the five of ``genecounts.SUMMARY_FIELDS`` (assigned, ambiguous, no_feature, filtered, unmapped), which add
        up to ``n_source_reads``.  ``strand``: "unstranded", "forward" or "reverse".  Only a spliced set has a read table."""
        from .genecounts import GeneModel, strand_code
        if not isinstance(model, GeneModel):
            raise TypeError("model must be a GeneModel")
        mode = strand_code(strand)
        counts = np.zeros(max(model.n_genes, 1), dtype=np.int64)
        summary = np.zeros(5, dtype=np.int64)
        _lib.check(self._lib.bsig_reads_gene_counts(self._h, model._h, int(mapqual), int(requiredF), int(filteredF), mode,
                                                    _ptr(counts), _ptr(summary)))
        return counts[:model.n_genes], summary

    @staticmethod
    def device_decode_timing():
        """Stage seconds of this thread's last ``from_bam`` (all 0 when it took the CPU decode)."""
        t = (C.c_double * 6)()
        _lib.load().bsig_device_decode_timing(t)
        return dict(zip(("block_scan", "inflate", "copy_wait", "gpu_parse", "total", "layout"), list(t)))

    def info(self):
        inf = _lib.ReadsInfo()
        _lib.check(self._lib.bsig_reads_get_info(self._h, C.byref(inf)))
        # class_*: [span <= 256 with a rare flag/mapq pair, <= 4096, <= 65536, longer, packed (span <= 256, one
        # word per read)]; n_codes = pairs in the packed class's table
        return dict(n_reads=inf.n_reads, hbm_bytes=inf.hbm_bytes, n_classes=inf.n_classes, n_codes=inf.n_codes,
                    class_n=list(inf.class_n), class_maxspan=list(inf.class_maxspan),
                    class_bucket_shift=list(inf.class_bucket_shift))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bsig_reads_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


def split_nucleotides(out, off, width, ss):
    """the flat cells of a nucleotide count -> one read-only (6, width) / (2, 6, width) view per range"""
    out.setflags(write=False)
    shape = (2, 6) if ss else (6,)
    return [out[int(a):int(b)].reshape(shape + (int(w),)) for a, b, w in zip(off[:-1], off[1:], width)]


def take_junctions(lib, handle, ss):
    """a bsig_junctions_result handle -> (seg_off, start, end, count, max_anchor); the handle is freed"""
    try:
        n_seg, n = int(lib.bsig_junctions_result_n_seg(handle)), int(lib.bsig_junctions_result_n_junctions(handle))
        out = [np.empty(n_seg + 1, dtype=np.int64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32),
               np.empty((n, 2) if ss else (n,), dtype=np.uint32), np.empty(n, dtype=np.int32)]
        _lib.check(lib.bsig_junctions_result_copy(handle, *[a.ctypes.data if a.size else None for a in out]))
    finally:
        lib.bsig_junctions_result_free(handle)
    return tuple(out)


def make_params(mode, tlen_filter=(), mapqual=0, binsize=1, shift=0, ss=False, requiredF=0,
                filteredF=-1, pe_mid=False, tspan=False, tile_cells=0, threads=0):
    p = _lib.Params()
    p.mode = mode
    p.mapqual = int(mapqual)
    p.binsize = int(binsize)
    p.shift = int(shift)
    p.ss = int(bool(ss))
    p.requiredF = int(requiredF)
    p.filteredF = int(filteredF)
    p.pe_mid = int(bool(pe_mid))
    p.tspan = int(bool(tspan))
    tf = [] if tlen_filter is None else [int(x) for x in tlen_filter]
    p.n_tlen_filter = len(tf)
    if len(tf) not in (0, 2):
        raise ValueError("tlen_filter must have 0 or 2 elements")
    for i, v in enumerate(tf):
        p.tlen_filter[i] = v
    p.tile_cells = int(tile_cells)
    p.threads = int(threads)
    return p


class _PlanBase:
    """What every kind of plan shares: the range arrays as contiguous int32 of one length, the handle's life, ``stats``."""

    def _ranges(self, ctx, reads, rid, loc, length, strand):
        """Keeps ``ctx`` and ``reads``; (n, the four arrays' pointers) for the kind's ``bsig_plan_create*`` call (a
        pointer keeps its array alive)."""
        self._lib = _lib.load()
        self.ctx, self.reads = ctx, reads
        rid, loc, length, strand = _i32(rid), _i32(loc), _i32(length), _i32(strand)
        n = len(rid)
        if not (len(loc) == len(length) == len(strand) == n):
            raise ValueError("range arrays differ in length")
        self.n_ranges = n
        return n, [_ptr(a) for a in (rid, loc, length, strand)]

    def stats(self):
        s = _lib.PlanStats()
        _lib.check(self._lib.bsig_plan_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bsig_plan_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


class Plan(_PlanBase):
    """Ranges + call parameters resident in HBM; run it any number of times.  ``frag_len`` (a coverage mode only, 1 ..
    2**24; 0: off): every read covers exactly that many bases from its 5' end in its own direction
    (bsig_plan_create_resized) -- an ordinary plan in every other respect."""

    def __init__(self, ctx, reads, rid, loc, length, strand, params, frag_len=0):
        n, ptrs = self._ranges(ctx, reads, rid, loc, length, strand)
        h = C.c_void_p()
        if frag_len:
            _lib.check(self._lib.bsig_plan_create_resized(ctx._h, reads._h, n, *ptrs, C.byref(params), int(frag_len), C.byref(h)))
        else:
            _lib.check(self._lib.bsig_plan_create(ctx._h, reads._h, n, *ptrs, C.byref(params), C.byref(h)))
        self._h = h
        self.cells = int(self._lib.bsig_plan_cells(h))
        self.offsets = np.ctypeslib.as_array(self._lib.bsig_plan_offsets(h), shape=(n + 1,)).copy()

    def run_host(self, out=None, pinned=False):
        """Run and return the flat int32 result in host memory.  ``out``: a reusable int32 array of
        ``cells`` elements (e.g. from ``pinned_empty``); ``pinned=True`` allocates a page-locked one
        (bsig_host_alloc), into which the D2H copy runs at PCIe DMA rate."""
        if out is None:
            out = pinned_empty(self.cells, np.int32) if pinned else np.empty(self.cells, dtype=np.int32)
        elif out.dtype != np.int32 or out.size != self.cells or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous int32 array of plan.cells elements")
        _lib.check(self._lib.bsig_plan_run_host(self._h, _ptr(out)))
        return out

    def run_device(self, out_ptr):
        """Asynchronous launch on the context's stream; ``out_ptr`` is a device address."""
        _lib.check(self._lib.bsig_plan_run(self._h, C.c_void_p(out_ptr)))

    def overflowed(self):
        """Did the last run take a coverage bin past INT32_MAX (binned coverage, heavy tiles)?  For ``run_device``
        callers; ``run_host`` raises by itself.  Synchronises where such a run is possible."""
        f = C.c_int32(0)
        _lib.check(self._lib.bsig_plan_overflowed(self._h, C.byref(f)))
        return bool(f.value)

    def runs(self):
        """The run-length encoder of this plan's result layout (bsig_plan_runs_create): ``n_ranges`` segments, or
        ``2 * n_ranges`` (segment ``2 * i + antisense``) with strands; ``encode`` what ``run_device`` wrote.  Not for a
        bamCount plan."""
        h = C.c_void_p()
        _lib.check(self._lib.bsig_plan_runs_create(self._h, C.byref(h)))
        return RunEncoder._adopt(self.ctx, h)

    def views(self):
        """The views encoder of this plan's result layout (bsig_plan_views_create): the segments of ``runs()``;
        ``encode`` what ``run_device`` wrote, at any thresholds.  Not for a bamCount plan."""
        h = C.c_void_p()
        _lib.check(self._lib.bsig_plan_views_create(self._h, C.byref(h)))
        return ViewEncoder._adopt(self.ctx, h)


class _ReducedPlan(_PlanBase):
    """A plan that reduces all its ranges to ``cells`` int64 (bsig_plan_create_<_KIND>, bsig_plan_run_<_KIND>[_host])."""

    _KIND = None

    def _create(self, ctx, reads, rid, loc, length, strand, params, *extra, variant=""):
        """``extra``: the kind's own int32 arguments, between the parameters and the handle; ``variant``: a suffix of the
        kind's create call (``"_resized"``)."""
        n, ptrs = self._ranges(ctx, reads, rid, loc, length, strand)
        h = C.c_void_p()
        create = getattr(self._lib, f"bsig_plan_create_{self._KIND}{variant}")
        _lib.check(create(ctx._h, reads._h, n, *ptrs, C.byref(params), *extra, C.byref(h)))
        self._h = h
        self.cells = int(getattr(self._lib, f"bsig_plan_{self._KIND}_cells")(h))

    def run_host(self, out=None):
        """Run and return the int64 result in host memory, laid out as the class says (``out``: a reusable contiguous
        int64 array of ``cells``)."""
        if out is None:
            out = np.empty(self.cells, dtype=np.int64)
        elif out.dtype != np.int64 or out.size != self.cells or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous int64 array of plan.cells elements")
        _lib.check(getattr(self._lib, f"bsig_plan_run_{self._KIND}_host")(self._h, _ptr(out)))
        return out

    def run_device(self, out_ptr):
        """Asynchronous launch on the context's stream; ``out_ptr``: device address of ``cells`` int64."""
        _lib.check(getattr(self._lib, f"bsig_plan_run_{self._KIND}")(self._h, C.c_void_p(out_ptr)))


class SumPlan(_ReducedPlan):
    """Ranges of one width + call parameters resident in HBM, summed over the ranges (bsig_plan_create_sum): each run
    gives the int64 sum of what ``Plan`` returns for the ranges, cell by cell -- ``n_bins`` cells, or ``2 x n_bins``
    (cell ``2 * bin + antisense``) with strands.  ``params.threads`` 64 / 128 / 256: tiles in flight per workgroup.
    ``frag_len`` as for ``Plan`` (bsig_plan_create_sum_resized)."""

    _KIND = "sum"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, frag_len=0):
        if frag_len:
            self._create(ctx, reads, rid, loc, length, strand, params, int(frag_len), variant="_resized")
        else:
            self._create(ctx, reads, rid, loc, length, strand, params)


class XcorrPlan(_ReducedPlan):
    """Ranges + call parameters resident in HBM for the strand cross-correlation (bsig_plan_create_xcorr): each run gives
    ``max_lag + 1 + 5`` int64 -- ``cross[d]``, the sum over ranges and cells of sense[x] * antisense[x + d] of the ranges'
    per-base, strand-split, unshifted ``Plan`` result, then the moments [cells, sum S, sum A, sum S^2, sum A^2].
    ``params``: a per-base profile without shift or midpoint; ``tile_cells`` = body cells of a tile, ``threads`` per
    workgroup.  ``stats()['heavy_tiles']`` counts the tiles that took the 32-bit image."""

    _KIND = "xcorr"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, max_lag):
        self._create(ctx, reads, rid, loc, length, strand, params, int(max_lag))
        self.max_lag = int(max_lag)


class FragPlan(_ReducedPlan):
    """Ranges + call parameters resident in HBM for the fragment-length histogram (bsig_plan_create_frag): each run gives
    ``tlen_filter[1] // len_bin + 1`` int64 -- row r counts the reads that ``Plan``'s bamCount (shift 0, unstranded) counts
    over all ranges with ``|tlen| // len_bin == r``.  ``params``: mode COUNT without shift, with a 2-element
    ``tlen_filter``; ``tile_cells`` = bases of a tile, ``threads`` per workgroup.  ``runs``: the runs of tiles (a
    workgroup each) the plan was cut into."""

    _KIND = "frag"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, len_bin=1):
        self._create(ctx, reads, rid, loc, length, strand, params, int(len_bin))
        self.len_bin = int(len_bin)
        self.runs = int(self._lib.bsig_plan_frag_runs(self._h))


class VplotPlan(_ReducedPlan):
    """Ranges of one width + call parameters resident in HBM for the V-plot (bsig_plan_create_vplot): each run gives
    ``rows x cols`` int64 -- cell (r, j) is the sum over the ranges of cell j of ``Plan``'s bamProfile (the caller's
    binsize, shift 0, unstranded) restricted to ``|tlen| // len_bin == r``; ``rows = tlen_filter[1] // len_bin + 1``,
    ``cols = ceil(width / binsize)``.  ``params``: mode PROFILE without shift or strands, with a 2-element
    ``tlen_filter``; ``tile_cells`` = bases of a tile, ``threads`` per workgroup.  ``form``: 0 the table in LDS, 1 global
    atomics; ``runs``: the runs of tiles (a workgroup each) the plan was cut into."""

    _KIND = "vplot"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, len_bin=1):
        self._create(ctx, reads, rid, loc, length, strand, params, int(len_bin))
        self.len_bin = int(len_bin)
        self.rows = int(self._lib.bsig_plan_vplot_rows(self._h))
        self.cols = int(self._lib.bsig_plan_vplot_cols(self._h))
        self.runs = int(self._lib.bsig_plan_vplot_runs(self._h))
        self.form = int(self._lib.bsig_plan_vplot_form(self._h))

    def run_host(self, out=None):
        """Run and return the ``(rows, cols)`` int64 table (``out``: a reusable contiguous int64 array of ``cells``)."""
        return super().run_host(out).reshape(self.rows, self.cols)


class HistPlan(_ReducedPlan):
    """Ranges + call parameters resident in HBM for the depth histogram (bsig_plan_create_hist): each run gives
    ``max_value + 1 + 2`` int64 -- row r counts the cells of value r that ``Plan`` returns for the ranges under the same
    parameters, the last row those of value >= ``max_value``; then the moments [cells, sum of the cell values].
    ``params``: mode COVERAGE (ss 0), or mode PROFILE with binsize 1 and shift 0 (ss: every (base, strand) a cell);
    ``tile_cells`` = cells of a tile (16 .. 2,048), ``threads`` per workgroup.  ``runs``: the runs of tiles (a workgroup
    each) the plan was cut into.  ``stats()['heavy_tiles']`` counts the tiles that took the 32-bit image."""

    _KIND = "hist"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, max_value):
        self._create(ctx, reads, rid, loc, length, strand, params, int(max_value))
        self.max_value = int(max_value)
        self.runs = int(self._lib.bsig_plan_hist_runs(self._h))


class SummaryPlan(_ReducedPlan):
    """Ranges + call parameters resident in HBM for the per-range summaries (bsig_plan_create_summary): each run gives
    ``(n_ranges, S, 3 + K)`` int64 in the caller's range order -- per (range, row) the sum of the cells that ``Plan``
    returns for the range under the same parameters, their max, the index of the first cell holding it (-1 for a range
    without width), and the cells ``>= thresholds[k]``.  ``params``: as ``HistPlan``'s; S = 2 (sense, antisense) for
    mode PROFILE with ss, else 1.  ``thresholds``: 0 .. 8 whole numbers rising from 1.  ``runs``: the runs of tiles (a
    workgroup each) the plan was cut into.  ``stats()['heavy_tiles']`` counts the tiles that took the 32-bit image."""

    _KIND = "summary"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, thresholds=()):
        thr = np.ascontiguousarray(thresholds, dtype=np.int32).reshape(-1)
        self._create(ctx, reads, rid, loc, length, strand, params, len(thr), _ptr(thr) if len(thr) else None)
        self.thresholds = tuple(int(t) for t in thr)
        self.n_ranges = len(_i32(length))
        self.rows = 2 if params.mode == _lib.MODE_PROFILE and params.ss else 1
        self.runs = int(self._lib.bsig_plan_summary_runs(self._h))

    def run_host(self, out=None):
        """Run and return the ``(n_ranges, S, 3 + K)`` int64 result in host memory (``out``: as the base class's)."""
        return super().run_host(out).reshape(self.n_ranges, self.rows, _lib.SUMMARY_FIXED + len(self.thresholds))


class ScaledPlan(_ReducedPlan):
    """Ranges + call parameters resident in HBM for the scaled regions (bsig_plan_create_scaled): each run gives
    ``(n_ranges, S, n_bins)`` int64 in the caller's range order -- every range cut into ``n_bins`` bins whatever its
    width ``w``: cell ``c`` of the cells that ``Plan`` returns for the range under the same parameters is added to bin
    ``c * n_bins // w``.  ``params``: as ``HistPlan``'s; S = 2 (sense, antisense) for mode PROFILE with ss, else 1.
    ``n_bins``: 1 .. 2,048.  ``runs``: the runs of tiles (a workgroup each) the plan was cut into.  ``segmented``:
    whether the plan took the segmented consumer (bsig_plan_scaled_segmented; the result does not depend on it).
    ``stats()['heavy_tiles']`` counts the tiles that took the 32-bit image."""

    _KIND = "scaled"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, n_bins):
        self._create(ctx, reads, rid, loc, length, strand, params, int(n_bins))
        self.n_bins = int(n_bins)
        self.n_ranges = len(_i32(length))
        self.rows = 2 if params.mode == _lib.MODE_PROFILE and params.ss else 1
        self.runs = int(self._lib.bsig_plan_scaled_runs(self._h))
        self.segmented = bool(self._lib.bsig_plan_scaled_segmented(self._h))

    def run_host(self, out=None):
        """Run and return the ``(n_ranges, S, n_bins)`` int64 result in host memory (``out``: as the base class's)."""
        return super().run_host(out).reshape(self.n_ranges, self.rows, self.n_bins)


class CappedPlan(_ReducedPlan):
    """Ranges + call parameters resident in HBM for the capped signals, keepDup (bsig_plan_create_capped): every per-base,
    per-strand 5'-end cell counts ``min(cell, keep_dup)`` before anything is binned, added or extended.  ``frag_len`` 0:
    ``params`` of mode PROFILE (binsize, ss, shift) or COUNT, and each run gives what ``Plan`` gives for them, capped;
    ``frag_len`` > 0: ``params`` of mode COVERAGE or COVERAGE_EX, and each run gives the coverage of the kept reads resized
    to ``frag_len`` bases, as ``Plan(..., frag_len=)`` lays it out.  No midpoint, no extension, no ``tlen_filter``.  The
    result is ``cells`` int32 at ``offsets`` (bsig_layout's order: the caller's range order).  ``runs``: the runs of
    tiles (a workgroup each) the plan was cut into.  ``stats()['heavy_tiles']`` counts the tiles that took the 32-bit
    image."""

    _KIND = "capped"

    def __init__(self, ctx, reads, rid, loc, length, strand, params, keep_dup, frag_len=0):
        self._create(ctx, reads, rid, loc, length, strand, params, int(keep_dup), int(frag_len))
        self.keep_dup, self.frag_len = int(keep_dup), int(frag_len)
        self.n_ranges = len(_i32(length))
        self.runs = int(self._lib.bsig_plan_capped_runs(self._h))
        off = self._lib.bsig_plan_offsets(self._h)
        self.offsets = np.ctypeslib.as_array(off, shape=(self.n_ranges + 1,)).copy()

    def run_host(self, out=None):
        """Run and return the flat int32 result in host memory (``out``: a reusable contiguous int32 array of ``cells``)."""
        if out is None:
            out = np.empty(self.cells, dtype=np.int32)
        elif out.dtype != np.int32 or out.size != self.cells or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous int32 array of plan.cells elements")
        _lib.check(self._lib.bsig_plan_run_capped_host(self._h, _ptr(out)))
        return out


class RunEncoder:
    """Run-length encoder of int32 device buffers (bsig_runs_*): segment k is the ``length[k]`` cells
    ``src[base[k] + p * stride]``; ``stride`` 1, or 2 for one row of the interleaved ``2 * bin + antisense`` layout.
    ``encode(src_ptr)`` counts, allocates and writes the runs on the device and returns their number; ``fetch()`` copies
    them to the host, ``device_pointers()`` leaves them in HBM.  An object encodes any number of buffers."""

    def __init__(self, ctx, base, length, stride=1):
        self._lib = _lib.load()
        base = np.ascontiguousarray(base, dtype=np.int64)
        length = _i32(length)
        if len(base) != len(length):
            raise ValueError("base and length differ in length")
        h = C.c_void_p()
        _lib.check(self._lib.bsig_runs_create(ctx._h, len(base), _ptr(base), _ptr(length), int(stride), C.byref(h)))
        self.ctx, self._h = ctx, h
        self.n_seg = len(base)
        self.cells = int(self._lib.bsig_runs_cells(h))
        self.n_runs = None

    @classmethod
    def _adopt(cls, ctx, h):
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self.ctx, self._h = ctx, h
        self.n_seg = int(self._lib.bsig_runs_n_seg(h))
        self.cells = int(self._lib.bsig_runs_cells(h))
        self.n_runs = None
        return self

    def encode(self, src_ptr):
        """Encode the int32 device buffer at ``src_ptr`` (synchronises); returns the number of runs."""
        n = C.c_int64(0)
        _lib.check(self._lib.bsig_runs_encode(self._h, C.c_void_p(src_ptr), C.byref(n)))
        self.n_runs = int(n.value)
        return self.n_runs

    def device_pointers(self):
        """(n_runs, seg_off, values, lengths): device addresses of the last encode's result (valid until the next)."""
        n = C.c_int64(0)
        so, va, le = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.bsig_runs_device(self._h, C.byref(n), C.byref(so), C.byref(va), C.byref(le)))
        return int(n.value), so.value, va.value, le.value

    def fetch(self):
        """(seg_off int64[n_seg + 1], values int32[n_runs], lengths int32[n_runs]) of the last encode, in host memory."""
        if self.n_runs is None:
            raise ValueError("nothing has been encoded yet")
        seg_off = np.empty(self.n_seg + 1, dtype=np.int64)
        values = np.empty(self.n_runs, dtype=np.int32)
        lengths = np.empty(self.n_runs, dtype=np.int32)
        _lib.check(self._lib.bsig_runs_fetch(self._h, _ptr(seg_off), _ptr(values), _ptr(lengths)))
        return seg_off, values, lengths

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bsig_runs_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


class ViewEncoder:
    """Views of int32 device buffers (bsig_views_*): the segments are ``RunEncoder``'s.  ``encode(src_ptr, lower, upper)``
    finds the maximal stretches of consecutive cells with ``lower <= v <= upper`` (signed) of every segment on the device
    and returns their number; ``fetch()`` copies them to the host -- ``seg_off`` (segment k owns views ``seg_off[k] ..
    seg_off[k + 1]``), ``start`` and ``width`` in cells of the segment, ``sum`` (int64), ``max`` and ``summit`` (the first
    cell of the segment that holds the max) -- ``device_pointers()`` leaves them in HBM.  An object encodes any number of
    buffers at any thresholds."""

    NAMES = ("seg_off", "start", "width", "sum", "max", "summit")
    DTYPES = (np.int64, np.int32, np.int32, np.int64, np.int32, np.int32)

    def __init__(self, ctx, base, length, stride=1):
        self._lib = _lib.load()
        base = np.ascontiguousarray(base, dtype=np.int64)
        length = _i32(length)
        if len(base) != len(length):
            raise ValueError("base and length differ in length")
        h = C.c_void_p()
        _lib.check(self._lib.bsig_views_create(ctx._h, len(base), _ptr(base), _ptr(length), int(stride), C.byref(h)))
        self.ctx, self._h = ctx, h
        self.n_seg = len(base)
        self.cells = int(self._lib.bsig_views_cells(h))
        self.n_views = None

    @classmethod
    def _adopt(cls, ctx, h):
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self.ctx, self._h = ctx, h
        self.n_seg = int(self._lib.bsig_views_n_seg(h))
        self.cells = int(self._lib.bsig_views_cells(h))
        self.n_views = None
        return self

    def encode(self, src_ptr, lower, upper=2**31 - 1):
        """Find the views of the int32 device buffer at ``src_ptr`` (synchronises); returns their number."""
        n = C.c_int64(0)
        self.n_views = None
        _lib.check(self._lib.bsig_views_encode(self._h, C.c_void_p(src_ptr), int(lower), int(upper), C.byref(n)))
        self.n_views = int(n.value)
        return self.n_views

    def device_pointers(self):
        """(n_views, seg_off, start, width, sum, max, summit): device addresses of the last encode's result (valid until
        the next; the five value addresses are None when there is no view)."""
        n = C.c_int64(0)
        ps = [C.c_void_p() for _ in range(6)]
        _lib.check(self._lib.bsig_views_device(self._h, C.byref(n), *[C.byref(p) for p in ps]))
        return (int(n.value),) + tuple(p.value for p in ps)

    def fetch(self):
        """(seg_off int64[n_seg + 1], start, width int32[n_views], sum int64[n_views], max, summit int32[n_views]) of the
        last encode, in host memory."""
        if self.n_views is None:
            raise ValueError("nothing has been encoded yet")
        out = [np.empty(self.n_seg + 1 if k == 0 else self.n_views, dtype=dt) for k, dt in enumerate(self.DTYPES)]
        _lib.check(self._lib.bsig_views_fetch(self._h, *[_ptr(a) if a.size else None for a in out]))
        return tuple(out)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bsig_views_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


class SegmentMap:
    """Device-side reassembly of sharded results: segment k of a source buffer goes to the destination at
    ``dst_off[which[k]]`` (bsig_segmap_*; the host-side twin is bsig_scatter_segments).  The tables are
    uploaded once; ``run`` is one asynchronous kernel launch on the context's stream."""

    def __init__(self, ctx, src_off, dst_off, which):
        self._lib = _lib.load()
        self.ctx = ctx
        src_off = np.ascontiguousarray(src_off, dtype=np.int64)
        dst_off = np.ascontiguousarray(dst_off, dtype=np.int64)
        which = np.ascontiguousarray(which, dtype=np.int64)
        if len(src_off) != len(which) + 1:
            raise ValueError("src_off must have one more entry than which")
        h = C.c_void_p()
        _lib.check(self._lib.bsig_segmap_create(ctx._h, len(which), _ptr(src_off), len(dst_off) - 1, _ptr(dst_off), _ptr(which),
                                                C.byref(h)))
        self._h = h

    def run(self, src_ptr, dst_ptr):
        _lib.check(self._lib.bsig_segmap_run(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr)))

    def run_narrow(self, msg_ptr, n_cells, cap, dst_ptr):
        """``run`` from a shard that travelled as a narrow message (``narrow_pack``): two bits a cell + exceptions."""
        _lib.check(self._lib.bsig_segmap_run_narrow(self._h, C.c_void_p(msg_ptr), int(n_cells), int(cap), C.c_void_p(dst_ptr)))

    def narrow_overflowed(self):
        """Did any narrow message so far hold more exceptions than its list had room for?  (Synchronises.)"""
        v = C.c_int(0)
        _lib.check(self._lib.bsig_segmap_narrow_overflowed(self._h, C.byref(v)))
        return bool(v.value)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bsig_segmap_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


def narrow_bytes(n_cells, cap):
    """Bytes of the narrow message of a shard of ``n_cells`` cells with room for ``cap`` exceptions (bsig_narrow_bytes)."""
    return int(_lib.load().bsig_narrow_bytes(int(n_cells), int(cap)))


def narrow_pack(ctx, src_ptr, n_cells, msg_ptr, cap):
    """Pack the int32 shard at ``src_ptr`` (device, 16-B aligned) into the narrow message at ``msg_ptr``: asynchronous, on
    the context's stream."""
    _lib.check(_lib.load().bsig_narrow_pack(ctx._h, C.c_void_p(src_ptr), int(n_cells), C.c_void_p(msg_ptr), int(cap)))


def narrow_count(ctx, msg_ptr):
    """Exceptions of the packed shard at ``msg_ptr`` (synchronises): what ``cap`` has to hold."""
    v = C.c_int64(0)
    _lib.check(_lib.load().bsig_narrow_count(ctx._h, C.c_void_p(msg_ptr), C.byref(v)))
    return int(v.value)


def layout(length, binsize, ss):
    """Flat offsets of the result (allocateList's shapes, ref: src/bamsignals.cpp:139-192)."""
    lib = _lib.load()
    length = _i32(length)
    off = np.empty(len(length) + 1, dtype=np.int64)
    lib.bsig_layout(len(length), _ptr(length), int(binsize), int(bool(ss)), _ptr(off))
    return off
