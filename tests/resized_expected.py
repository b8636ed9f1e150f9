"""What bamCoverage gives for single-end reads resized to the fragment (bamCoverage(fragLength=L), Plan(frag_len=L)),
without a line of new oracle code: the resizing is a transform of the read columns -- a forward read (flag & 16 == 0)
becomes [pos, pos + L - 1], a reverse read [end - L + 1, end] -- and the expected result is the project's existing oracle
coverage (oracle/oracle_c.py: coverage_core, plain, binned and stranded as tests/forms_deck.py builds them) on the
transformed columns.  The start of a reverse fragment is clipped at 0: no range holds a base below 0, so the clipped
columns give the same coverage, and they stay columns a BAM could hold.  Flags, mapq and tlen are kept, and the rows are
sorted again by (reference, pos), stably, because a resized reverse read may start in front of its neighbours.

`brute_force` is the per-base loop the transform itself is checked against (tests/test_resized_cpu.py)."""
import numpy as np

COLUMNS = ("pos", "end", "flag", "mapq", "tlen")


def resize_columns(cols, L):
    """A copy of the columns (dict with ref_off, pos, end, flag, mapq, tlen; other keys are carried over) in which every
    read covers exactly L bases from its 5' end in its own direction, re-sorted stably by (reference, pos)."""
    L = int(L)
    assert L >= 1
    pos, end = np.asarray(cols["pos"], np.int64), np.asarray(cols["end"], np.int64)
    rev = (np.asarray(cols["flag"]).astype(np.int64) & 16) != 0
    new_pos = np.where(rev, np.maximum(end - L + 1, 0), pos)
    new_end = np.where(rev, end, pos + L - 1)
    assert new_end.max(initial=0) < 2 ** 31
    ref_off = np.asarray(cols["ref_off"], np.int64)
    rid = np.repeat(np.arange(len(ref_off) - 1), np.diff(ref_off))
    order = np.lexsort((new_pos, rid))                           # (stable: ties keep their order)
    out = dict(cols)
    out["pos"], out["end"] = new_pos[order].astype(np.int32), new_end[order].astype(np.int32)
    for k in ("flag", "mapq", "tlen"):
        out[k] = np.asarray(cols[k])[order]
    return out


def brute_force(cols, rid, lo, hi, L, reverse=None):
    """Per-base coverage of the bases [lo, hi) of reference `rid` by the reads resized to L, one read and one base at a
    time (reverse: None all reads, False the forward ones, True the reverse ones).  Bases below 0 are never covered."""
    out = np.zeros(hi - lo, np.int64)
    for i in range(int(cols["ref_off"][rid]), int(cols["ref_off"][rid + 1])):
        rev = (int(cols["flag"][i]) & 16) != 0
        if reverse is not None and rev != reverse:
            continue
        s, e = (int(cols["end"][i]) - L + 1, int(cols["end"][i])) if rev else (int(cols["pos"][i]), int(cols["pos"][i]) + L - 1)
        for x in range(max(s, lo, 0), min(e, hi - 1) + 1):
            out[x - lo] += 1
    return out


def oracle_reads(cols, mask=None):
    from oracle import oracle_c
    if mask is None:
        return oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    n_ref = len(cols["ref_off"]) - 1
    rid = np.repeat(np.arange(n_ref), np.diff(np.asarray(cols["ref_off"], np.int64)))
    off = np.concatenate([[0], np.cumsum(np.bincount(rid[mask], minlength=n_ref))]).astype(np.int64)
    return oracle_c.OracleReads(off, *(np.asarray(cols[k])[mask] for k in COLUMNS))


def _binned(v, b):
    return np.add.reduceat(v, np.arange(0, len(v), b)) if len(v) else np.zeros(0, np.int64)


def coverage(cols, rg, binsize=1, ss=False, **filters):
    """Oracle coverage of `cols` as they are over the ranges, in a plan's flat layout: (int64 cells, offsets).  Per base
    from the oracle (a '-' range mirrored), summed over bins here; with ss the forward and the reverse reads apart, the
    sense row the reads on the range's strand ('*' = '+'), cell 2 * bin + antisense -- tests/forms_deck.py's construction
    of ("coverage", dict(binsize=..., ss=...)).  filters: the oracle's tlen_filter, mapqual, requiredF, filteredF, tspan."""
    from oracle import oracle_c

    def per_base(mask):
        out, off = oracle_c.coverage_core(oracle_reads(cols, mask), rg, **filters)
        return [out[off[i]:off[i + 1]].astype(np.int64) for i in range(len(off) - 1)]
    if not ss:
        parts = [_binned(v, binsize) for v in per_base(None)]
    else:
        fwd = (np.asarray(cols["flag"]) & 16) == 0
        parts = []
        for i, (f, r) in enumerate(zip(per_base(fwd), per_base(~fwd))):
            sense, anti = (r, f) if rg["strand"][i] < 0 else (f, r)
            parts.append(np.stack([_binned(sense, binsize), _binned(anti, binsize)]).T.reshape(-1))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), off


def expected(cols, rg, L, binsize=1, ss=False, **filters):
    """(flat int32 cells, offsets) of resized coverage: the oracle's coverage of resize_columns(cols, L)"""
    out, off = coverage(resize_columns(cols, L), rg, binsize, ss, **filters)
    assert out.max(initial=0) < 2 ** 31
    out = out.astype(np.int32)
    out.setflags(write=False)
    return out, off
