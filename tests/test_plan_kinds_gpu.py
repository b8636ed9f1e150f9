"""GPU: every run entry point against every kind of plan (plain, sum, xcorr, frag, hist) -- 11 x 5 calls, each either
accepted (0) or refused with BSIG_ERR_ARG and one exact sentence, written out below.  A plan of a later kind than the
entry's (plain < sum < xcorr < frag < hist) is told which call runs it; one of an earlier kind is told what it is not."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REF_LEN = [2_000_000, 700_017]
KINDS = ("plain", "sum", "xcorr", "frag", "hist")
# (entry point, kind of plan, return code, bsig_last_error() of a refusal)
TABLE = (
    ("bsig_plan_run", "plain", 0, None),
    ("bsig_plan_run", "sum", -1, "a sum plan runs with bsig_plan_run_sum"),
    ("bsig_plan_run", "xcorr", -1, "an xcorr plan runs with bsig_plan_run_xcorr"),
    ("bsig_plan_run", "frag", -1, "a frag plan runs with bsig_plan_run_frag"),
    ("bsig_plan_run", "hist", -1, "a hist plan runs with bsig_plan_run_hist"),
    ("bsig_plan_run_host", "plain", 0, None),
    ("bsig_plan_run_host", "sum", -1, "a sum plan runs with bsig_plan_run_sum_host"),
    ("bsig_plan_run_host", "xcorr", -1, "an xcorr plan runs with bsig_plan_run_xcorr_host"),
    ("bsig_plan_run_host", "frag", -1, "a frag plan runs with bsig_plan_run_frag_host"),
    ("bsig_plan_run_host", "hist", -1, "a hist plan runs with bsig_plan_run_hist_host"),
    ("bsig_plan_run_host_async", "plain", 0, None),
    ("bsig_plan_run_host_async", "sum", -1, "a sum plan runs with bsig_plan_run_sum"),
    ("bsig_plan_run_host_async", "xcorr", -1, "an xcorr plan runs with bsig_plan_run_xcorr"),
    ("bsig_plan_run_host_async", "frag", -1, "a frag plan runs with bsig_plan_run_frag"),
    ("bsig_plan_run_host_async", "hist", -1, "a hist plan runs with bsig_plan_run_hist"),
    ("bsig_plan_run_sum", "plain", -1, "not a sum plan: bsig_plan_run runs it"),
    ("bsig_plan_run_sum", "sum", 0, None),
    ("bsig_plan_run_sum", "xcorr", -1, "an xcorr plan runs with bsig_plan_run_xcorr"),
    ("bsig_plan_run_sum", "frag", -1, "a frag plan runs with bsig_plan_run_frag"),
    ("bsig_plan_run_sum", "hist", -1, "a hist plan runs with bsig_plan_run_hist"),
    ("bsig_plan_run_sum_host", "plain", -1, "not a sum plan: bsig_plan_run_host runs it"),
    ("bsig_plan_run_sum_host", "sum", 0, None),
    ("bsig_plan_run_sum_host", "xcorr", -1, "an xcorr plan runs with bsig_plan_run_xcorr_host"),
    ("bsig_plan_run_sum_host", "frag", -1, "a frag plan runs with bsig_plan_run_frag_host"),
    ("bsig_plan_run_sum_host", "hist", -1, "a hist plan runs with bsig_plan_run_hist_host"),
    ("bsig_plan_run_xcorr", "plain", -1, "not an xcorr plan: bsig_plan_run runs it"),
    ("bsig_plan_run_xcorr", "sum", -1, "not an xcorr plan: bsig_plan_run_sum runs it"),
    ("bsig_plan_run_xcorr", "xcorr", 0, None),
    ("bsig_plan_run_xcorr", "frag", -1, "a frag plan runs with bsig_plan_run_frag"),
    ("bsig_plan_run_xcorr", "hist", -1, "a hist plan runs with bsig_plan_run_hist"),
    ("bsig_plan_run_xcorr_host", "plain", -1, "not an xcorr plan: bsig_plan_run_host runs it"),
    ("bsig_plan_run_xcorr_host", "sum", -1, "not an xcorr plan: bsig_plan_run_sum_host runs it"),
    ("bsig_plan_run_xcorr_host", "xcorr", 0, None),
    ("bsig_plan_run_xcorr_host", "frag", -1, "a frag plan runs with bsig_plan_run_frag_host"),
    ("bsig_plan_run_xcorr_host", "hist", -1, "a hist plan runs with bsig_plan_run_hist_host"),
    ("bsig_plan_run_frag", "plain", -1, "not a frag plan: bsig_plan_run runs it"),
    ("bsig_plan_run_frag", "sum", -1, "not a frag plan: bsig_plan_run_sum runs it"),
    ("bsig_plan_run_frag", "xcorr", -1, "not a frag plan: bsig_plan_run_xcorr runs it"),
    ("bsig_plan_run_frag", "frag", 0, None),
    ("bsig_plan_run_frag", "hist", -1, "a hist plan runs with bsig_plan_run_hist"),
    ("bsig_plan_run_frag_host", "plain", -1, "not a frag plan: bsig_plan_run_host runs it"),
    ("bsig_plan_run_frag_host", "sum", -1, "not a frag plan: bsig_plan_run_sum_host runs it"),
    ("bsig_plan_run_frag_host", "xcorr", -1, "not a frag plan: bsig_plan_run_xcorr_host runs it"),
    ("bsig_plan_run_frag_host", "frag", 0, None),
    ("bsig_plan_run_frag_host", "hist", -1, "a hist plan runs with bsig_plan_run_hist_host"),
    ("bsig_plan_run_hist", "plain", -1, "not a hist plan: bsig_plan_run runs it"),
    ("bsig_plan_run_hist", "sum", -1, "not a hist plan: bsig_plan_run_sum runs it"),
    ("bsig_plan_run_hist", "xcorr", -1, "not a hist plan: bsig_plan_run_xcorr runs it"),
    ("bsig_plan_run_hist", "frag", -1, "not a hist plan: bsig_plan_run_frag runs it"),
    ("bsig_plan_run_hist", "hist", 0, None),
    ("bsig_plan_run_hist_host", "plain", -1, "not a hist plan: bsig_plan_run_host runs it"),
    ("bsig_plan_run_hist_host", "sum", -1, "not a hist plan: bsig_plan_run_sum_host runs it"),
    ("bsig_plan_run_hist_host", "xcorr", -1, "not a hist plan: bsig_plan_run_xcorr_host runs it"),
    ("bsig_plan_run_hist_host", "frag", -1, "not a hist plan: bsig_plan_run_frag_host runs it"),
    ("bsig_plan_run_hist_host", "hist", 0, None),
)
# the entries that write device memory (the others write host memory; the async one only enqueues its copy)
DEVICE = ("bsig_plan_run", "bsig_plan_run_sum", "bsig_plan_run_xcorr", "bsig_plan_run_frag", "bsig_plan_run_hist")


def test_every_run_entry_on_every_kind():
    import torch
    from bamsignals_amd import _lib
    from bamsignals_amd.device import Context, FragPlan, HistPlan, Plan, Reads, SumPlan, XcorrPlan, make_params, pinned_empty
    from bamsignals_amd.synth import synth_reads
    assert len(TABLE) == 55 and len({t[:2] for t in TABLE}) == 55
    assert sum(t[2] == 0 for t in TABLE) == 11 and sum(t[2] == -1 and bool(t[3]) for t in TABLE) == 44
    lib = _lib.load()
    ctx = Context(0)
    cols = synth_reads(400_000, REF_LEN, seed=92, paired=True)
    reads = Reads(ctx, cols["ref_len"], cols["ref_off"], cols["pos"], cols["flag"], cols["mapq"], cols["tlen"],
                  cigar_off=cols["cigar_off"], cigar=cols["cigar"])
    plans = {}
    try:
        a = ([0], [10], [100], [1])
        prof = make_params(_lib.MODE_PROFILE)
        plans["plain"] = Plan(ctx, reads, *a, prof)
        plans["sum"] = SumPlan(ctx, reads, *a, prof)
        plans["xcorr"] = XcorrPlan(ctx, reads, *a, prof, 20)
        plans["frag"] = FragPlan(ctx, reads, *a, make_params(_lib.MODE_COUNT, tlen_filter=(0, 24), binsize=-1, requiredF=66), 1)
        plans["hist"] = HistPlan(ctx, reads, *a, make_params(_lib.MODE_COVERAGE), 24)
        assert [plans[k].cells for k in KINDS] == [100, 100, 26, 25, 27]

        # ---- the 44 refusals: code, words, and nothing written
        b32, b64 = np.zeros(400, np.int32), np.zeros(400, np.int64)
        p32, p64 = b32.ctypes.data_as(C.c_void_p), b64.ctypes.data_as(C.c_void_p)
        for entry, kind, code, says in TABLE:
            if code == 0:
                continue
            plain_entry = entry in ("bsig_plan_run", "bsig_plan_run_host", "bsig_plan_run_host_async")
            assert getattr(lib, entry)(plans[kind]._h, p32 if plain_entry else p64) == code, (entry, kind)
            assert lib.bsig_last_error().decode() == says, (entry, kind)
        assert not b32.any() and not b64.any()

        # ---- the 11 accepted calls; a kind's device call and its host call give one result
        got = {}
        for entry, kind, code, _ in TABLE:
            if code != 0:
                continue
            plan = plans[kind]
            dtype = np.int32 if kind == "plain" else np.int64
            if entry in DEVICE:
                buf = torch.full((max(plan.cells, 4),), -7, dtype=torch.int32 if kind == "plain" else torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                assert getattr(lib, entry)(plan._h, C.c_void_p(buf.data_ptr())) == 0, (entry, lib.bsig_last_error())
                ctx.sync()
                out = buf.cpu().numpy()[:plan.cells]
            else:
                out = pinned_empty(plan.cells, dtype)
                out[:] = -7
                assert getattr(lib, entry)(plan._h, out.ctypes.data_as(C.c_void_p)) == 0, (entry, lib.bsig_last_error())
                ctx.sync()
            got.setdefault(kind, []).append(np.array(out))
        assert [len(got[k]) for k in KINDS] == [3, 2, 2, 2, 2]
        for kind in KINDS:
            for g in got[kind][1:]:
                assert np.array_equal(g, got[kind][0]), kind
            assert (got[kind][0] >= 0).all(), kind
        # (100 bases: the xcorr's and the hist's first moment, the hist's rows)
        assert got["xcorr"][0][21] == 100 and got["hist"][0][25] == 100 and got["hist"][0][:25].sum() == 100
        assert np.array_equal(got["sum"][0], got["plain"][0].astype(np.int64))

        # ---- a kind's queries answer for that kind alone
        queries = {"sum": ("bsig_plan_sum_cells",), "xcorr": ("bsig_plan_xcorr_cells",),
                   "frag": ("bsig_plan_frag_cells", "bsig_plan_frag_runs"), "hist": ("bsig_plan_hist_cells", "bsig_plan_hist_runs")}
        for own, names in queries.items():
            for name in names:
                for kind in KINDS:
                    v = getattr(lib, name)(plans[kind]._h)
                    assert (v != 0) == (kind == own), (name, kind, v)
                assert getattr(lib, name)(None) == 0
        assert lib.bsig_plan_sum_cells(plans["sum"]._h) == 100 and lib.bsig_plan_xcorr_cells(plans["xcorr"]._h) == 26
        assert lib.bsig_plan_frag_cells(plans["frag"]._h) == 25 and lib.bsig_plan_hist_cells(plans["hist"]._h) == 27
        assert lib.bsig_plan_frag_runs(plans["frag"]._h) == 1 and lib.bsig_plan_hist_runs(plans["hist"]._h) == 1
    finally:
        for p in plans.values():
            p.close()
        reads.close()
        ctx.close()
