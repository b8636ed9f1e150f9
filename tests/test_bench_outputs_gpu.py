"""GPU: a plain bench.py run (no --full) at a small size: it times exactly --steps steps, reports them in its result
line, and --dump-outputs writes what the last step computed -- checked here against the oracle on the same
seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_plain_run_reports_its_steps_and_dumps_the_last_result(tmp_path):
    from bamsignals_amd.synth import synth_ranges
    from oracle import oracle_c
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BAMSIGNALS_DEVICES")}
    steps, warmup, seed = 7, 2, 0xBA51
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C2small", "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=560, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["metric"] == "Mbases profiled/sec (bamProfile binsize=1)" and res["unit"] == "Mbases/s"
    assert res["higher_is_better"] is True and res["dtype"] == "int32" and res["steps"] == steps and res["warmup"] == warmup
    cfg = bench.CONFIGS["C2small"]
    nb = res["config"]["batches"]
    bases = cfg["ranges"] * cfg["width"]
    assert res["ms_per_step"] > 0 and abs(res["value"] - bases / (res["ms_per_step"] * 1e-3) / 1e6) <= 1e-6 * res["value"]
    # a plain run measures nothing else
    assert res["parity_checked"] is None and res["cpu_baseline"] is None and res["end_to_end"] is None and "also" not in res
    assert res["roofline"]["kernel_ms"] > 0

    # the last step ran batch (steps - 1) % nb: its ranges and the reads from the seeds bench.py uses
    b = (steps - 1) % nb
    rg = synth_ranges(cfg["ranges"], cfg["width"], cfg["ref_len"], seed=seed + 1 + 7919 * b)
    order = np.lexsort((rg["loc"], rg["rid"]))
    rg = {k: v[order] for k, v in rg.items()}
    cols = bench.make_reads(cfg["reads"], cfg["ref_len"], seed, cfg["paired"])
    orc = oracle_c.OracleReads(cols["ref_off"], cols["pos"], cols["end"], cols["flag"], cols["mapq"], cols["tlen"])
    want, woff = oracle_c.pileup_core(orc, rg, **cfg["args"])
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("cells_sample", "range_sums", "range_widths")}
    assert sorted(os.listdir(tmp_path / "out")) == ["cells_sample.npy", "range_sums.npy", "range_widths.npy"]
    assert sum(v.nbytes for v in got.values()) <= 64e6 and all(v.dtype == np.float64 for v in got.values())
    ci = bench.dump_pick(want.size, bench.DUMP_CELLS, 0xD0C5)
    assert np.array_equal(got["cells_sample"], want[ci].astype(np.float64))
    cs = np.concatenate([[0], np.cumsum(want, dtype=np.int64)])
    assert np.array_equal(got["range_sums"], (cs[woff[1:]] - cs[woff[:-1]]).astype(np.float64))
    assert np.array_equal(got["range_widths"], np.diff(woff).astype(np.float64))
    assert got["range_sums"].sum() > 0
