"""A plain `bench.py` run on the GPU at a small size: it times exactly --steps steps, its line
carries the headline's figures and none of --full's records, it writes nothing but the
--dump-outputs directory, and the dumped positions are the oracle's lower bounds of the
same seeded queries."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_positions(tmp_path):
    n, nq, m = 1 << 16, 4096, 32
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_ENV}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--n", str(n), "--nq", str(nq), "--m", str(m), "--prefix-chars", "8",
                        "--dump-outputs", "out"], env=env, cwd=tmp_path, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "lookups/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    # value = queries per step / the step time (both printed to 4 digits)
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / nq - 1) < 2e-3
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["configs"] == {}
    assert line["verified"] is False and line["detail"] is None
    assert os.listdir(tmp_path) == ["out"] and os.listdir(tmp_path / "out") == ["positions.npy"]
    got = np.load(tmp_path / "out" / "positions.npy")
    assert got.dtype == np.float64 and got.shape == (nq,)
    t = O.random_string(n, bench.SEED)
    off = bench.rank_query_offsets(n, nq, m, 0).astype(np.int64)
    qb = np.concatenate([t[o:o + m] for o in off] + [np.zeros(64, np.uint8)])
    expect, _ = O.search_many(O.padded(t), n, O.build_sa(t), qb, np.arange(nq, dtype=np.uint64) * m,
                              np.full(nq, m, np.uint32))
    assert np.array_equal(got, expect.astype(np.float64))
