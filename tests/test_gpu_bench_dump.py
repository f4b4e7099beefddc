"""bench.py --dump-outputs DIR: what the headline pass computed in its last timed step, written as .npy files that two builds
can be compared by.  Same arguments = same inputs, so two runs must write the same node lists and sizes and the same logits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--nodes", "200000", "--edges", "3000000", "--call-group", "16", "--groups-per-step", "2", "--no-variants",
           "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_of_the_last_step_are_reproducible(hiplib, tmp_path):
    d1, a = _bench(tmp_path / "a", 3)
    d2, b = _bench(tmp_path / "b", 3)
    for d in (d1, d2):
        assert d["steps"] == 3 and d["timed_call_groups"] == 6 and d["ms_per_step"] > 0
    assert set(a) == {"logits", "logit_rows", "n_id", "sizes"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["logits"].dtype == np.float32 and all(a[k].dtype == np.float64 for k in ("logit_rows", "n_id", "sizes"))
    # one entry per call group of the last step (--groups-per-step 2): 8192 of the 16 x 1024 seed rows, 47 classes, two hops
    assert a["logits"].shape == (2, 8192, 47) and a["sizes"].shape == (2, 2, 2) and a["n_id"].shape == (2, 4096)
    assert np.isfinite(a["logits"]).all() and np.abs(a["logits"]).max() > 0
    assert (a["sizes"] > 0).all() and (a["n_id"] >= 0).all() and (a["n_id"] < 200000).all()
    for k in ("logit_rows", "n_id", "sizes"):
        assert np.array_equal(a[k], b[k]), k
    np.testing.assert_allclose(a["logits"], b["logits"], rtol=1e-5, atol=1e-6)
    # a different number of steps ends on different call groups (the walk's seeds follow the group index)
    _, c = _bench(tmp_path / "c", 4)
    assert not np.array_equal(a["n_id"], c["n_id"])


def test_plain_run_prints_the_headline_alone(hiplib):
    """Without --full the run times the headline and nothing else: the line carries the headline's fields, none of what the
    variants, the per-stage pass or the CPU baseline would add."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--nodes", "200000", "--edges", "3000000", "--call-group", "16", "--groups-per-step", "2"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "sampled-edges/s" and d["higher_is_better"] is True
    assert d["steps"] == 2 and d["timed_call_groups"] == 4 and "ids" in d["dtype"] and "workload" in d["config"]
    for key in ("variants", "roofline", "cpu_baseline", "stage_ms_per_call_group", "edges_per_batch", "placements", "selftest"):
        assert key not in d, key
