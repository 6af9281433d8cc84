"""bench.py's plain line and --dump-outputs on the device: a plain run carries the headline figure only, --full
adds the rest on the same timed launch, and two runs of the same arguments dump the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--chains-per-gpu", "256"]


def _run(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = r.stdout.decode().strip().splitlines()
    assert len(out) == 1, out
    return json.loads(out[0])


def _read(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_plain_line_and_dumped_outputs(hip, tmp_path):
    a, b, full = tmp_path / "a", tmp_path / "b", tmp_path / "full"
    one = _run(["--dump-outputs", str(a)])
    two = _run(["--dump-outputs", str(b)])
    wide = _run(["--full", "--no-cpu", "--no-multi-step", "--no-sv-leg", "--no-extra-legs", "--dump-outputs", str(full)])
    for ln in (one, two, wide):
        assert ln["metric"] == "leapfrog_steps_per_s" and ln["unit"] == "leapfrog_steps/s"
        assert ln["higher_is_better"] is True and ln["dtype"] == "f64" and ln["steps"] == 3
        assert ln["value"] > 0 and ln["ms_per_step"] > 0
    for k in ("ess_per_s", "rhat_max", "roofline", "models", "cpu_baseline"):
        assert k not in one, k
    assert "ess_per_s" in wide and "roofline" in wide
    for k in ("step_size", "divergent_transitions", "mean_leapfrogs_per_draw"):
        assert one[k] == two[k] == wide[k], k
    da, db, dfull = _read(str(a)), _read(str(b)), _read(str(full))
    assert sorted(da) == ["accept_prob", "chain_index", "divergent", "draws", "n_steps", "tree_depth"]
    assert da["draws"].shape == (50, 10, 256) and da["n_steps"].shape == (50, 256)
    for k in da:
        assert da[k].dtype == np.float64
        assert np.array_equal(da[k], db[k]) and np.array_equal(da[k], dfull[k]), k
    assert np.all(da["n_steps"] >= 1) and np.all(np.isfinite(da["draws"]))


def test_full_line_past_the_bulk_ess_kernel(hip):
    """--full at more draws per chain than the library's bulk-ESS rank kernel holds: the line is made, with the
    bulk figures null and the reason given, and the sv leg that rides along keeps the 1000-draw protocol."""
    import bench
    steps = bench.ESS_BULK_MAX_DRAWS // 50 + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        "1", "--chains-per-gpu", "256", "--full", "--no-cpu", "--no-multi-step", "--no-extra-legs"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    ln = json.loads(r.stdout.decode().strip())
    assert ln["steps"] == steps and ln["config"]["draws_per_chain"] == steps * 50
    assert ln["ess_bulk_min_total"] is None and ln["ess_bulk_per_s"] is None and "ess_bulk_note" in ln
    assert ln["ess_min_total"] > 0 and ln["rhat_routes_agree"] is True
    sv = ln["models"]["sv"]
    assert sv["steps"] == 20 and sv["config"]["draws_per_chain"] == bench.PROTOCOL_DRAWS
    assert sv["ess_bulk_min_total"] > 0 and "ess_bulk_note" not in sv
