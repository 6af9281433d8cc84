"""bench.py --dump-outputs (bench.dump_outputs): float64 .npy files of the timed launch's last step, at most
DUMP_BYTES in all, the same seeded sample of the chains on every run where they do not all fit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _arrays(B=5, d=3, C=40):
    g = np.random.default_rng(7)
    return {"draws": torch.from_numpy(g.standard_normal((B, d, C))),
            "n_steps": torch.from_numpy(g.integers(1, 1023, (B, C)).astype(np.int32)),
            "tuning": g.standard_normal((d + 3, C))}


def _read(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_every_chain_when_they_fit(tmp_path):
    a = _arrays()
    bench.dump_outputs(str(tmp_path), a)
    got = _read(str(tmp_path))
    assert sorted(got) == ["chain_index", "draws", "n_steps", "tuning"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["chain_index"], np.arange(40))
    assert np.array_equal(got["draws"], a["draws"].numpy())
    assert np.array_equal(got["n_steps"], a["n_steps"].numpy())
    assert np.array_equal(got["tuning"], a["tuning"])


def test_a_seeded_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    a = _arrays()
    runs = []
    for i in range(2):
        out = tmp_path / str(i)
        bench.dump_outputs(str(out), a, rank=1, world=2, chain_lo=40)
        runs.append(_read(str(out)))
        assert sum(os.path.getsize(out / f) - 128 for f in os.listdir(out)) <= 4000 // 2   # less the .npy headers
    assert sorted(runs[0]) == ["chain_index.rank1", "draws.rank1", "n_steps.rank1", "tuning.rank1"]
    idx = runs[0]["chain_index.rank1"]
    assert 0 < len(idx) < 40 and np.all(np.diff(idx) > 0) and idx[0] >= 40
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    cols = (idx - 40).astype(int)
    assert np.array_equal(runs[0]["draws.rank1"], a["draws"].numpy()[..., cols])
    assert np.array_equal(runs[0]["tuning.rank1"], a["tuning"][..., cols])
