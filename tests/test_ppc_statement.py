"""The statement of the posterior predictive checks (tests/ppc_statement.py) on the CPU, on the replicates
tests/predictive_inputs.py already provides: its counts are numpy's own comparisons; its moments agree
with numpy's within rounding; p-values and PIT values are probabilities; a batch sharded at a multiple of
64 chains equals the whole; on data drawn from the model the check is calibrated (no extreme value). (The
BEAM side as source files: tests/test_beam_boundary_sources.py.)"""

import numpy as np
import pytest

import ppc_statement as PPC
import predictive_inputs as PI
import predictive_statement as PS
from exmc_amd import models

U = 2.0 ** -53      # the unit roundoff of float64

_runs = {}


def run(kind):
    if kind not in _runs:
        yrep = PI.expected(kind)[1]
        y = PPC.observed(kind, PI.spec(kind).data)
        _runs[kind] = (yrep, y, PPC.run(yrep, y))
    return _runs[kind]


@pytest.mark.parametrize("kind", PI.KINDS)
def test_observed_values_are_the_kinds_data(kind):
    spec = PI.spec(kind)
    y = PPC.observed(kind, spec.data)
    assert y.shape == (PS.n_data(kind, spec.data),)
    if kind == models.EIGHT_SCHOOLS:
        assert y.tolist() == models.EIGHT_SCHOOLS_Y
    if kind == models.LOGISTIC:
        assert y.tobytes() == models.logistic_data()[1].tobytes()
    if kind == models.RADON:       # the handle's order is the county-sorted one
        assert y.tobytes() == models.radon_data()[3][spec.datum_order].tobytes()


@pytest.mark.parametrize("kind", PI.KINDS)
def test_counts_are_numpys_comparisons(kind):
    yrep, y, r = run(kind)
    S, N, Cn = yrep.shape
    assert r["sums"].shape == (2, N, 2) and r["counts"].shape == (2, N, 2) and r["counts"].dtype == np.int64
    lt, eq = yrep < y[None, :, None], yrep == y[None, :, None]
    for b, (lo, hi) in enumerate([(0, 64), (64, 70)]):
        assert (r["counts"][b, :, 0] == lt[:, :, lo:hi].sum(axis=(0, 2))).all()
        assert (r["counts"][b, :, 1] == eq[:, :, lo:hi].sum(axis=(0, 2))).all()
    assert (r["p_lt"] == lt.sum(axis=(0, 2)) / (S * Cn)).all() and (r["p_eq"] == eq.sum(axis=(0, 2)) / (S * Cn)).all()
    if kind == models.LOGISTIC:    # replicates in {0, 1} and so are the observations: ties are the rule
        assert (r["counts"][:, :, 1].sum(axis=0) > 0).all()
    # the statistics of the replicated data sets against numpy's, and their counts
    assert r["tstat"].shape == (S, 4, Cn) and r["chain_counts"].shape == (4, Cn) and r["chain_counts"].dtype == np.int32
    assert r["tstat"][:, 2].tobytes() == yrep.min(axis=1).tobytes()
    assert r["tstat"][:, 3].tobytes() == yrep.max(axis=1).tobytes()
    assert r["t_obs"][2] == y.min() and r["t_obs"][3] == y.max()
    assert (r["chain_counts"] == (r["tstat"] >= r["t_obs"][None, :, None]).sum(axis=0)).all()
    assert (r["p_value"] == r["chain_counts"].sum(axis=1) / (S * Cn)).all()


@pytest.mark.parametrize("kind", PI.KINDS)
def test_moments_agree_with_numpy_within_rounding(kind):
    """The statement's E is a running sum of n = S C terms e = yrep - y, each rounded once (u) and at most
    D = max |yrep - y| large: |E - exact| <= n u sum |e| <= n^2 u D to first order, so E / n is within
    (n + 1) u D of the exact mean of e, and y + E / n within that plus u |mean|. numpy's pairwise mean is
    within (log2 n + 2) u max |yrep|. Both are below 2 (n + 2) u scale, scale = max |yrep| + |y|.
    E2 sums n terms e^2 <= D^2, each rounded twice: within n (n + 1) u D^2. (E E) / n inherits
    2 |E| n^2 u D / n <= 2 n^2 u D^2 and two more roundings of E^2 / n <= n D^2. The numerator is within
    (3 n^2 + 4 n) u D^2 <= 4 n^2 u D^2 (n >= 4), the quotient by n - 1 within 4 n^2 / (n - 1) u D^2 <=
    4 (n + 2) u D^2. numpy's two-pass variance is within (log2 n + 5) u (2 D)^2 n / (n - 1), far less.
    Both are below 8 (n + 2) u D^2."""
    yrep, y, r = run(kind)
    S, N, Cn = yrep.shape
    n = S * Cn
    per_datum = yrep.transpose(1, 0, 2).reshape(N, n)
    scale = np.abs(per_datum).max(axis=1) + np.abs(y)
    D = np.abs(per_datum - y[:, None]).max(axis=1)
    assert (np.abs(r["mean"] - per_datum.mean(axis=1)) <= 2 * (n + 2) * U * scale).all()
    assert (np.abs(r["var"] - per_datum.var(axis=1, ddof=1)) <= 8 * (n + 2) * U * D * D).all()
    # ... and the statistics of the replicated data sets, with N in the place of n
    m0 = r["m0"]
    Dm = np.abs(yrep - m0).max(axis=1)
    sc = np.abs(yrep).max(axis=1) + abs(m0)
    assert (np.abs(r["tstat"][:, 0] - yrep.mean(axis=1)) <= 2 * (N + 2) * U * sc).all()
    assert (np.abs(r["tstat"][:, 1] - yrep.var(axis=1, ddof=1)) <= 8 * (N + 2) * U * Dm * Dm).all()
    assert abs(r["t_obs"][0] - y.mean()) <= 2 * (N + 2) * U * (np.abs(y).max() + abs(m0))
    assert abs(r["t_obs"][1] - y.var(ddof=1)) <= 8 * (N + 2) * U * np.abs(y - m0).max() ** 2


@pytest.mark.parametrize("kind", PI.KINDS)
def test_p_values_and_pit_are_probabilities(kind):
    _, _, r = run(kind)
    for k in ("p_lt", "p_eq", "pit", "p_value"):
        assert ((r[k] >= 0.0) & (r[k] <= 1.0)).all(), k
    assert (r["pit"] == r["p_lt"] + 0.5 * r["p_eq"]).all()
    assert r["p_value"].shape == (4,)


@pytest.mark.parametrize("kind", PI.KINDS)
def test_two_shards_equal_the_whole(kind):
    yrep, y, whole = run(kind)
    shards = PPC.run_sharded(yrep, y, [0, 64, 70])
    assert set(shards) == set(whole)
    for k, v in whole.items():
        assert np.asarray(shards[k]).tobytes() == np.asarray(v).tobytes(), k


def test_nan_replicates_are_in_neither_count_and_poison_the_sums():
    yrep = np.arange(24.0).reshape(2, 3, 4)
    yrep[1, 2, 3] = np.nan
    r = PPC.run(yrep, np.array([3.0, 100.0, -1.0]))
    assert r["counts"][0].tolist() == [[3, 1], [8, 0], [0, 0]]
    assert np.isnan(r["sums"][0, 2]).all() and np.isfinite(r["sums"][0, :2]).all()
    assert np.isnan(r["tstat"][1, :2, 3]).all() and r["tstat"][1, 2:, 3].tolist() == [15.0, 19.0]     # min, max skip it
    assert r["chain_counts"][:2, 3].tolist() == [(r["tstat"][0, k, 3] >= r["t_obs"][k]) * 1 for k in range(2)]


def test_calibration_on_data_drawn_from_the_model():
    """y drawn from simple's likelihood at the parameters the trace sits at, replicates from the statement
    at 300 draws x 8 chains: no observation is outside its replicates and no statistic is extreme."""
    rng = np.random.default_rng(20240607)
    mu, sigma, N, S, Cn = 2.0, 1.0, 12, 300, 8
    spec = models.simple(y=(mu + sigma * rng.normal(size=N)).tolist())
    x = np.empty((S, 2, Cn))
    x[:, 0, :] = mu + 0.1 * rng.normal(size=(S, Cn))
    x[:, 1, :] = np.log(sigma) + 0.1 * rng.normal(size=(S, Cn))
    yrep = PS.run(models.SIMPLE, spec.data, x, seed=3)[0]
    r = PPC.run(yrep, PPC.observed(models.SIMPLE, spec.data))
    assert ((r["pit"] > 0.0) & (r["pit"] < 1.0)).all(), r["pit"]
    assert ((r["p_value"] > 0.0) & (r["p_value"] < 1.0)).all(), r["p_value"]
