"""The reference's integration tests 17, 18 and 19 (test/integration_test.exs:513-607) with their
literals and assertions: Normal-Normal models sampled as generated plug-ins (Sampler.sample/3, 300
warmup + 300 draws, seed 42), the pointwise log-likelihood of each obs formed on the host by
normal.ex's logpdf, reduced on the device by waic_from_pointwise / loo_from_pointwise."""
import numpy as np
import pytest

from exmc_amd import codegen, sampler
from exmc_amd import model_comparison as MC

pytestmark = pytest.mark.gpu

OPTS = dict(num_warmup=300, num_samples=300, seed=42)


def normal_logpdf(x, mu, sigma):
    """normal.ex:15-24 (the f32 log(2 pi) literal)"""
    z = (x - mu) / sigma
    return -0.5 * (z * z + (codegen.LOG_2PI_F32 + 2.0 * np.log(sigma)))


def _sample(ir, name):
    spec = codegen.compile_ir(ir, name=name)
    trace, _ = sampler.sample(sampler.compile(spec), {}, OPTS)
    return np.asarray(trace["mu"], dtype=np.float64)


def _pointwise(mu, obs):
    """ll [S][N][1]: one chain, obs in the reference's key order"""
    return np.stack([normal_logpdf(v, mu, 1.0) for v in obs], axis=1)[:, :, None]


def _ir(prior_mu, prior_sigma, obs):
    ir = codegen.IR()
    ir.rv("mu", "normal", dict(mu=prior_mu, sigma=prior_sigma))
    for name, value in obs:
        ir.rv(name, "normal", dict(mu="mu", sigma=1.0))
        ir.obs(name + "_obs", name, value)
    return ir


def test_17_waic_on_normal_normal(hip):
    mu = _sample(_ir(0.0, 10.0, [("x", 5.0)]), "ic_ref17")
    ll = _pointwise(mu, [5.0])
    assert ll.shape == (300, 1, 1)
    assert np.all(np.isfinite(ll)) and np.all(ll < 0.0)
    r = MC.waic_from_pointwise(ll, names=["x_obs"])
    for k in ("waic", "elpd_waic", "p_waic", "se"):
        assert isinstance(r[k], float)
    assert r["n_obs"] == 1
    assert r["waic"] > 0.0
    assert 0.0 < r["p_waic"] < 5.0


def test_18_better_model_has_lower_waic(hip):
    good = MC.waic_from_pointwise(_pointwise(_sample(_ir(5.0, 1.0, [("x", 5.0)]), "ic_ref18_good"), [5.0]))
    bad = MC.waic_from_pointwise(_pointwise(_sample(_ir(0.0, 1.0, [("x", 5.0)]), "ic_ref18_bad"), [5.0]))
    assert good["elpd_waic"] > bad["elpd_waic"], (good["elpd_waic"], bad["elpd_waic"])
    compared = MC.compare([("good", good), ("bad", bad)])
    assert compared[0]["label"] == "good"


def test_19_loo_over_two_observations(hip):
    mu = _sample(_ir(0.0, 10.0, [("x1", 4.0), ("x2", 5.0)]), "ic_ref19")
    ll = _pointwise(mu, [4.0, 5.0])
    assert ll.shape[1] == 2
    r = MC.loo_from_pointwise(ll, names=["x1_obs", "x2_obs"])
    for k in ("loo", "elpd_loo", "p_loo", "se"):
        assert isinstance(r[k], float)
    assert r["n_obs"] == 2
    assert r["loo"] > 0.0


def test_generated_model_handle_has_no_per_datum_terms(hip):
    """EXMC_MODEL_CUSTOM: every handle entry point answers EXMC_ERR_UNSUPPORTED; waic / loo raise and
    point to *_from_pointwise"""
    import torch
    from exmc_amd import _lib
    comp = sampler.compile(codegen.compile_ir(_ir(0.0, 10.0, [("x", 5.0)]), name="ic_ref17"))
    L = comp.L
    x = torch.zeros((4, comp.d, 2), dtype=torch.float64, device="cuda")
    out = torch.empty((4 * 4 * 2,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert L.exmc_hip_model_n_data(comp.h) < 0
    assert L.exmc_hip_ic_stats(comp.h, x.data_ptr(), 4, comp.d, 2, out.data_ptr()) == _lib.ERR_UNSUPPORTED
    assert L.exmc_hip_pointwise_loglik(comp.h, x.data_ptr(), 4, comp.d, 2, out.data_ptr()) == _lib.ERR_UNSUPPORTED
    h = np.zeros((2, 4, comp.d))
    o = np.zeros(16)
    assert L.exmc_hip_ic_stats_host(comp.h, h.ctypes.data_as(MC._lib.C.POINTER(MC._lib.C.c_double)), 4, comp.d, 2,
                                    o.ctypes.data_as(MC._lib.C.POINTER(MC._lib.C.c_double))) == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.ExmcHipError, match="from_pointwise"):
        MC.waic(comp, x)
    with pytest.raises(_lib.ExmcHipError):
        MC.loo(comp, x)
