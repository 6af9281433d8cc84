"""waic / loo at the BASELINE sizes: the fused call on the sampled device trace, 8 datums spread over N
against the host statement on the downloaded trace; p_waic_i, p_loo_i >= 0 (Jensen) and every value
finite."""
import numpy as np
import pytest
import torch

import ic_checker as IC
from exmc_amd import models, sampler
from exmc_amd import model_comparison as MC

pytestmark = pytest.mark.gpu

CONFIGS = {
    "eight_schools": (models.eight_schools, 4096),
    "sv": (lambda: models.sv(models.sv_returns()), 2048),
    "sv_ncp": (lambda: models.sv_ncp(models.sv_returns()), 2048),
    "logistic": (models.logistic, 8192),
    "radon": (models.radon, 1024),
}


def _reduced(kind, blob, sel):
    """the kind's data blob restricted to the datums `sel` (handle order, increasing)"""
    if kind == models.LOGISTIC:
        N = blob.size // 21
        X, y = blob[:N * 20].reshape(N, 20), blob[N * 20:]
        return np.concatenate([X[sel].reshape(-1), y[sel]])
    if kind == models.RADON:
        N = (blob.size - 171) // 2
        u, cs = blob[:85], blob[85:171]
        fl, y = blob[171:171 + N], blob[171 + N:]
        cs2 = np.array([np.sum(sel < c) for c in cs], dtype=float)
        return np.concatenate([u, cs2, fl[sel], y[sel]])
    return blob


@pytest.mark.parametrize("name", list(CONFIGS))
def test_full_size(name, hip):
    make, Cn = CONFIGS[name]
    spec = make()
    comp = sampler.compile(spec)
    opts = dict(num_warmup=200, num_samples=1000, seed=11)
    _, stats = sampler.sample_chains_compiled(comp, Cn, opts)
    raw = stats[0]["extra"]["raw"]["draws"]                     # [C][S][d]
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(raw).transpose(1, 2, 0))).cuda()
    del raw, stats
    w = MC.waic(comp, x)
    lo = MC.loo(comp, x)
    st = MC.pointwise_stats(comp, x)                            # caller's order
    assert np.isfinite(st).all() and w["n_obs"] == st.shape[1]
    assert (st[1] >= 0).all() and (st[3] >= 0).all()
    assert np.isfinite([w["waic"], w["se"], lo["loo"], lo["se"]]).all()
    N = st.shape[1]
    order = MC._datum_order(comp, N)
    hs = st[:, order]                                           # handle order
    sel = np.unique(np.linspace(0, N - 1, 8).astype(int))
    xh = x.cpu().numpy()
    kind = spec.kind
    if kind in (models.LOGISTIC, models.RADON):
        want = IC.stats_kind(kind, _reduced(kind, spec.data, sel), xh)
    else:
        want = IC.stats_kind(kind, spec.data, xh)[:, sel]
    assert hs[:, sel].tobytes() == want.tobytes(), (hs[:, sel], want)
