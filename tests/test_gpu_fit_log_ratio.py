"""fit_log_ratio_kernel on the GPU (exmc_amd/csrc/exmc_fit_psis.hpp, exmc_hip_fit_log_ratio): lr = log p - log q
and logp of every draw of a batch of fits against the statement in lane mode (tests/fit_psis_statement.py
log_ratio_lane: the oracle model in the lane layout, exo_det_log / exo_det_exp, the layout's sum over the
dimensions), byte for byte. Each built kind in its default layout at 3 fits and at 70 (more than one
wavefront of lane groups, the last one partly filled), both scale kinds, two generated layouts through
their plug-ins, and the hostile operands: a NaN in a draw, a draw at 1e308, a fit with NaN mu."""
import numpy as np
import pytest
import torch

import fit_psis_statement as FS
import gen_checker as GC
import oracle as O
import sv_ncp_checker as SN
from exmc_amd import _lib, codegen as cg, models, sampler

pytestmark = pytest.mark.gpu

S = 5


def _logistic():
    X, y = models.logistic_data(seed=140, n=40, k=20)
    return models.logistic(X, y)


def _radon():
    from test_radon_chunks import _survey_like
    return models.radon(_survey_like())


# name: (spec, oracle model of the spec, the kind's default lanes)
KINDS = {
    "simple": (models.simple, O.model_for, 1),
    "eight_schools": (models.eight_schools, O.model_for, 16),
    "sv": (lambda: models.sv(models.sv_returns()), O.model_for, 64),
    "sv_ncp": (lambda: models.sv_ncp(models.sv_returns()), lambda spec: SN.model(models.sv_returns(), True), 64),
    "logistic": (_logistic, O.model_for, 16),
    "radon": (_radon, O.model_for, 64),
}


@pytest.fixture(scope="module")
def handles(hip):
    made = {}

    def get(name):
        if name not in made:
            if name in KINDS:
                spec = KINDS[name][0]()
                made[name] = (sampler.compile(spec), KINDS[name][1](spec), KINDS[name][2])
            elif name == "gen_simple":          # a one-lane layout
                spec = cg.compile_ir(cg.simple_ir())
                made[name] = (sampler.compile(spec), GC.model(spec.gen, 1), 1)
            else:                               # the 64-lane scan chain of non-centred sv
                r = np.asarray(models.sv_returns())
                spec = cg.compile_ir(cg.sv_ir(r), ncp=True, name="gen_sv_ncp",
                                     default_init=models.sv_ncp(r).default_init, lanes=64, waves_per_simd=2)
                made[name] = (sampler.compile(spec), GC.model(spec.gen, 64), 64)
        return made[name]
    yield get
    for comp, _, _ in made.values():
        comp.close()


def fits(d, n_fits, seed, kind):
    """mu, scale [C][d] and draws [C][S][d] around them, as a fit would leave them"""
    rng = np.random.default_rng(seed)
    mu = 0.1 * rng.normal(size=(n_fits, d))
    ls = -1.0 + 0.3 * rng.normal(size=(n_fits, d))
    draws = mu[:, None, :] + np.exp(ls)[:, None, :] * rng.normal(size=(n_fits, S, d))
    return draws, mu, (ls if kind == FS.LOG_SIGMA else np.exp(ls))


def device(comp, lanes, draws, mu, scale, kind, want_logp=True):
    Cn, Sn, d = draws.shape
    x = torch.from_numpy(np.ascontiguousarray(draws.transpose(1, 2, 0))).cuda()
    m = torch.from_numpy(np.ascontiguousarray(mu.T)).cuda()
    sc = torch.from_numpy(np.ascontiguousarray(scale.T)).cuda()
    lr = torch.full((Sn, Cn), 7.0, dtype=torch.float64, device="cuda")
    lp = torch.full((Sn, Cn), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    comp.check(comp.L.exmc_hip_fit_log_ratio(comp.h, x.data_ptr(), m.data_ptr(), sc.data_ptr(), kind, Sn, d, Cn, lanes,
                                             lr.data_ptr(), lp.data_ptr() if want_logp else None))
    torch.cuda.synchronize()
    return lr.cpu().numpy(), lp.cpu().numpy()


def statement(om, lanes, draws, mu, scale, kind):
    cols = [FS.log_ratio_lane(om, lanes, draws[c], mu[c], scale[c], kind) for c in range(draws.shape[0])]
    return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)


def same(got, want, what):
    """bytes; a NaN carries no payload contract: NaN where the statement has NaN"""
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    assert got[~nan].tobytes() == want[~nan].tobytes(), (what, np.argwhere(got != want)[:5], got[~nan][:4], want[~nan][:4])


def check(comp, om, lanes, n_fits, seed, kind, hostile=False, ask=None):
    """`ask`: the lanes_per_chain handed to the call where it is not `lanes` (0: the kind's default)"""
    draws, mu, scale = fits(om.d, n_fits, seed, kind)
    if hostile:
        draws[1, 2, om.d // 2] = np.nan      # a draw with a NaN entry
        draws[0, 3, 0] = 1e308               # a draw at 1e308
        mu[2, :] = np.nan                    # what a failed Pathfinder path reports
    lr, lp = device(comp, lanes if ask is None else ask, draws, mu, scale, kind)
    wlr, wlp = statement(om, lanes, draws, mu, scale, kind)
    same(lr, wlr, "lr")
    same(lp, wlp, "logp")
    return lr, lp


@pytest.mark.parametrize("n_fits", [3, 70])
@pytest.mark.parametrize("name", list(KINDS))
def test_kinds_default_layout(handles, name, n_fits):
    comp, om, lanes = handles(name)
    assert comp.default_lanes == lanes
    kind = FS.SIGMA if n_fits == 3 else FS.LOG_SIGMA
    lr, lp = check(comp, om, lanes, n_fits, 5, kind, ask=0)
    assert np.isfinite(lr).mean() > 0.5
    if n_fits == 3:     # the other scale kind on the same fits: sigma = exp(log_sigma) rounds once more
        lr2, lp2 = check(comp, om, lanes, n_fits, 5, FS.LOG_SIGMA)
        assert lp2.tobytes() == lp.tobytes()
        np.testing.assert_allclose(lr2[np.isfinite(lr)], lr[np.isfinite(lr)], rtol=1e-9)


@pytest.mark.parametrize("name,n_fits", [("gen_simple", 70), ("gen_sv_ncp", 3)])
def test_generated_layouts_through_their_plugins(handles, name, n_fits):
    comp, om, lanes = handles(name)
    lr, _ = check(comp, om, lanes, n_fits, 9, FS.SIGMA)
    check(comp, om, lanes, n_fits, 9, FS.LOG_SIGMA)
    assert np.isfinite(lr).mean() > 0.5


@pytest.mark.parametrize("kind", [FS.SIGMA, FS.LOG_SIGMA])
@pytest.mark.parametrize("name", ["eight_schools", "sv"])
def test_hostile_operands(handles, name, kind):
    comp, om, lanes = handles(name)
    lr, lp = check(comp, om, lanes, 3, 13, kind, hostile=True)
    assert np.isneginf(lr[2, 1]) and np.isneginf(lr[3, 0]) and np.all(np.isneginf(lr[:, 2]))
    assert np.all(np.isfinite(lp[:, 2]))            # the draws of the failed fit are what they are
    assert np.isfinite(lr[0, 0]) and np.isfinite(lr[4, 1])


def test_logp_is_optional_and_arguments_are_checked(handles):
    comp, om, lanes = handles("eight_schools")
    draws, mu, scale = fits(om.d, 3, 1, FS.SIGMA)
    lr, _ = device(comp, lanes, draws, mu, scale, FS.SIGMA)
    lr2, lp2 = device(comp, lanes, draws, mu, scale, FS.SIGMA, want_logp=False)
    assert lr2.tobytes() == lr.tobytes() and np.all(lp2 == 7.0)
    x = torch.zeros((S, om.d, 3), dtype=torch.float64, device="cuda")
    m = torch.ones((om.d, 3), dtype=torch.float64, device="cuda")
    o = torch.zeros((S, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f = comp.L.exmc_hip_fit_log_ratio
    args = [comp.h, x.data_ptr(), m.data_ptr(), m.data_ptr(), 0, S, om.d, 3, 0, o.data_ptr(), None]
    assert f(*args) == _lib.OK
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (4, 2), (5, 0), (6, om.d + 1), (7, 0), (9, None)):
        a = list(args)
        a[at] = bad
        assert f(*a) == _lib.ERR_BADARG, at
    a = list(args)
    a[8] = 5        # no row of eight_schools has five lanes
    assert f(*a) == _lib.ERR_UNSUPPORTED
