"""Pathfinder and ADVI on the GPU in every compiled lane layout that is not the kind's default (the
defaults: test_gpu_pathfinder.py, test_gpu_advi.py): pathfinder_kernel<M, G> and advi_kernel<M, G>
against the statements in lane mode, every output those files compare, bit for bit.

  eight_schools at 1, 2, 4, 8   64, 32, 16, 8 fits per wavefront; group_bcast_c as the identity, as a
                                quad_perm DPP (2, 4), as __shfl (8); ADVI's one-lane window sums
  sv, radon at 32               group_bcast_c as two v_readlane and a select; DPL = 4 with invalid slots
  logistic at 4, 8, 64          at 4 the matrix-core model, the only hand-written kCoop one (pinned by
                                test_fit_layouts_catalogue.py): lane groups without a fit shadow the
                                last fit and leave after the loop; per-wavefront LDS scratch
  generated models              eight_schools_ir in its one-lane layout (d = 10 in one lane), sv_ir
                                compiled at 32 lanes

Every case also runs the statement at another lane count of the model (the kind's default) and asserts
that its result differs, or says why it does not: a case that passed with the wrong row dispatched
would check nothing. The conditions on convergence and pushes are asserted on the statement's own run;
they were read there, not measured on the device. test_fit_layouts_catalogue.py reads the tables."""
import ctypes as C

import numpy as np
import pytest

import gen_checker as GC
import gen_models as GM
import oracle as O
import test_gpu_advi as TA
import test_gpu_pathfinder as TP
from exmc_amd import _lib, codegen as cg, models, sampler
from test_gpu_layouts import LAYOUTS

pytestmark = pytest.mark.gpu

# lanes: (paths, fits). Pathfinder: 64 / G + 1 paths (70 at one lane); ADVI: two wavefronts and more,
# the last of them partial
EIGHT_SCHOOLS = {1: (70, 70), 2: (33, 40), 4: (17, 20), 8: (9, 12)}
# lanes: batch sizes. At 4 lanes 3 fits leave 13 shadow groups in the one wavefront, 17 put one real
# fit and 15 shadows into a second
LOGISTIC = {4: (3, 17), 8: (3,), 64: (2,)}
WIDE = {"sv": 32, "radon": 32}
# the (kind, lanes) pairs both kernels run below
FIT_LAYOUTS = ({("eight_schools", g) for g in EIGHT_SCHOOLS} | {("logistic", g) for g in LOGISTIC} |
               set(WIDE.items()))
GENERATED_LAYOUTS = {("eight_schools_ir", 1), ("sv_ir", 32)}
DEFAULT = {kind: row[1][0] for kind, row in LAYOUTS.items()}


def _differs(a, b, keys):
    return any(not np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _pf(comp, om, lanes, seed, n, other, differs=True, **kw):
    """device = statement at `lanes`; the statement of `other` = (model, lanes) differs from it"""
    got, want = TP._check(comp, om, lanes, seed, n, **kw)
    assert _differs(want, TP._statement(other[0], other[1], seed, n, **kw), TP.KEYS) == differs
    return got, want


def _advi(comp, om, lanes, seed, n, other, differs=True, **kw):
    got, want = TA._check(comp, om, lanes, seed, n, **kw)
    assert _differs(want, TA._statement(other[0], other[1], seed, n, **kw), TA.KEYS) == differs
    return got, want


def _sharp():
    return models.eight_schools([3.0 * v for v in O.EIGHT_SCHOOLS_Y], [0.1 * v for v in O.EIGHT_SCHOOLS_SIGMA])


def _logistic():
    X, y = models.logistic_data(seed=140, n=40, k=20)     # k = 20: what Logistic<4> is built for
    return models.logistic(X, y)


def _radon():
    from test_radon_chunks import _survey_like
    return models.radon(_survey_like())


SPECS = {"eight_schools": models.eight_schools, "es_sharp": _sharp, "sv": lambda: models.sv(models.sv_returns()),
         "radon": _radon, "logistic": _logistic}


@pytest.fixture(scope="module")
def handles(hip):
    made = {}

    def get(name):
        if name not in made:
            spec = SPECS[name]()
            made[name] = (sampler.compile(spec), O.model_for(spec))
        return made[name]
    yield get
    for comp, _ in made.values():
        comp.close()


# ---- eight_schools at 1, 2, 4, 8 ---------------------------------------------------------------------
@pytest.mark.parametrize("data,history_size", [("eight_schools", 6), ("es_sharp", 2)])
@pytest.mark.parametrize("lanes", sorted(EIGHT_SCHOOLS))
def test_eight_schools_pathfinder(handles, lanes, data, history_size):
    """The benchmark data (no pair is pushed) and the sharp data of
    test_eight_schools_history_fills_and_wraps with two pairs of history: the two-loop recursion and
    the truncation in each layout (seeds 11 + 7919 c, c < 5: 4, 2, 4, 6, 5 pushes at each of these lane
    counts). More than one wavefront, the last one partial."""
    comp, om = handles(data)
    n = EIGHT_SCHOOLS[lanes][0]
    assert n * lanes > 64 and (n * lanes) % 64 != 0
    # one lane: 0.0 + v[0] + v[1] + ... , the left-to-right order of the 16-lane kSeqSum group: no bit differs
    _, want = _pf(comp, om, lanes, 11, n, (om, DEFAULT["eight_schools"]), differs=lanes != 1, max_iters=12, num_draws=2,
                  history_size=history_size)
    if data == "es_sharp":
        assert min(want["pushes"]) >= 2 and max(want["pushes"]) > 2
        assert want["pushes"][:5] == [4, 2, 4, 6, 5]
    assert (want["status"] == 0).all()


@pytest.mark.parametrize("kw", [dict(window_size=9), dict(window_size=8), dict(window_size=9, num_mc_samples=2)],
                         ids=["odd_window", "even_window", "two_samples"])
@pytest.mark.parametrize("lanes", sorted(EIGHT_SCHOOLS))
def test_eight_schools_advi_mixed_convergence(handles, lanes, kw):
    """The settings of test_mixed_convergence_in_one_wavefront at 64, 32, 16 and 8 fits per wavefront:
    in the first wavefront 18 of 64, 12 of 32, 6 of 16 and 3 of 8 fits converge before max_iters (9, 5,
    2 and 2 with two samples) and the others run to the end, so converged fits are predicated off next
    to active ones; the odd lane's half sum of the window goes to the whole group."""
    comp, om = handles("eight_schools")
    n, per_wave = EIGHT_SCHOOLS[lanes][1], 64 // lanes
    assert n > per_wave and n % per_wave != 0
    # one lane equals sixteen bit for bit (see above); the window's half sums are sequential in every layout
    _, want = _advi(comp, om, lanes, 11, n, (om, DEFAULT["eight_schools"]), differs=lanes != 1, max_iters=15,
                    num_draws=2, learning_rate=0.05, convergence_tol=0.02, **kw)
    assert 0 < want["converged"][:per_wave].sum() < per_wave
    assert sum(want["non_finite"]) == 0


# ---- sv and radon at 32: two lane groups per wavefront, three fits -------------------------------------
def test_sv_32_lanes_pathfinder(handles):
    comp, om = handles("sv")
    _, want = _pf(comp, om, 32, 5, 3, (om, DEFAULT["sv"]), max_iters=10, num_draws=3)
    assert sum(want["pushes"]) > 0


def test_sv_32_lanes_advi(handles):
    comp, om = handles("sv")
    # against 64 lanes mu and the ELBOs differ (log_sigma and the draws do not at these settings)
    _, want = _advi(comp, om, 32, 5, 3, (om, DEFAULT["sv"]), max_iters=10, num_draws=3, window_size=4,
                    learning_rate=1.0e-3)
    assert sum(want["non_finite"]) == 0


def test_radon_32_lanes_pathfinder(handles):
    comp, om = handles("radon")
    _, want = _pf(comp, om, 32, 4, 3, (om, DEFAULT["radon"]), max_iters=6, num_draws=2)
    assert (want["status"] == 0).all()


def test_radon_32_lanes_advi(handles):
    """at the default rate the density is not finite in the first iterations (mu = -inf compares little);
    at 1e-3 every compared number is finite"""
    comp, om = handles("radon")
    got, want = _advi(comp, om, 32, 4, 3, (om, DEFAULT["radon"]), max_iters=6, num_draws=2, window_size=4,
                      learning_rate=1.0e-3)
    assert sum(want["non_finite"]) == 0
    assert all(np.isfinite(want[k]).all() and np.isfinite(got[k]).all() for k in TA.KEYS)


# ---- logistic at 4 (matrix cores, kCoop), 8 and 64 -----------------------------------------------------
LOGISTIC_CASES = [(g, n) for g in sorted(LOGISTIC) for n in LOGISTIC[g]]


@pytest.mark.parametrize("lanes,n", LOGISTIC_CASES)
def test_logistic_pathfinder(handles, lanes, n):
    """at 4 lanes every lane group of the wavefront takes part in the MFMAs: those without a path repeat
    the last one (chain = C - 1), return after the loop and write nothing"""
    comp, om = handles("logistic")
    _, want = _pf(comp, om, lanes, 2, n, (om, DEFAULT["logistic"]), max_iters=8, num_draws=2)
    assert (want["status"] == 0).all()


@pytest.mark.parametrize("lanes,n", LOGISTIC_CASES)
def test_logistic_advi(handles, lanes, n):
    """at 4 lanes the shadow groups store the last fit's ELBO into the last fit's window: the same
    value to the same word"""
    comp, om = handles("logistic")
    _, want = _advi(comp, om, lanes, 2, n, (om, DEFAULT["logistic"]), max_iters=8, num_draws=2, window_size=4)
    assert sum(want["non_finite"]) == 0


@pytest.mark.parametrize("n,stops", [(3, [14, 14, 11]), (5, [14, 14, 11, 4, 14])])
def test_logistic_4_lanes_advi_shadows_and_convergence(handles, n, stops):
    """Settings found by reading the statement's run (seeds 2 + 7919 c, rate 0.01, tolerance 0.01, window
    4): the fits would stop at 14 (max_iters), 14, 11, 4, 14. With three fits the shadows' owner, fit 2,
    converges at 11 and is predicated off with its 13 shadows while fits 0 and 1 go on; with five the
    owner, fit 4, and its 11 shadows run to the end while fits 2 and 3 have converged."""
    comp, om = handles("logistic")
    _, want = _advi(comp, om, 4, 2, n, (om, DEFAULT["logistic"]), max_iters=14, num_draws=2, window_size=4,
                    learning_rate=0.01, convergence_tol=0.01)
    assert want["num_iters"].tolist() == stops
    assert want["converged"].tolist() == [1 if s < 14 else 0 for s in stops]
    assert sum(want["non_finite"]) == 0


# ---- generated models ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated(hip):
    made = {}

    def get(name):
        if name not in made:
            if name == "eight_schools_ir":      # the plug-in carries the 1- and the 16-lane layout side by side
                spec = cg.compile_ir(cg.eight_schools_ir())
                om, other = GC.model(spec.gen, 1), (GC.model(spec.gen, 16), 16)
            else:                               # as test_gpu_codegen_lanes.py builds gen_sv_32
                ir, ncp, hand, _ = GM.baseline_pair("sv")
                spec = cg.compile_ir(ir, ncp=ncp, name="gen_sv_32", default_init=hand.default_init, lanes=32)
                om, other = GC.model(spec.gen, 32), (GC.model(cg.generate(ir, ncp=ncp, lanes=64), 64), 64)
            made[name] = (sampler.compile(spec), om, other)
        return made[name]
    yield get
    for comp, _, _ in made.values():
        comp.close()


GENERATED_CASES = [("eight_schools_ir", 1, 66), ("sv_ir", 32, 3)]


@pytest.mark.parametrize("name,lanes,n", GENERATED_CASES)
def test_generated_pathfinder(generated, name, lanes, n):
    """Custom<1> with ten dimensions in one lane (two wavefronts, the second partial) and a generated
    32-lane layout"""
    comp, om, other = generated(name)
    assert comp.default_lanes == (16 if lanes == 1 else lanes)     # one lane is not what 0 would resolve to
    # (the generated 16-lane layout adds its plate sums through the butterfly: unlike the hand-written kind,
    # one lane differs from it)
    _pf(comp, om, lanes, 9, n, other, max_iters=6, num_draws=2)


@pytest.mark.parametrize("name,lanes,n", GENERATED_CASES)
def test_generated_advi(generated, name, lanes, n):
    comp, om, other = generated(name)
    _, want = _advi(comp, om, lanes, 9, n, other, max_iters=6, num_draws=2, window_size=4,
                    learning_rate=1.0e-3)
    assert sum(want["non_finite"]) == 0


# ---- a lane count without a row is refused by both entry points ----------------------------------------
@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_lane_counts_without_a_row_are_refused(hip, kind):
    from test_gpu_layouts import Handle, _spec
    hd = Handle(hip, _spec(kind))
    try:
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        elbo, cv = np.zeros(1), np.zeros(1, np.int32)
        for lanes in sorted(set(range(1, 65)) - LAYOUTS[kind][0]):
            rc = hip.exmc_hip_pathfinder_host(hd.h, _lib.PfOpts(1, 1, 6, 8, lanes), 1, 0, dp(), dp(), dp(),
                                              elbo.ctypes.data_as(dp), ip(), ip(), ip())
            assert rc == _lib.ERR_UNSUPPORTED, ("pathfinder", lanes, rc)
            rc = hip.exmc_hip_advi_host(hd.h, _lib.AdviOpts(1, 1, 1, 2, 0.01, 1.0e-4, 8, lanes), 1, 0, dp(), dp(),
                                        dp(), dp(), ip(), cv.ctypes.data_as(ip))
            assert rc == _lib.ERR_UNSUPPORTED, ("advi", lanes, rc)
    finally:
        hd.close()
