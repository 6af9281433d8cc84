"""The push-style streaming form of the sampling kernel, nuts_kernel<M, G, LDSL, false, true>, held to the
checker in every layout of exmc_layouts.inc that carries it (kRoleStream): the six hand-written kinds at
their default lanes, and the three generated layouts -- one lane, the 16-lane plate layout, the lane
layouts of codegen_lanes.py. It is an instantiation of its own (its own register allocation, a per-draw
system-scope release in the trace sink), launched by exmc_hip_stream_start only, for the one resident chain
exmc_hip_stream_begin leaves behind.

The reference is ONE cold-start run of the checker's sample/3 (tests/stream_push.py): tuning, all seven
columns of a first run and of a second run on the same resident chain, the divergence count of each run, the
published count, and every row that was read while the launch was in flight.

Every case first asserts ON THE CHECKER'S OUTPUT what it is there for; the seeds were picked with the
checker so that these conditions hold. The eight_schools cases at the end walk the ground of
tests/test_gpu_tree_prefix.py and tests/test_gpu_rng_window.py (tree_prefix, RngRowWindow /
draw_momentum_window, row_seqsum_lanes) with the streaming twin: the states a stream starts from cannot be
given, but num_warmup, target_accept, max_tree_depth and the seed steer them."""
import numpy as np
import pytest

import gen_checker as GC
import gen_models as GM
import oracle as O
import stream_push as SP
import sv_ncp_checker as S
from exmc_amd import codegen as cg, models, sampler

pytestmark = pytest.mark.gpu

N_WARMUP, RUNS = 40, (24, 6)
HAND_LANES = dict(eight_schools=16, simple=1, sv=64, sv_ncp=64, logistic=16, radon=64)
GENERATED = ("gen_es_1", "gen_es_16", "gen_sv", "gen_logistic", "gen_walk16")
KINDS = sorted(HAND_LANES) + list(GENERATED)

# kind: {setting: (target_accept, max_tree_depth, seed)}; the first seed of 1..40 that shows, in the
# checker's thirty rows, what the setting is there for (_shows). What the checker showed for each is in
# the comment: the tree sizes, the divergent rows, the leapfrogs of the thirty draws.
SETTINGS = {
    # sizes {7, 15, 23, 31}, 498 leapfrogs | {3, 7}, 206 | 7 divergent rows, sizes {1, 2, 3, 4, 5, 7}, step size 1.675
    "eight_schools": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 1)),
    # {1, 3, 7, 11, 15}, 180 | {1, 3, 5, 7}, 138 | 17 divergent, {1, 2, 3}, step size 0.496
    "simple": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 1)),
    # {47, 63, 79, 127, 191, 255, 511}, 4514 | {7}, 210 | 12 divergent, {2, 3, 4, 5, 7, 11, 15}, step size 0.0437
    "sv": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 8)),
    # sixteen sizes from 6 to 127, 16 divergent rows, 2297 | {7}, 210 | 29 divergent, sixteen sizes from 3 to 63
    "sv_ncp": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 3)),
    # {7, 15}, 298 (seeds 1 and 2: 15 only) | {7}, 210 | 1 divergent, {1, 3}, step size 0.331
    "logistic": dict(shipped=(0.8, 10, 3), capped=(0.8, 3, 1), coarse=(0.3, 10, 1)),
    # {127, 255}, 4834 (seeds 1-3: 255 only) | {7}, 210 | 29 divergent, {2, 3} (seeds 1-29: all thirty rows diverge)
    "radon": dict(shipped=(0.8, 10, 4), capped=(0.8, 3, 1), coarse=(0.3, 10, 30)),
    # the generated eight_schools, one lane and the plate layout: as the hand-written kind
    "gen_es_1": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 1)),
    "gen_es_16": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 1)),
    # {127, 255, 511}, 9058 | {7}, 210 | 6 divergent, {2, 3, 5, 7, 10}, step size 0.0546
    "gen_sv": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 8)),
    # as the hand-written kind: {7, 15}, 298 | {7}, 210 | 1 divergent, {1, 3}
    "gen_logistic": dict(shipped=(0.8, 10, 3), capped=(0.8, 3, 1), coarse=(0.3, 10, 1)),
    # {7, 15, 23, 31, 47, 63, 79}, 962 | {7}, 210 | 13 divergent, {2, 3, 5, 6, 7, 10, 11}, step size 0.309
    "gen_walk16": dict(shipped=(0.8, 10, 1), capped=(0.8, 3, 1), coarse=(0.3, 10, 1)),
}

_specs, _layouts = {}, {}


def _spec(kind):
    """(ModelSpec, lanes of the sampling layout the stream runs in); one plug-in build per generated model"""
    key = "gen_es" if kind.startswith("gen_es") else kind
    if key not in _specs:
        if kind in ("sv", "sv_ncp"):
            _specs[key] = getattr(models, kind)(models.sv_returns())
        elif kind in HAND_LANES:
            _specs[key] = getattr(models, kind)()
        elif key == "gen_es":
            init = {n: 0.0 for n in ["mu"] + ["theta_%d" % j for j in range(8)]}
            init["tau"] = 1.0
            _specs[key] = cg.compile_ir(GM.eight_schools_ir(), name="gen_eight_schools", default_init=init)
        elif kind == "gen_walk16":      # as tests/test_gpu_codegen_lanes.py _compiled builds them
            _specs[key] = cg.compile_ir(GM.walk_ir(), name="walk16", default_init=GM.WALK_INIT, lanes=16)
        else:
            which = kind[len("gen_"):]
            ir, ncp, hand, lanes = GM.baseline_pair(which)
            _specs[key] = cg.compile_ir(ir, ncp=ncp, name="gen_" + which, default_init=hand.default_init, lanes=lanes)
    spec = _specs[key]
    if kind in HAND_LANES:
        return spec, HAND_LANES[kind]
    return spec, {"gen_es_1": 1, "gen_es_16": 16}.get(kind, spec.gen.lanes)


def _checker(kind):
    """(the checker's model of the layout, the kind's default start, lanes): no device needed"""
    spec, lanes = _spec(kind)
    if kind == "sv_ncp":
        om = S.model(np.asarray(models.sv_returns()))     # (O.model_for of the spec is not its statement)
    elif kind in HAND_LANES:
        om = O.model_for(spec)
    else:
        om = GC.model(spec.gen, lanes)
    return om, np.ascontiguousarray(spec.to_unconstrained(spec.default_init)), lanes


def _layout(kind):
    """(handle, checker model, start, lanes): one compiled model per layout for all its settings"""
    if kind not in _layouts:
        spec, lanes = _spec(kind)
        comp = sampler.compile(spec)
        if kind in HAND_LANES:
            assert comp.default_lanes == lanes
        _layouts[kind] = (comp,) + _checker(kind)
    return _layouts[kind]


def _shows(setting, ot):
    n, div = ot["n_steps"], ot["divergent"]
    if setting == "shipped":
        return len(set(n.tolist())) >= 2
    if setting == "capped":
        return bool((n <= 7).all() and (n == 7).any())
    assert setting == "coarse"
    return bool(0 < int(div.sum()) < div.size)


@pytest.mark.parametrize("setting", ["shipped", "capped", "coarse"])
@pytest.mark.parametrize("kind", KINDS)
def test_stream_equals_checker(kind, setting, hip):
    comp, om, q0, lanes = _layout(kind)
    target, depth, seed = SETTINGS[kind][setting]
    if setting == "coarse":
        assert target <= 0.3 and depth == 10
    else:
        assert (target, depth) == ((0.8, 10) if setting == "shipped" else (0.8, 3))
    ot, ost, _ = SP.reference(om, q0, sum(RUNS), N_WARMUP, depth, target, seed, lanes)
    assert _shows(setting, ot), (sorted(set(ot["n_steps"].tolist())), int(ot["divergent"].sum()))
    got = SP.run(comp, q0, RUNS, N_WARMUP, depth, target, seed, lanes)
    SP.assert_equals_checker(got, ot, ost)


# ---- the eight_schools twin (one chain, 16 lanes, default start) on the ground of tree_prefix and the
# generator window. x[i] = the words the ten normals of momentum i took beyond one each, from the checker's
# generator states alone (SP.extra_words). A momentum with x > 0 has a long-way draw; a call's first momentum
# has no window, every other reads the window the transition before it built: shifts up to LAST_SHIFT are in
# it, beyond it the stepping loop is entered mid-way. ----
WINDOW = 14                    # EXMC_RNG_WINDOW
LAST_SHIFT = WINDOW - 12


def _es_reference(num_warmup, target, depth, seed, n):
    comp, om, q0, lanes = _layout("eight_schools")
    ot, ost, states = SP.reference(om, q0, n, num_warmup, depth, target, seed, lanes)
    return comp, q0, lanes, ot, ost, SP.extra_words(states, om.d)


def _sizes(ot, divergent=None):
    n = ot["n_steps"] if divergent is None else ot["n_steps"][ot["divergent"] == divergent]
    return set(n.tolist())


def _through_the_twin(comp, q0, lanes, ot, ost, runs, num_warmup, target, depth, seed):
    got = SP.run(comp, q0, runs, num_warmup, depth, target, seed, lanes)
    SP.assert_equals_checker(got, ot, ost)


def test_es_divergence_at_every_leaf_of_the_prefix(hip):
    """A step size of 2.084: trees that end in a divergence at each of the seven leaves of tree_prefix and
    nowhere else, short trees followed by a momentum with a long-way draw (the window does not depend on how
    many of its uniforms the tree took), momenta at the window's last shift and past it."""
    cfg = (120, 0.2, 10, 7)
    comp, q0, lanes, ot, ost, x = _es_reference(*cfg, 200)
    assert round(ost.step_size, 3) == 2.084
    assert _sizes(ot, 1) == {1, 2, 3, 4, 5, 6, 7} and _sizes(ot) == {1, 2, 3, 4, 5, 6, 7}
    assert int(ot["divergent"].sum()) == 47
    assert int(((ot["n_steps"][:-1] <= 5) & (x[1:] > 0)).sum()) == 31
    assert int((x[1:] == LAST_SHIFT).sum()) == 12 and int((x[1:] > LAST_SHIFT).sum()) == 2
    _through_the_twin(comp, q0, lanes, ot, ost, (160, 40), *cfg)


def test_es_divergences_in_the_prefix_and_hand_over_past_it(hip):
    """Diverged trees inside the prefix and one of 15 leapfrogs, trees of 11 and 15 that the prefix hands
    over to the general loop."""
    cfg = (60, 0.1, 10, 12)
    comp, q0, lanes, ot, ost, x = _es_reference(*cfg, 200)
    assert _sizes(ot, 1) == {1, 2, 3, 4, 5, 6, 15}
    assert _sizes(ot) == {1, 2, 3, 4, 5, 6, 7, 11, 15}
    assert int((x[1:] > LAST_SHIFT).sum()) == 3 and int((x[1:] == LAST_SHIFT).sum()) == 16
    _through_the_twin(comp, q0, lanes, ot, ost, (160, 40), *cfg)


def test_es_no_warmup(hip):
    """num_warmup = 0: the step size is the search's own value, 2.0, and the mass is the identity. The run's
    very first momentum goes the long way (four further words) where no window exists yet."""
    cfg = (0, 0.8, 10, 12)
    comp, q0, lanes, ot, ost, x = _es_reference(*cfg, 200)
    assert ost.step_size == 2.0 and np.array_equal(np.array(ost.inv_mass[:10]), np.ones(10))
    assert _sizes(ot, 1) == {1, 2, 3, 4, 5, 6, 7}
    assert x[0] == 4
    assert int((x[1:] > LAST_SHIFT).sum()) == 4 and int((x[1:] == LAST_SHIFT).sum()) == 15
    _through_the_twin(comp, q0, lanes, ot, ost, (160, 40), *cfg)


def test_es_window_overflow_at_the_shipped_step_size(hip):
    """400 draws under the adapted step size (0.46): of the momenta drawn from a window, 55 stand at shift 1
    or 2, 27 of them at the last shift, and 5 run past it; the run's first momentum has a long-way draw."""
    cfg = (120, 0.8, 10, 7)
    comp, q0, lanes, ot, ost, x = _es_reference(*cfg, 400)
    assert _sizes(ot) == {1, 3, 7, 11, 15, 23} and int(ot["divergent"].sum()) == 0
    assert x[0] == 1
    assert int(((x[1:] >= 1) & (x[1:] <= LAST_SHIFT)).sum()) == 55
    assert int((x[1:] == LAST_SHIFT).sum()) == 27 and int((x[1:] > LAST_SHIFT).sum()) == 5
    _through_the_twin(comp, q0, lanes, ot, ost, (320, 80), *cfg)


@pytest.mark.parametrize("cap, seed, sizes", [(1, 1, {1}), (2, 7, {1, 3}), (3, 1, {3, 7}), (4, 6, {3, 7, 11, 15})])
def test_es_depth_caps(cap, seed, sizes, hip):
    """max_tree_depth 1 to 4: the prefix ends at the cap (1, 3 and 7 leapfrogs), cap 4 leaves it."""
    cfg = (120, 0.8, cap, seed)
    comp, q0, lanes, ot, ost, _ = _es_reference(*cfg, 60)
    assert _sizes(ot) == sizes
    _through_the_twin(comp, q0, lanes, ot, ost, (48, 12), *cfg)


def test_es_no_window_on_entry(hip):
    """stream_start of 1, 1, 1 and 9 draws: every call's first transition has no window. The twelve rows are
    the checker's, with a long-way momentum among the first four and among the rest."""
    cfg = (120, 0.2, 10, 7)
    comp, q0, lanes, ot, ost, x = _es_reference(*cfg, 12)
    assert x.tolist() == [1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 4]
    assert (x[:4] > 0).any() and (x[4:] > 0).any()
    _through_the_twin(comp, q0, lanes, ot, ost, (1, 1, 1, 9), *cfg)
