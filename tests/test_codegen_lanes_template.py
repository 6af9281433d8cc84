"""The template builder's soundness rule on its own (exmc_amd/codegen_lanes.py _Template.bounds /
make): 0 * x is folded to 0 only when x is proven finite for every unit and every position, because
0 * inf and 0 * NaN are NaN and the generated text must give what the unfolded product gives.
Whole models check the same rule through their values (tests/test_codegen_lanes.py
test_zero_factor_is_folded_only_when_the_other_factor_is_provably_finite)."""
import math

import numpy as np

from exmc_amd import codegen_lanes as cl

N = 5


def _template(**cols):
    """A template over N units with the named raw columns; -> (template, {name: node}) with `zero` (a
    column of zeros: a constant factor that is 0 in every unit) and `v` (a gathered variable)."""
    t = cl._Template(N, [])
    nodes = {}
    for name, vals in dict(cols, zero=[0.0] * N).items():
        t.raw_cols.append(np.asarray(vals, dtype=np.float64))
        nodes[name] = t.T._node("col", -len(t.raw_cols))
    nodes["v"] = t.T._node("gat", 0)
    return t, nodes


def _is_zero(t, node):
    return t.T.ops[node][0] == "lit" and t.T.lit_value(node) == 0.0


def test_a_product_with_an_unbounded_gathered_variable_is_not_folded():
    t, n = _template()
    assert t.bounds(n["v"]) == (-math.inf, math.inf, False)
    for args in ([n["zero"], n["v"]], [n["v"], n["zero"]]):
        out = t.make("mul", args)
        assert t.T.ops[out][0] == "mul" and not _is_zero(t, out)
    # nor with a function of it that can overflow, nor with a constant that is not finite in some unit
    assert not _is_zero(t, t.make("mul", [n["zero"], t.T.exp(n["v"])]))
    t, n = _template(bad=[1.0, 2.0, math.nan, 3.0, 4.0], big=[1.0, math.inf, 0.0, 0.0, 0.0])
    assert t.bounds(n["bad"])[2] is False and t.bounds(n["big"])[2] is False
    assert not _is_zero(t, t.make("mul", [n["zero"], n["bad"]]))
    assert not _is_zero(t, t.make("mul", [n["zero"], n["big"]]))


def test_a_product_with_exp_of_a_bounded_constant_column_is_folded():
    t, n = _template(c=[-3.0, 0.5, 2.0, 7.0, 1.0])
    e = t.T.exp(n["c"])
    lo, hi, ok = t.bounds(e)
    assert ok and lo == float(np.exp(-3.0)) and hi == float(np.exp(7.0))
    assert _is_zero(t, t.make("mul", [n["zero"], e]))
    assert _is_zero(t, t.make("mul", [e, n["zero"]]))
    # and with a value that depends on the position but is bounded whatever it is: exp(min(v, c)) in (0, e^7]
    capped = t.T.exp(t.T.min(n["v"], n["c"]))
    assert t.bounds(capped) == (0.0, float(np.exp(7.0)), True)
    assert _is_zero(t, t.make("mul", [n["zero"], capped]))
    # the exp of a column that reaches the overflow range proves nothing
    t, n = _template(c=[1.0, 2.0, 3.0, 4.0, 705.0])
    assert t.bounds(t.T.exp(t.T.min(n["v"], n["c"])))[2] is False


def test_a_quotient_by_an_interval_that_contains_zero_is_unknown():
    t, n = _template(lo=[-1.0] * N, hi=[0.5, 1.0, 1.0, 1.0, 2.0], plo=[0.25] * N)
    one = t.T.lit(1.0)
    clamp = t.T.min(t.T.max(n["v"], n["lo"]), n["hi"])          # in [-1, 2]: it may be 0
    assert t.bounds(clamp) == (-1.0, 2.0, True)
    assert t.bounds(t.T._node("div", one, clamp)) == (-math.inf, math.inf, False)
    assert not _is_zero(t, t.make("mul", [n["zero"], t.T._node("div", one, clamp)]))
    pos = t.T.min(t.T.max(n["v"], n["plo"]), n["hi"])           # in [0.25, 2]
    assert t.bounds(t.T._node("div", one, pos)) == (0.5, 4.0, True)
    assert _is_zero(t, t.make("mul", [n["zero"], t.T._node("div", one, pos)]))


def test_max_and_min_with_one_unknown_side():
    """fmax / fmin pass the other operand for a NaN: the known side bounds the result from one side, and
    the result is never NaN; the other side stays open, so nothing is folded."""
    t, n = _template(c=[-2.0, 0.0, 1.0, 3.0, 3.0])
    mx, mn = t.T.max(n["v"], n["c"]), t.T.min(n["c"], n["v"])
    assert t.bounds(mx) == (-2.0, math.inf, True)
    assert t.bounds(mn) == (-math.inf, 3.0, True)
    assert not t.finite(mx) and not t.finite(mn)
    assert not _is_zero(t, t.make("mul", [n["zero"], mx]))
    assert not _is_zero(t, t.make("mul", [n["zero"], mn]))
    both = t.T.max(n["v"], t.T._node("gat", 1))
    assert t.bounds(both) == (-math.inf, math.inf, False)


def test_exact_rewrites_of_constant_factors_and_summands():
    t, n = _template(one=[1.0] * N, minus=[-1.0] * N, c=[1.0, 2.0, 3.0, 4.0, 5.0])
    v = n["v"]
    assert t.make("mul", [n["one"], v]) == v and t.make("add", [v, n["zero"]]) == v
    assert t.make("sub", [v, n["zero"]]) == v
    assert t.T.ops[t.make("mul", [v, n["minus"]])] == ("neg", v)
    assert t.T.ops[t.make("sub", [n["zero"], v])] == ("neg", v)
    assert t.cval(n["c"]) is None and t.cval(n["one"]) == 1.0 and t.cval(v) is None
    # a constant that comes out as 0 / 1 / -1 in every unit becomes the literal
    assert _is_zero(t, t.make("mul", [n["zero"], n["c"]]))
    assert t.T.lit_value(t.make("sub", [n["c"], t.make("sub", [n["c"], n["one"]])])) == 1.0


def test_families_and_chains_reject_an_undeclared_attribute():
    for obj in (cl._Family(), cl._Chain()):
        try:
            obj.not_a_field = 1
        except AttributeError:
            continue
        raise AssertionError("%s took an undeclared attribute" % type(obj).__name__)
