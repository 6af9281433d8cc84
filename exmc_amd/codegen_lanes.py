"""Several dimensions per lane: the lane layout for generated models of any size (d > 16).

The one-lane layout of codegen.py holds the whole position in one lane's registers (d <= 20) and the
plate layout of codegen_vec.py gives every dimension a lane of a 16-lane row (d <= 16). The three
larger BASELINE models are hand-written lane layouts (exmc_models.hpp: SV<64>, Radon<64>,
Logistic<16>): a chain over G lanes, dimension i in slot i / G of lane i % G, the model's repeated
terms spread over the lanes. This module derives that layout from the expression graph of ANY
Builder IR (compiler.ex:176-269 walks the same nodes), so that stochastic volatility (a 100-step
random walk with StudentT observations), the radon model (85 county intercepts, 919 observations)
and the 500 x 20 logistic regression compile from node lists like every smaller model.

  * The log-density is a sum of terms (compiler.ex:394-395). Terms that are themselves sums -- a
    vector observation's elements, the steps of a GaussianRandomWalk, the reduction inside a Custom
    closure -- are split into their summands: the *units*.
  * Units whose expression DAGs are identical up to their leaves form a *family*. Inside a family a
    node that is the SAME graph node in every unit (the graph is hash-consed, so a shared
    hyper-parameter and everything computed from shared hyper-parameters alone is one node) is
    *uniform*: it is evaluated once per leapfrog, outside the family's loop, by every lane alike.
    The remaining nodes are the family's template; its leaves are uniform values, per-unit
    constants (columns of a table folded from the data when the model is generated) and free
    variables that differ from unit to unit (*gathered*: read through a per-unit index).
  * Unit u of a family runs on lane u % G in slot u / G of a counted loop. The position is
    published in an LDS strip of d doubles per chain, so a gathered leaf is one LDS read at a
    per-unit address and a shared variable a broadcast read.
  * Reverse mode per family (codegen._Grad on the template): the adjoints of the uniform inputs are
    summed per lane over its slots and cross the chain group in ONE butterfly together with the
    lane's partial log-density; the adjoints of gathered leaves go to a per-family LDS strip, one
    cell per unit, and the lane that owns a dimension adds the cells that belong to it in a fixed
    order (family, leaf position, unit) read from an index table padded to the widest lane.
  * The uniform part (hyper-priors, everything derived from shared variables, terms that occur
    once) is differentiated as in the one-lane layout, seeded with the reduced adjoints.

What keeps the generated kernels near the hand-written ones (measured there):

  * Families INSIDE the uniform part (_uniform_families): a sum of >= 4 like terms of shared values
    (the quotients of a Lanczos series) is evaluated one term per lane, value and partials reduced
    in a butterfly of their own; the tangent of the sum is the chain rule over its inputs.
  * Batches (_UniformText.stmts): the chain-scalar exp / log / reciprocals of one dependency level are
    evaluated together, argument i on lane i, and broadcast back.
  * Quotients (_Template.quotient): one reciprocal per distinct denominator serves value and
    adjoint; by a constant it is folded into the tables, by a uniform value it leaves the loop
    (_emit_family hoists what does not change from unit to unit).
  * Zero factors (_split_by_zero_factors, _Template.make / bounds): units that differ in WHICH of
    their constant factors are zero form separate families; 0 * x is folded when interval bounds
    prove x finite (each half of a Bernoulli likelihood evaluates one logarithm).
  * Fetching ahead (_loop_head): short table rows and gathered variables of a block of slots are
    loaded before the block's arithmetic (a lone wave per SIMD cannot hide the round trips).
  * One chain on a whole wavefront (EXMC_GEN_G0 / _NG / _XGROUP): for the shared warmup a layout of
    fewer than 64 lanes per chain spreads the slots of every family over the 64 / G lane groups and
    adds the groups' sums in group order.
  * waves_per_simd = 2 (generate): the register cap of two resident waves, with the plug-in's LDS
    sized so that eight workgroups fit a CU (exmc_models.hpp EXMC_GEN_LDS_*).
  * Scan chains (find_chains, 64 lanes only): the non-centred rewrite turns a random walk of chained
    Normals into n_k = n_{k-1} + sigma z_k, which resolves to a serial chain of fused multiply-adds
    that every lane evaluated, with its adjoint. A chain is a maximal path h -> n_1 -> ... -> n_m of
    non-centred nodes with mu(n_k) = n_{k-1} and one common sigma reference, every n_k but the last
    the mu of exactly one non-centred node (a node that is the mu of several, or whose successor has
    another sigma, ends the chain; the next ones start chains of their own with it as head). It is
    evaluated as a wave-wide prefix sum of (h, sigma z_1, ..., sigma z_m), element e in slot e / 64
    of lane e % 64 (EXMC_GEN_SCAN_FWD: exmc_device.hpp wave_scan_fwd), published in an extension of
    the LDS strip, from which the families gather n_k like a position entry; its adjoint is the suffix
    sum A_e of the owner sums of the families' cells (EXMC_GEN_SCAN_BWD: wave_scan_bwd), and
    d/dz_e += sigma A_e (a strip cell the owner of z_e adds), d/dsigma += sum_e z_e A_e (per lane
    over its slots, then the butterfly), d/dh += A_0 seed the uniform part's gradient. A chain is
    scanned when it has at least MIN_SCAN increments and its m + 1 elements fit the DPL slots; and
    the uniform part must not read its walk values (it runs before the forward scans and after the
    backward ones): a chain whose values a head, a sigma or a lone term reads keeps the unrolled
    text, and the others are tried again without it. scan=False (codegen.generate) keeps every walk
    unrolled, the text of earlier versions byte for byte. The generated text carries a host
    statement of both macros (include/exmc_scan.h, the whole chain from the strip alone), which the
    host checker runs where the device runs the scans.

Numeric contract: the lane contract of DESIGN.md section 2 -- per lane left to right over its slots,
then the xor butterfly over the group -- so the sum of a family's terms is NOT the reference's
left-to-right Nx.sum (nor, for models above 32 nodes, the hash order of an Erlang map, which is not
restated: terms are taken in sorted-id order); the difference is rounding of a sum (a few ulp of
the log-density). The host checker (tests/gen_checker.py) runs the same text over G virtual lanes
in that order and the GPU equals it bit for bit; against the hand-written models of the oracle the
generated log-density and gradient agree to 1e-12 relative. A scan chain's walk and adjoint are
summed in the scans' order (in-row Hillis-Steele, the two cross-row stages, the slot carry: the
order of the hand-written sv_ncp kind), not in sequence; every stage selects, and elements past
the walk are 0.0 by a select, never by a multiplication.
"""
import math

import numpy as np

from . import codegen as cg

MIN_FAMILY = 4          # fewer units than this are evaluated by every lane (the uniform part)
MIN_SCAN = 16           # increments of a scan chain: a shorter walk keeps the unrolled text
# doubles of table rows / gathered variables fetched ahead per lane (_loop_head), by resident waves
# per SIMD: a lone wave has 512 registers and nobody to hide its latency, a pair 256 each
PAIR_MIN_COLS = 8      # families of at least this many per-unit columns store them in interleaved pairs (_table_layout)
PREFETCH_DOUBLES = {1: int(__import__("os").environ.get("EXMC_GEN_PREFETCH", "64")), 2: 24}


class _LGraph(cg._Graph):
    """_Graph with the template's leaves: `ext j` (uniform dynamic input j), `uc k` (uniform
    constant k), `col c` (column c of the family's table), `gat p` (gathered variable p) and,
    in the uniform graph, `red j` (reduced sum j after the butterfly)."""

    LEAF_CONST = {"lit": True, "data": True, "q": False, "ext": False, "uc": True, "col": True,
                  "gat": False, "red": False, "wred": False}

    def _node(self, op, *args):
        k = (op,) + args
        i = self.key.get(k)
        if i is None:
            i = len(self.ops)
            self.ops.append(k)
            c = self.LEAF_CONST[op] if op in self.LEAF_CONST else all(self.const[a] for a in args)
            self.const.append(c)
            self.key[k] = i
        return i


_LEAVES = ("lit", "data", "q", "ext", "uc", "col", "gat", "red", "wred", "scn")


def _np_eval(g, nodes, leaf):
    """Values of the const nodes `nodes` (and what they need) with numpy float64 semantics;
    leaf(op) gives the value of a leaf (a scalar or an array over units). exp / log of a constant
    of the data come from numpy here (a rounding-level difference in a constant, like the
    Cholesky of codegen's MvNormal)."""
    memo = {}
    order, seen, stack = [], set(), list(nodes)
    while stack:
        n = stack.pop()
        if n in seen:
            continue
        op = g.ops[n]
        if op[0] in _LEAVES:
            seen.add(n)
            memo[n] = np.float64(float.fromhex(op[1])) if op[0] == "lit" else leaf(op)
            continue
        pend = [a for a in op[1:] if a not in seen]
        if pend:
            stack.append(n)
            stack.extend(pend)
        else:
            seen.add(n)
            order.append(n)
    f64 = lambda x: np.asarray(x, dtype=np.float64)   # noqa: E731
    with np.errstate(all="ignore"):
        for n in order:
            op = g.ops[n]
            a = [f64(memo[x]) for x in op[1:]]
            k = op[0]
            if k == "add": v = a[0] + a[1]
            elif k == "sub": v = a[0] - a[1]
            elif k == "mul": v = a[0] * a[1]
            elif k == "div": v = a[0] / a[1]
            elif k == "neg": v = -a[0]
            elif k == "exp": v = np.exp(a[0])
            elif k == "log": v = np.log(a[0])
            elif k == "log1p": v = np.log1p(a[0])
            elif k == "erf":
                from scipy.special import erf
                v = erf(a[0])
            elif k == "abs": v = np.abs(a[0])
            elif k == "max": v = np.fmax(a[0], a[1])
            elif k == "min": v = np.fmin(a[0], a[1])
            elif k == "sel_gt": v = np.where(a[0] > a[1], a[2], a[3])
            else:
                raise cg.CodegenError("cannot fold %s" % k)
            memo[n] = v
    return memo


def _flatten(g, root, full):
    """The summands of a term: through registered sums (codegen._sum_left) and through `add` nodes
    that lead to one; the result of a Custom closure that holds no registered sum is a reduction
    written by hand (Enum.reduce with Nx.add, validate_posteriordb.exs:279-295) and is split at
    every `add` at its top."""
    worthy = {}

    def is_worthy(n):
        stack = [n]
        while stack:
            x = stack[-1]
            if x in worthy:
                stack.pop()
                continue
            if x in g.sums:
                worthy[x] = True
                stack.pop()
            elif g.ops[x][0] == "add":
                a, b = g.ops[x][1:]
                if a in worthy and b in worthy:
                    worthy[x] = worthy[a] or worthy[b]
                    stack.pop()
                else:
                    stack.extend(c for c in (a, b) if c not in worthy)
            else:
                worthy[x] = False
                stack.pop()
        return worthy[n]

    full = full and not is_worthy(root)
    out, stack = [], [root]
    while stack:
        n = stack.pop()
        if n in g.sums:
            stack.extend(reversed(g.sums[n]))
        elif g.ops[n][0] == "add" and (full or is_worthy(n)):
            stack.extend(reversed(g.ops[n][1:]))
        else:
            out.append(n)
    return out


def _signature(g, root, wild=False):
    """(shape, ids): the unit's DAG in post-order with local numbering; shape is what two units of
    a family share, ids[k] the graph node behind local index k. wild: a literal is a per-unit
    constant like a datum (the coefficients of a series written out term by term)."""
    local, shape, ids = {}, [], []
    stack = [(root, False)]
    is_wild = (lambda a: g.ops[a][0] == "lit") if wild else (lambda a: False)
    while stack:
        n, done = stack.pop()
        if n in local:
            continue
        op = g.ops[n]
        if op[0] in ("lit", "q", "data"):
            local[n] = len(shape)
            shape.append((("wlit",) if wild else ("lit", op[1])) if op[0] == "lit" else (op[0],))
            ids.append(n)
        elif not done:
            stack.append((n, True))
            stack.extend((a, False) for a in reversed(op[1:]) if a not in local and not is_wild(a))
        else:
            args = []
            for a in op[1:]:
                if is_wild(a):            # every occurrence of a literal is a leaf of its own: the graph
                    args.append(len(shape))   # shares equal literals, the terms of a series do not
                    shape.append(("wlit",))
                    ids.append(a)
                else:
                    args.append(local[a])
            local[n] = len(shape)
            shape.append((op[0],) + tuple(args))
            ids.append(n)
    return tuple(shape), ids


class _Family:
    """Units of one shape: a family of the model's terms (plan), or a sum of like terms inside the
    uniform part (_uniform_families: a spread sum). An undeclared attribute is an error."""
    __slots__ = (
        # planning (plan, _uniform_families)
        "shape",       # the units' common DAG (_signature)
        "members",     # positions of the units in the list of units
        "uniform",     # per shape node: the same graph node in every unit
        "ids",         # per unit: the graph node behind each shape node
        "out", "const_part", "inputs",   # spread sums only: the sum's node, its constant terms, the non-constant
                                         # uniform nodes its terms read
        # template (_build_once, _build_template)
        "n", "S", "npad",        # units, slots per lane, units padded to whole slots
        "T", "troot", "tmap",    # the template graph, its root, shape node -> template node
        "raw_cols",              # per-unit data as they stand in the model (leaf `col -1 - c`), one array each
        "gather",                # per gathered leaf: the position index of every unit
        "ext_adj", "gat_adj",    # adjoint nodes: boundary index -> node; per gathered leaf (None: no adjoint)
        "live",                  # template nodes the value and the adjoints need
        "cols", "col_of",        # folded per-unit columns; constant template node -> ("col", c) / ("uc", slot)
        "strip",                 # per gathered leaf: where its adjoint strip starts in the LDS strip (-1: none)
        # uniform part (_uniform_part), spread sums only
        "w0", "w_of",            # slot of w[] for the sum; boundary index -> slot of w[] for its partial
        "cpart",                 # the constant terms' sum
        # table layout (_table_layout)
        "paired",                # columns stored in interleaved pairs
        "cpos",                  # per column: (offset, stride) in doubles
        "ioff",                  # where the gather indices start in the int32 part
    )


def _const_value(g, n):
    """The value of a constant node of the model's graph."""
    return float(_np_eval(g, [n], lambda op: np.float64(g.data[op[1]]))[n])


def _nonzero_const(g, n):
    """A constant node whose value is finite and not zero (so that its reciprocal is a constant too)."""
    v = _const_value(g, n)
    return math.isfinite(v) and v != 0.0 and math.isfinite(1.0 / v)


def _forward_tangents(g, roots, spread=None):
    """{node: {shared variable index: tangent node}} for every non-constant node the roots need.
    Local rules mirror codegen._Grad (max / min pass the tangent on strict inequality only).
    spread: {sum node: [(input node, node holding d sum / d input)]} for the sums evaluated over the
    lanes (_uniform_families): their tangent is the chain rule over their inputs."""
    spread = spread or {}
    def inputs(n):
        args = [e for e, _ in spread[n]] if n in spread else g.ops[n][1:] if g.ops[n][0] not in _LEAVES else ()
        return [a for a in args if not g.const[a]]
    need = cg._reachable([r for r in roots if not g.const[r]], inputs)
    zero = g.lit(0.0)
    tan = {}

    def both(ta, tb, fa, fb, fab):
        out = {}
        for v in set(ta) | set(tb):
            if v in ta and v in tb:
                out[v] = fab(ta[v], tb[v])
            elif v in ta:
                out[v] = fa(ta[v])
            else:
                out[v] = fb(tb[v])
        return out
    for n in sorted(need):
        op = g.ops[n]
        k = op[0]
        if k == "q":
            tan[n] = {op[1]: g.lit(1.0)}
            continue
        if k in _LEAVES:
            tan[n] = {}
            continue
        if n in spread:
            r = {}
            for e, part in spread[n]:
                for v, x in tan.get(e, {}).items():
                    term = g.mul(part, x)
                    r[v] = term if v not in r else g.add(r[v], term)
            tan[n] = r
            continue
        a = op[1:]
        t = [tan.get(x, {}) for x in a]
        ident = lambda x: x   # noqa: E731
        if k == "add":
            r = both(t[0], t[1], ident, ident, g.add)
        elif k == "sub":
            r = both(t[0], t[1], ident, g.neg, g.sub)
        elif k == "neg":
            r = {v: g.neg(x) for v, x in t[0].items()}
        elif k == "mul":
            r = both(t[0], t[1], lambda x: g.mul(x, a[1]), lambda y: g.mul(a[0], y),
                     lambda x, y: g.add(g.mul(x, a[1]), g.mul(a[0], y)))
        elif k == "div":
            if not t[0] and g.const[a[0]] and _nonzero_const(g, a[0]):
                # c / b with a constant numerator: d/db = -y^2 / c, and 1 / c is folded with the data --
                # no second division at run time (a Lanczos series is eight such terms)
                rc = g.recip(a[0])
                r = {v: g.neg(g.mul(g.mul(g.mul(n, n), rc), y)) for v, y in t[1].items()}
            else:
                rb = g.recip(a[1])
                r = both(t[0], t[1], lambda x: g.mul(x, rb), lambda y: g.neg(g.mul(g.mul(n, y), rb)),
                         lambda x, y: g.mul(g.sub(x, g.mul(n, y)), rb))
        elif k == "exp":
            r = {v: g.mul(n, x) for v, x in t[0].items()}
        elif k == "log":
            ra = g.recip(a[0])
            r = {v: g.mul(x, ra) for v, x in t[0].items()}
        elif k == "log1p":
            ra = g.recip(g.add(g.lit(1.0), a[0]))
            r = {v: g.mul(x, ra) for v, x in t[0].items()}
        elif k == "erf":
            d = g.mul(g.lit(2.0 / math.sqrt(math.pi)), g.exp(g.neg(g.mul(a[0], a[0]))))
            r = {v: g.mul(x, d) for v, x in t[0].items()}
        elif k == "abs":
            r = {v: g.sel_gt(a[0], zero, x, g.sel_gt(zero, a[0], g.neg(x), zero)) for v, x in t[0].items()}
        elif k in ("max", "min"):
            first, second = (a[0], a[1]) if k == "max" else (a[1], a[0])
            r = both(t[0], t[1], lambda x: g.sel_gt(first, second, x, zero),
                     lambda y: g.sel_gt(second, first, y, zero),
                     lambda x, y: g.add(g.sel_gt(first, second, x, zero), g.sel_gt(second, first, y, zero)))
        elif k == "sel_gt":
            r = both(t[2], t[3], lambda x: g.sel_gt(a[0], a[1], x, zero), lambda y: g.sel_gt(a[0], a[1], zero, y),
                     lambda x, y: g.sel_gt(a[0], a[1], x, y))
        else:
            raise cg.CodegenError("no tangent rule for %s" % k)
        tan[n] = r
    return tan


def _uniform_families(g, roots):
    """Sums of >= MIN_FAMILY like terms in the non-constant graph under `roots` whose terms read
    shared values and constants only (no variable that differs from term to term); outermost first,
    and none whose inputs depend on another one's result."""
    reach = cg._reachable([r for r in roots if not g.const[r]], lambda n: [a for a in g.ops[n][1:] if not g.const[a]]
                          if g.ops[n][0] not in _LEAVES else ())
    found, absorbed = [], set()
    for V in sorted((n for n in reach if n in g.sums), reverse=True):
        if V in absorbed:
            continue
        terms = g.sums[V]
        dyn = [t for t in terms if not g.const[t]]
        if len(dyn) < MIN_FAMILY or len(set(dyn)) != len(dyn):
            continue
        sigs = [_signature(g, t, wild=True) for t in dyn]
        shape = sigs[0][0]
        if any(sg[0] != shape for sg in sigs[1:]):
            continue
        ids = [sg[1] for sg in sigs]
        uniform = [all(i[k] == ids[0][k] for i in ids) for k in range(len(shape))]
        if uniform[-1]:
            continue
        # the template: from the root down to uniform nodes; a variable of its own per term -> not this kind
        need = cg._reachable([len(shape) - 1], lambda k: shape[k][1:] if not uniform[k] and shape[k][0] not in
                             ("wlit", "data", "q") else ())
        if any(shape[k][0] == "q" and not uniform[k] for k in need):
            continue
        f = _Family()
        f.shape, f.members, f.uniform, f.ids = shape, list(range(len(dyn))), uniform, ids
        f.out, f.const_part = V, [t for t in terms if g.const[t]]
        f.inputs = [ids[0][k] for k in sorted(need) if uniform[k] and not g.const[ids[0][k]]]
        found.append(f)
        # the partial sums between the terms and the terms' own nodes are no longer evaluated
        acc = terms[0]
        for t in terms[1:]:
            acc = g.key.get(("add", acc, t))
            if acc is not None:
                absorbed.add(acc)
        for i in ids:
            absorbed.update(i[k] for k in need if not uniform[k])
    # one level: drop a family whose inputs are computed from another family's sum
    outs = set(f.out for f in found)
    memo = {}

    def depends(n):
        stack = [n]
        while stack:
            x = stack[-1]
            if x in memo:
                stack.pop()
                continue
            if g.const[x] or g.ops[x][0] in _LEAVES:
                memo[x] = False
                stack.pop()
                continue
            if x in outs:
                memo[x] = True
                stack.pop()
                continue
            pend = [a for a in g.ops[x][1:] if a not in memo]
            if pend:
                stack.extend(pend)
            else:
                memo[x] = any(memo[a] for a in g.ops[x][1:])
                stack.pop()
        return memo[n]
    kept = []
    for f in sorted(found, key=lambda f: f.out):
        if any(depends(i) for i in f.inputs):
            outs.discard(f.out)
            memo.clear()
            continue
        kept.append(f)
    return kept


def _split_by_zero_factors(g, shape, members, sigs):
    """Units of one shape, split by WHICH of their constant factors are exactly zero (a 0 / 1 datum y
    in y * log p + (1 - y) * log(1 - p): the units with y = 1 and those with y = 0). In a subfamily
    such a factor is the same constant for every unit, and the template builder folds 0 * (a provably
    finite value) away -- each half of a Bernoulli likelihood then evaluates one logarithm, not two.
    Kept together when a part would have fewer than MIN_FAMILY units or there are more than four."""
    def costly(k, seen):          # a transcendental or a quotient under shape node k
        if k in seen:
            return False
        seen.add(k)
        e = shape[k]
        if e[0] in ("log", "exp", "log1p", "erf", "div"):
            return True
        return e[0] not in ("lit", "q", "data") and any(costly(a, seen) for a in e[1:])
    factors = []
    for k, e in enumerate(shape):
        if e[0] != "mul":
            continue
        for a, b in ((e[1], e[2]), (e[2], e[1])):
            node0 = sigs[members[0]][a]
            if (g.const[node0] and not g.const[sigs[members[0]][b]] and a not in factors
                    and costly(b, set())):         # (0 * a plain variable saves nothing worth a loop)
                factors.append(a)
    if not factors:
        return [members]
    leaf = lambda op: np.float64(g.data[op[1]])   # noqa: E731
    patterns = {}
    for m in members:
        nodes = [sigs[m][k] for k in factors]
        vals = _np_eval(g, nodes, leaf)
        patterns.setdefault(tuple(bool(vals[n] == 0.0) for n in nodes), []).append(m)
    if len(patterns) == 1 or len(patterns) > 4 or min(len(v) for v in patterns.values()) < MIN_FAMILY:
        return [members]
    return [patterns[p] for p in sorted(patterns, key=lambda p: patterns[p][0])]


def plan(g, term_roots, custom_roots, D, G):
    """Units, families and the uniform remainder of the graph `g` whose terms are `term_roots`."""
    units = []
    for t in term_roots:
        units.extend(_flatten(g, t, t in custom_roots))
    by_shape, sigs = {}, {}
    for pos, u in enumerate(units):
        if g.const[u]:
            continue
        shape, ids = _signature(g, u)
        sigs[pos] = ids
        by_shape.setdefault(shape, []).append(pos)
    families, in_family = [], set()
    for shape, all_members in by_shape.items():
        if len(all_members) < MIN_FAMILY:
            continue
        for members in _split_by_zero_factors(g, shape, all_members, sigs):
            first = sigs[members[0]]
            uniform = [all(sigs[m][k] == first[k] for m in members) for k in range(len(shape))]
            if uniform[-1]:
                continue            # the same node n times: n uniform terms
            f = _Family()
            f.shape, f.members, f.uniform = shape, members, uniform
            f.ids = [sigs[m] for m in members]
            families.append(f)
            in_family.update(members)
    families.sort(key=lambda f: f.members[0])
    scalar_units = [units[p] for p in range(len(units)) if p not in in_family]
    return families, scalar_units


class _Chain:
    """A path h -> n_1 -> ... -> n_m of non-centred nodes (find_chains) and, when it is evaluated as
    a scan, its place in the layout. An undeclared attribute is an error."""
    __slots__ = (
        # planning (find_chains)
        "ids", "nodes",            # n_1 .. n_m: the model's ids, the graph nodes
        "head_id", "sigma_id",     # the ids of h and of the scale
        "head", "sigma",           # their graph nodes
        "z",                       # the position index of every increment z_1 .. z_m
        "m",                       # the number of increments
        # strip layout (generate; assigned again on every retry)
        "N",                       # slots per lane: (m + 1 elements) / 64, rounded up
        "w0", "ga0",               # where the walk's values and the cells sigma * A_e start in the LDS strip
        # uniform part (_uniform_part)
        "sz", "a0",                # `scn` leaves: the run-time values sum_e z_e A_e and A_0
        # owner lists (_owner_lists)
        "W", "eoff",               # cells an element adds at most; where the elements' lists start in a lane's list
        # table layout (_table_layout)
        "zoff",                    # where the position indices of z start in the int32 part
    )


def find_chains(g, ncp_info, ncp_nodes):
    """The scan chains of a model: maximal paths h -> n_1 -> ... -> n_m of non-centred nodes
    (n_k = n_{k-1} + sigma z_k after the rewrite) where mu(n_k) = n_{k-1}, all n_k share ONE sigma
    reference, and every n_k but the last is the mu of exactly one non-centred node (its successor).
    A node that is the mu of several non-centred nodes ends its chain, and each of those starts a
    chain of its own whose head is that node; so does a node whose sigma differs from its mu's.
    Only resolved nodes count (a walk's tail that nothing reads is not in the graph). The head h
    (mu of n_1) is any resolved value. -> [_Chain], in the order of their first ids."""
    kids = {}
    for c in sorted(ncp_nodes):
        kids.setdefault(ncp_info[c]["mu"], []).append(c)

    def succ(p):
        ks = kids.get(p, [])
        return ks[0] if (len(ks) == 1 and ncp_info[ks[0]]["sigma"] == ncp_info[p]["sigma"]) else None
    starts = [c for c in sorted(ncp_nodes)
              if not (ncp_info[c]["mu"] in ncp_nodes and succ(ncp_info[c]["mu"]) == c)]
    out = []
    for c0 in starts:
        ids = [c0]
        while succ(ids[-1]) is not None:
            ids.append(succ(ids[-1]))
        ch = _Chain()
        ch.ids, ch.nodes = ids, [ncp_nodes[i] for i in ids]
        ch.head_id, ch.sigma_id = ncp_info[c0]["mu"], ncp_info[c0]["sigma"]
        op = g.ops[ch.nodes[0]]
        ch.head = op[1]
        ch.sigma = g.ops[op[2]][1]
        ch.z = []
        prev, ok = ch.head, True
        for n in ch.nodes:                     # n = add(prev, mul(sigma, q z)), as resolve_ref builds it
            op = g.ops[n]
            m = g.ops[op[2]] if op[0] == "add" else None
            ok = ok and op[1] == prev and m is not None and m[0] == "mul" and m[1] == ch.sigma \
                and g.ops[m[2]][0] == "q"
            if not ok:
                break
            ch.z.append(g.ops[m[2]][1])
            prev = n
        if ok:
            ch.m = len(ids)
            out.append(ch)
    return out


class _SGraph(cg._Graph):
    """The graph of a layout with scan chains: `scn j` is a run-time value of the scans (the
    sigma reduction and A_0 of chain j // 2) that the differentiation does not look into."""
    LEAF_CONST = dict(cg._Graph.LEAF_CONST, scn=False, wred=False)


def _with_walk_leaves(g, leaf_of):
    """A copy of g where each walk node n (leaf_of[n] = its strip index) is a position-like leaf
    `q`: its value is read from the chain's strip like a position entry. Node indices are kept,
    so the terms, the registered sums and every other node stay what they are."""
    h = _SGraph()
    h.ops, h.const, h.key = list(g.ops), list(g.const), dict(g.key)
    h.data, h.f32, h.sums = list(g.data), set(g.f32), {k: list(v) for k, v in g.sums.items()}
    for n, i in leaf_of.items():
        del h.key[h.ops[n]]
        h.ops[n] = ("q", i)
        h.key[h.ops[n]] = n
        h.const[n] = False
    return h


class _WalkRead(Exception):
    """The uniform part reads a walk value of these chains (a head or a scale that is a step of
    another walk, a lone term of a step): they keep the unrolled text."""

    def __init__(self, chains):
        Exception.__init__(self)
        self.chains = chains


def generate(g, term_roots, custom_roots, D, G, waves_per_simd=1, chains=()):
    """-> dict(text, data, lanes, dpl, ...) for the lane layout. waves_per_simd: resident waves per
    SIMD the sampling kernel's register allocation must allow (ModelDefaults::kNutsWavesPerSimd):
    1 leaves the allocator the whole file; 2 caps it at 256 vector registers, which can pay when a
    launch has more wavefronts than the chip has SIMDs (chains x lanes / 64 > 1024) -- it does for
    the hand-written sv and logistic kinds, it does not for their generated forms, whose bodies
    then spill inside the leaf loop (profiles/r3_gen). chains: find_chains of the model; those that
    qualify (module docstring, scan chains) are evaluated as wave-wide scans."""
    if waves_per_simd not in (1, 2):
        raise cg.CodegenError("waves_per_simd must be 1 or 2")
    if G not in (16, 32, 64):
        raise cg.CodegenError("lanes per chain must be 16, 32 or 64")
    DPL = (D + G - 1) // G
    use = [c for c in chains if G == 64 and c.m >= MIN_SCAN and (c.m + 1 + 63) // 64 <= DPL]
    while use:
        base, leaf_of = D + 1, {}
        for c in use:                          # strip: [position][0.0][walks][walk adjoints][...]
            c.N, c.w0 = (c.m + 64) // 64, base
            leaf_of.update((n, c.w0 + 1 + k) for k, n in enumerate(c.nodes))
            base += c.m + 1
        for c in use:
            c.ga0 = base
            base += c.m + 1
        try:
            return _generate(_with_walk_leaves(g, leaf_of), term_roots, custom_roots, D, G, waves_per_simd,
                             use, base)
        except _WalkRead as e:
            use = [c for c in use if c not in e.chains]
    return _generate(g, term_roots, custom_roots, D, G, waves_per_simd, [], D + 1)


def _scan_host_defaults(chains):
    """The scans of the generated text as host C (tests/gen_checker.py runs the lane function lane
    after lane, so no lane sees another's registers): each macro computes the whole chain from the
    LDS strip alone, in the device's association order (include/exmc_scan.h), and writes every
    element. The device defines them first (exmc_models.hpp: wave_scan_fwd / wave_scan_bwd)."""
    return [
        "/* scan chains (codegen_lanes.py): %d; their host statement unless the includer defines the scans */" % len(chains),
        "#ifndef EXMC_GEN_SCAN_FWD",
        '#include "exmc_scan.h"',
        "#define EXMC_GEN_SCAN_FWD(N, v, m, zo, h, sg, wo) do { \\",
        "    double e_[64 * (N)]; \\",
        "    for (int i_ = 0; i_ < 64 * (N); i_++) \\",
        "      e_[i_] = (i_ == 0) ? (h) : ((i_ <= (m)) ? (sg) * EXMC_GEN_SH(EXMC_GEN_IT((zo) + i_)) : 0.0); \\",
        "    exmc_scan_fwd64(e_, (N)); \\",
        "    for (int i_ = 0; i_ <= (m); i_++) EXMC_GEN_SH((wo) + i_) = e_[i_]; \\",
        "    (void)(v); } while (0)",
        "#endif",
        "#ifndef EXMC_GEN_SCAN_BWD",
        "#define EXMC_GEN_SCAN_BWD(N, v, m, zo, sg, we, ww, ga, sz, a0) do { \\",
        "    double e_[64 * (N)], p_[64]; \\",
        "    const int* el_ = (const int*)lt + EXMC_GEN_ELL_OFF; \\",
        "    for (int i_ = 0; i_ < 64 * (N); i_++) { \\",
        "      double acc_ = 0.0; \\",
        "      for (int j_ = 0; j_ < (ww); j_++) \\",
        "        acc_ = acc_ + EXMC_GEN_SH(el_[(i_ & 63) * EXMC_GEN_NELL + (we) + (i_ >> 6) * (ww) + j_]); \\",
        "      e_[i_] = acc_; \\",
        "    } \\",
        "    exmc_scan_bwd64(e_, (N)); \\",
        "    for (int i_ = 1; i_ <= (m); i_++) EXMC_GEN_SH((ga) + i_) = (sg) * e_[i_]; \\",
        "    for (int l_ = 0; l_ < 64; l_++) { \\",
        "      double q_ = 0.0; \\",
        "      for (int k_ = 0; k_ < (N); k_++) { \\",
        "        const int i_ = l_ + 64 * k_; \\",
        "        q_ = (i_ >= 1 && i_ <= (m)) ? q_ + EXMC_GEN_SH(EXMC_GEN_IT((zo) + i_)) * e_[i_] : q_; \\",
        "      } \\",
        "      p_[l_] = q_; \\",
        "    } \\",
        "    (sz) = exmc_allsum64(p_); \\",
        "    (a0) = e_[0]; \\",
        "    (void)(v); } while (0)",
        "#endif",
        "",
    ]


class _Shared:
    """The two numberings that every template and the uniform part share: the uniform constants
    (EXMC_GEN_LT(k)) and the boundary nodes (`ext j`, s[1 + ...]). A number is given at FIRST USE and
    is part of the generated text, so the stages receive this object in the order they run: the
    families' templates, the spread sums' templates, then the uniform part's own constants."""
    __slots__ = ("g", "uc_of", "uc_vals", "boundary", "b_index")

    def __init__(self, g):
        self.g = g
        self.uc_of, self.uc_vals = {}, []       # key -> slot, slot -> value
        self.boundary, self.b_index = [], {}    # distinct uniform dynamic nodes read by templates; node -> index

    def uc_slot(self, key, value):
        if key not in self.uc_of:
            self.uc_of[key] = len(self.uc_vals)
            self.uc_vals.append(float(value))
        return self.uc_of[key]

    def uc_node(self, n):
        """the slot of a constant node of the model's graph"""
        return self.uc_slot(("node", n), _const_value(self.g, n))

    def uc_value(self, v):
        """the slot of a value (equal values share one)"""
        return self.uc_slot(("val", float(v).hex()), v)

    def ext(self, n):
        """the boundary index of a uniform dynamic node"""
        if n not in self.b_index:
            self.b_index[n] = len(self.boundary)
            self.boundary.append(n)
        return self.b_index[n]


class _Template:
    """The graph T of one family's template while it is built, with what decides its rewrites: the
    per-unit values of its constants (raw_cols: the family's raw data columns, leaf `col -1 - c`;
    uc_vals: the uniform constants), interval bounds, the quotient contract. The memo tables live
    as long as the build."""

    def __init__(self, n, uc_vals):
        self.T, self.n = _LGraph(), n
        self.raw_cols, self.uc_vals = [], uc_vals
        self._cval, self._bnd = {}, {}

    def const_leaf(self, op):
        if op[0] == "col":
            return self.raw_cols[-op[1] - 1]
        if op[0] == "uc":
            return np.float64(self.uc_vals[op[1]])
        raise cg.CodegenError("unexpected leaf %r in a constant" % (op,))

    def num_ok(self, node):
        """a constant of the template that is finite and non-zero in every unit, and so is 1 / it"""
        v = np.asarray(_np_eval(self.T, [node], self.const_leaf)[node], dtype=np.float64)
        with np.errstate(all="ignore"):
            return bool(np.all(np.isfinite(v)) and np.all(v != 0.0) and np.all(np.isfinite(1.0 / v)))

    def quotient(self, a, b, shared):
        """a / b of the template. One reciprocal per distinct denominator serves the value and the
        adjoint (the lane layout's own contract, like its fused multiply-adds: a * (1 / b) is within
        an ulp of a / b): by a constant the reciprocal is folded into the tables, by a uniform
        value it leaves the loop. c / b with a usable constant numerator stays a quotient -- its
        adjoint is -(y * y) / c and needs no reciprocal at all."""
        T = self.T
        if T.const[b]:
            return T.mul(a, T.recip(b)) if self.num_ok(b) else T._node("div", a, b)
        if T.const[a] and self.num_ok(a) and not shared:
            return T._node("div", a, b)
        return T.mul(a, T.recip(b))

    def cvals(self, node):
        """per-unit values of a constant template node"""
        if node not in self._cval:
            v = np.asarray(_np_eval(self.T, [node], self.const_leaf)[node], dtype=np.float64)
            self._cval[node] = np.broadcast_to(v, (self.n,))
        return self._cval[node]

    def cval(self, node):
        """the value of a constant template node that is the same for every unit, else None"""
        if not self.T.const[node]:
            return None
        v = self.cvals(node)
        return float(v[0]) if np.all(v == v[0]) else None

    def bounds(self, node):
        """(lo, hi, never NaN) of a template node over all units and all positions: what lets
        0 * x be folded to 0. Conservative: anything not proven is (-inf, inf, False). fmax / fmin
        return the other operand for a NaN (IEEE maxNum, the emitted fmax / fmin and v_max_f64)."""
        if node in self._bnd:
            return self._bnd[node]
        inf, unknown = math.inf, (-math.inf, math.inf, False)
        op = self.T.ops[node]
        k, r = op[0], unknown
        if self.T.const[node]:
            v = self.cvals(node)
            r = (float(np.min(v)), float(np.max(v)), True) if np.all(np.isfinite(v)) else unknown
        elif k in ("gat", "ext", "q", "red", "wred"):
            r = unknown
        else:
            b = [self.bounds(a) for a in op[1:]]
            fin = lambda x: x[2] and math.isfinite(x[0]) and math.isfinite(x[1])   # noqa: E731
            with np.errstate(all="ignore"):
                if k == "neg":
                    r = (-b[0][1], -b[0][0], b[0][2])
                elif k in ("add", "sub") and fin(b[0]) and fin(b[1]):
                    r = ((b[0][0] + b[1][0], b[0][1] + b[1][1], True) if k == "add"
                         else (b[0][0] - b[1][1], b[0][1] - b[1][0], True))
                elif k == "mul" and fin(b[0]) and fin(b[1]):
                    c = [x * y for x in b[0][:2] for y in b[1][:2]]
                    r = (min(c), max(c), True)
                elif k == "div" and fin(b[0]) and fin(b[1]) and (b[1][0] > 0.0 or b[1][1] < 0.0):
                    c = [x / y for x in b[0][:2] for y in b[1][:2]]
                    r = (min(c), max(c), True)
                elif k == "exp" and b[0][2] and b[0][1] < 700.0:
                    r = (float(np.exp(b[0][0])), float(np.exp(b[0][1])), True)
                elif k == "log" and fin(b[0]) and b[0][0] > 0.0:
                    r = (float(np.log(b[0][0])), float(np.log(b[0][1])), True)
                elif k == "log1p" and fin(b[0]) and b[0][0] > -1.0:
                    r = (float(np.log1p(b[0][0])), float(np.log1p(b[0][1])), True)
                elif k == "abs" and b[0][2]:
                    r = (0.0, max(abs(b[0][0]), abs(b[0][1])), True)
                elif k == "erf":
                    r = (-1.0, 1.0, b[0][2])
                elif k in ("max", "min") and (b[0][2] or b[1][2]):
                    los = [x[0] for x in b if x[2]]
                    his = [x[1] if x[2] else inf for x in b]
                    lo_all = [x[0] if x[2] else -inf for x in b]
                    r = ((max(los), max(his), True) if k == "max" else (min(lo_all), min(x[1] for x in b if x[2]), True))
                elif k == "sel_gt":
                    r = (min(b[2][0], b[3][0]), max(b[2][1], b[3][1]), b[2][2] and b[3][2])
            if not (r[0] == r[0] and r[1] == r[1]):          # a NaN bound proves nothing
                r = unknown
        self._bnd[node] = r
        return r

    def finite(self, node):
        lo, hi, ok = self.bounds(node)
        return ok and math.isfinite(lo) and math.isfinite(hi)

    def simple(self, node):
        """a constant that is 0, 1 or -1 in every unit as a literal (so that the exact rewrites of
        the graph's own mul / neg apply to it in the adjoint pass too)"""
        c = self.cval(node)
        return self.T.lit(c) if c in (0.0, 1.0, -1.0) and self.T.ops[node][0] != "lit" else node

    def make(self, kind, a):
        """a template node with the rewrites a constant factor or summand allows: 1 * x, x + 0 and
        0 * x for an x that is finite whatever the position (bounds)."""
        T, cval = self.T, self.cval
        if kind == "mul":
            for x, y in ((a[0], a[1]), (a[1], a[0])):
                c = cval(x)
                if c == 0.0 and self.finite(y):
                    return T.lit(0.0)
                if c == 1.0:
                    return y
                if c == -1.0:
                    return T.neg(y)
        elif kind == "add":
            if cval(a[0]) == 0.0:
                return a[1]
            if cval(a[1]) == 0.0:
                return a[0]
        elif kind == "sub":
            if cval(a[1]) == 0.0:
                return a[0]
            if cval(a[0]) == 0.0:
                return T.neg(a[1])
        return self.simple(T._node(kind, *a))


def _build_once(g, G, f, shared, share_recip):
    """The template of family f, its adjoints and its folded columns (the template fields of f).
    share_recip: shape nodes whose reciprocal the template needs anyway (_build_template)."""
    n, shape = len(f.members), f.shape
    S = (n + G - 1) // G
    f.n, f.S, f.npad = n, S, S * G
    root = len(shape) - 1
    # nodes of the template: reachable from the root without passing a uniform node
    need = cg._reachable([root], lambda k: shape[k][1:] if not f.uniform[k] and shape[k][0] not in
                         ("lit", "wlit", "q", "data") else ())
    tp = _Template(n, shared.uc_vals)
    T, tmap = tp.T, {}
    f.raw_cols, f.gather = tp.raw_cols, []     # raw data columns; gathered q indices per unit
    for k in sorted(need):
        node0 = f.ids[0][k]
        kind = shape[k][0]
        if kind == "lit":
            tmap[k] = T._node("lit", shape[k][1])
        elif kind == "wlit" and f.uniform[k]:
            tmap[k] = T._node("lit", g.ops[node0][1])
        elif f.uniform[k]:
            tmap[k] = T._node("uc", shared.uc_node(node0)) if g.const[node0] else T._node("ext", shared.ext(node0))
        elif kind == "q":
            f.gather.append([g.ops[ids[k]][1] for ids in f.ids])
            tmap[k] = T._node("gat", len(f.gather) - 1)
        elif kind in ("data", "wlit"):
            vals = [g.data[g.ops[ids[k]][1]] if kind == "data" else float.fromhex(g.ops[ids[k]][1])
                    for ids in f.ids]
            if all(v == vals[0] for v in vals):
                tmap[k] = (T.lit(vals[0]) if vals[0] in (0.0, 1.0, -1.0)
                           else T._node("uc", shared.uc_value(vals[0])))
            else:
                f.raw_cols.append(np.asarray(vals, dtype=np.float64))
                tmap[k] = T._node("col", -len(f.raw_cols))      # raw columns: negative ids
        elif kind == "div":
            tmap[k] = tp.quotient(tmap[shape[k][1]], tmap[shape[k][2]], shape[k][2] in share_recip)
        else:
            tmap[k] = tp.make(kind, [tmap[a] for a in shape[k][1:]])
    f.T, f.troot = T, tmap[root]
    n_fwd = len(T.ops)
    ad = cg._Grad(T, f.troot, const_num_ok=tp.num_ok)
    ad.run(n_fwd)
    f.ext_adj = {}
    for key, node in list(T.key.items()):
        if key[0] == "ext" and ad.adj.get(node) is not None:
            f.ext_adj[key[1]] = ad.adj[node]
    f.gat_adj = [ad.adj.get(T.key[("gat", p)]) for p in range(len(f.gather))]
    # fold what depends on constants only (per-unit data, uniform constants) into columns
    outputs = [f.troot] + list(f.ext_adj.values()) + [a for a in f.gat_adj if a is not None]
    live = set(cg._reachable(outputs, lambda i: T.ops[i][1:] if T.ops[i][0] not in _LEAVES and not T.const[i] else ()))
    fold = sorted(i for i in live if T.const[i] and T.ops[i][0] not in ("lit", "uc"))
    vals = _np_eval(T, fold, tp.const_leaf)
    f.cols, f.col_of = [], {}
    for i in fold:
        v = np.broadcast_to(np.asarray(vals[i], dtype=np.float64), (n,))
        if np.all(v == v[0]):
            f.col_of[i] = ("uc", shared.uc_value(v[0]))
        else:
            f.col_of[i] = ("col", len(f.cols))
            f.cols.append(np.array(v))
    f.live, f.tmap = live, tmap


def _build_template(g, G, f, shared, sh_off):
    """Twice: the second time the quotients by a denominator whose reciprocal the first pass
    needed anyway (the adjoint of log b, of another quotient) take that reciprocal too.
    sh_off: the first free double of the LDS strip; -> the first one after f's adjoint strips."""
    _build_once(g, G, f, shared, frozenset())
    T = f.T
    shared_recip = frozenset(k for k, node in f.tmap.items()
                             if T.key.get(("div", T.lit(1.0), node)) in f.live and not T.const[node])
    if shared_recip:
        _build_once(g, G, f, shared, shared_recip)
    # LDS strips of the gathered adjoints
    f.strip = []
    for p in range(len(f.gather)):
        f.strip.append(sh_off if f.gat_adj[p] is not None else -1)
        if f.gat_adj[p] is not None:
            sh_off += f.npad
    return sh_off


class _Layout:
    """The plan of one lane layout: what the stages of _generate hand on, each group filled by the
    stage named in front of it."""
    __slots__ = (
        # _generate: the graph, d, lanes per chain, dimensions per lane, resident waves per SIMD, the scan
        # chains, and the first double of the LDS strip after [position][0.0][walks][walk adjoints]
        "g", "D", "G", "DPL", "waves_per_simd", "chains", "sh_base",
        # _generate (plan, _build_template): the families with their templates, the units left to the uniform
        # part, the shared numberings, and the doubles of the strip with the families' adjoint strips
        "families", "scalar_units", "shared", "lsh",
        # _uniform_part
        "scalar_lp",      # the sum of the scalar units
        "ufams", "uf_of",  # spread sums inside the uniform part (_uniform_families); sum node -> its family
        "NW",             # doubles of w[]: per spread sum its value and the partials of its inputs
        "n_split",        # graph nodes below this are evaluated before the family loops, the others after
        "acc_of", "NS",   # boundary index -> slot of s[] that reduces its adjoint; doubles of s[]
        "ug",             # dimension -> node of the uniform part's gradient entry
        "live",           # the nodes of the graph the uniform part evaluates or reads
        "after_w",        # those of them that need a spread sum (emitted after its butterfly)
        # _owner_lists
        "width",          # per slot k: the longest list of strip cells a dimension of that slot adds
        "ell_off",        # per slot k: where its cells start in a lane's list
        "NELL", "ell",    # ints of one lane's list; the lists of all lanes, lane after lane
        # _table_layout
        "NUC",            # uniform constants, padded to 128 bytes
        "ioff_doubles",   # where the int32 part starts, in doubles
        "ell_base",       # where the owner lists start in the int32 part
        "data",           # the table
    )

    def __init__(self, g, D, G, waves_per_simd, chains, sh_base):
        self.g, self.D, self.G, self.DPL = g, D, G, (D + G - 1) // G
        self.waves_per_simd, self.chains, self.sh_base = waves_per_simd, chains, sh_base


def _uniform_part(p):
    """The uniform part: scalar units + the boundary nodes, differentiated with the reduced
    adjoints as seeds (U = scalar_lp + sum_j red_j * b_j)."""
    g, shared, chains, boundary = p.g, p.shared, p.chains, p.shared.boundary
    scalar_lp = None
    for t in p.scalar_units:
        scalar_lp = t if scalar_lp is None else g.add(t, scalar_lp)
    if scalar_lp is None:
        scalar_lp = g.lit(0.0)
    p.scalar_lp = scalar_lp

    # ---- families INSIDE the uniform part: a sum of like terms of shared values only (the eight
    # quotients of a Lanczos series, math.ex:27-52) is evaluated one term per lane and reduced in a
    # butterfly of its own before the family loops, instead of by every lane in full. Per term the
    # value and its partial derivatives with respect to the term's uniform inputs; the tangent of the
    # sum is sum_e (reduced partial e) * tangent(e). One level: a sum whose inputs need another
    # spread sum stays where it is. ----
    ufams = p.ufams = _uniform_families(g, [scalar_lp] + list(boundary))
    for f in ufams:
        _build_template(g, p.G, f, shared, p.lsh)
        if f.gather:
            raise cg.CodegenError("internal: a uniform family gathered a variable")
    uf_of = p.uf_of = {f.out: f for f in ufams}
    p.NW = 0
    for f in ufams:
        f.w0 = p.NW
        f.w_of = {j: f.w0 + 1 + k for k, j in enumerate(sorted(f.ext_adj))}
        p.NW += 1 + len(f.ext_adj)
        cpart = np.float64(0.0)
        for c in f.const_part:                 # folded left to right, added after the reduction
            cpart = cpart + np.float64(_const_value(g, c))
        f.cpart = float(cpart)
    p.n_split = len(g.ops)
    for ci, c in enumerate(chains):            # the scans' run-time values: sum_e z_e A_e and A_0
        c.sz, c.a0 = g._node("scn", 2 * ci), g._node("scn", 2 * ci + 1)
    # reduced values: s[0] = log-density of the families, s[1 + j] = adjoint of boundary node j
    acc_of = p.acc_of = {}
    for f in p.families:
        for j in sorted(f.ext_adj):
            if j not in acc_of:
                acc_of[j] = 1 + len(acc_of)
    p.NS = 1 + len(acc_of)
    # Forward mode for the uniform part: it has few inputs (the shared variables) and is evaluated
    # BEFORE the family loops, while its reduced adjoint seeds only exist after them -- a reverse
    # sweep would keep every intermediate of e.g. two Lanczos series alive across the loops (a
    # hundred vector registers in the sampling kernel). Tangents d node / d shared variable are
    # computed next to the values instead; what stays live is the Jacobian of the boundary nodes:
    #   d logp / d q_i = d scalar_lp / d q_i + sum_j red_j * d b_j / d q_i
    scan_inputs = [x for c in chains for x in (c.head, c.sigma)]
    spread = {f.out: [(boundary[j], g._node("wred", f.w_of[j])) for j in sorted(f.ext_adj)] for f in ufams}
    tan = _forward_tangents(g, [scalar_lp] + list(boundary) + scan_inputs, spread)
    ug = p.ug = {}
    for i in range(p.D):
        acc = tan.get(scalar_lp, {}).get(i)
        for j, sl_ in sorted(acc_of.items(), key=lambda kv: kv[1]):
            tj = tan.get(boundary[j], {}).get(i)
            if tj is not None:
                term = g.mul(g._node("red", sl_), tj)
                acc = term if acc is None else g.add(acc, term)
        for c in chains:                       # d/dsigma += sum_e z_e A_e, d/dhead += A_0
            for x, tj in ((c.sz, tan.get(c.sigma, {}).get(i)), (c.a0, tan.get(c.head, {}).get(i))):
                if tj is not None:
                    term = g.mul(x, tj)
                    acc = term if acc is None else g.add(acc, term)
        if acc is not None:
            ug[i] = acc

    # liveness of the uniform graph (a spread sum's terms are evaluated by the lanes, not here)
    def children(i):
        if i in uf_of:
            return uf_of[i].inputs
        return g.ops[i][1:] if g.ops[i][0] not in _LEAVES and not g.const[i] else ()
    live = p.live = set(cg._reachable([scalar_lp] + list(ug.values()) + list(boundary) + scan_inputs, children))
    # a walk value is read by the lanes' families only: the uniform part runs before the forward scans
    # and after the backward ones (module docstring, scan chains)
    read = [c for c in chains if any(g.ops[i][0] == "q" and c.w0 < g.ops[i][1] <= c.w0 + c.m for i in live)]
    if read:
        raise _WalkRead(read)
    for i in sorted(live):
        if g.const[i] and g.ops[i][0] != "lit":
            shared.uc_node(i)
    for f in ufams:
        if f.const_part:
            shared.uc_value(f.cpart)
    # nodes that need a spread sum come after its butterfly
    after_w = p.after_w = set()
    for i in sorted(live):
        if i in uf_of or (not g.const[i] and g.ops[i][0] not in _LEAVES and any(a in after_w for a in g.ops[i][1:])):
            after_w.add(i)


def _owner_lists(p):
    """The gather lists of the owner lanes (padded to the widest lane per slot): which strip cells
    the lane that owns a dimension, or an element of a scan chain, adds."""
    D, G, DPL, chains = p.D, p.G, p.DPL, p.chains
    contrib = [[] for _ in range(p.sh_base)]
    for f in p.families:
        for q in range(len(f.gather)):
            if f.strip[q] < 0:
                continue
            for u, var in enumerate(f.gather[q]):
                contrib[var].append(f.strip[q] + u)
    for c in chains:                           # d/dz_e += sigma A_e: the cell the backward scan writes
        for e, var in enumerate(c.z, 1):
            contrib[var].append(c.ga0 + e)
    width = p.width = [0] * DPL
    for i in range(D):
        width[i // G] = max(width[i // G], len(contrib[i]))
    zero_cell = D
    # per lane contiguous: [lane][slot k][j < width[k]] -- a lane's whole list is NELL ints, which the
    # device functor keeps in registers when it is short (Lane::ell)
    p.ell_off, NELL = [], 0
    for k in range(DPL):
        p.ell_off.append(NELL)
        NELL += width[k]
    for c in chains:                           # then each walk's elements: [slot k][j < c.W]
        c.W = max(len(contrib[c.w0 + e]) for e in range(c.m + 1))
        c.eoff = NELL
        NELL += c.N * c.W
    p.NELL = NELL
    ell = p.ell = []
    for l in range(G):
        for k in range(DPL):
            i = l + k * G
            for j in range(width[k]):
                ell.append(contrib[i][j] if (i < D and j < len(contrib[i])) else zero_cell)
        for c in chains:
            for k in range(c.N):
                e = l + k * G
                cells = contrib[c.w0 + e] if e <= c.m else []
                ell.extend(cells[j] if j < len(cells) else zero_cell for j in range(c.W))


def _table_layout(p):
    """The table: [uc][double columns][int32 columns (gather indices, owner lists)].
    Per-unit columns in PAIRS since round 6: columns 2p and 2p + 1 of a family are interleaved over its units
    (unit u's two entries at doff + 2 p npad + 2 u, + 1; an odd last column alone, one double per unit), the first
    pair on a 128-byte boundary of the table. A unit's pair is one 16-byte load, and the G lanes of a chain --
    and the 64 / G chains of a wavefront, which read the same units -- read 16 G CONSECUTIVE bytes per load:
    whole cache lines from L2, and no bank conflict when the table sits in an LDS image. Row-major (unit u's
    columns consecutive: a stride of 8 ncol bytes between lanes) cost the generated 500 x 20 regression 21
    bank-conflict cycles per LDS read in the workgroup form (profiles/r6_gen_wg)."""
    uc_vals = p.shared.uc_vals
    NUC = max(1, len(uc_vals))
    NUC += (-NUC) % 16
    p.NUC = doff = NUC
    for f in p.families + p.ufams:
        nc_ = len(f.cols)
        # (offset, stride in doubles) of column c. Short rows stay row-major (unit u's columns consecutive): one or
        # two loads per unit either way, and the lone-wave kernels of radon / sv measured 3-7 % slower in pairs
        f.paired = nc_ >= PAIR_MIN_COLS
        if f.paired:
            f.cpos = [(doff + (c // 2) * 2 * f.npad + (c & 1), 2) if c < nc_ - (nc_ & 1)
                      else (doff + (nc_ - 1) * f.npad, 1) for c in range(nc_)]
        else:
            f.cpos = [(doff + c, nc_) for c in range(nc_)]
        doff += nc_ * f.npad
    ints = []
    for f in p.families:
        f.ioff = len(ints)
        for q in range(len(f.gather)):
            ints.extend(list(f.gather[q]) + [f.gather[q][0]] * (f.npad - f.n))
    for c in p.chains:                         # the position index of z_e, element e of the scan
        c.zoff = len(ints)
        ints.extend([0] + list(c.z) + [0] * (c.N * 64 - c.m - 1))
    p.ell_base = len(ints)
    ints.extend(p.ell)
    if len(ints) % 2:
        ints.append(0)
    dtab = [np.asarray(uc_vals + [0.0] * (NUC - len(uc_vals)), dtype=np.float64)]
    for f in p.families + p.ufams:
        if f.cols:
            rows = np.stack(f.cols, axis=1)                       # [n][ncol]
            rows = np.concatenate([rows, np.repeat(rows[:1], f.npad - f.n, axis=0)])
            nc_ = rows.shape[1]
            if not f.paired:
                dtab.append(rows.ravel())                                               # [npad][ncol]
                continue
            for p_ in range(nc_ // 2):
                dtab.append(np.ascontiguousarray(rows[:, 2 * p_:2 * p_ + 2]).ravel())   # [npad][2]
            if nc_ & 1:
                dtab.append(np.ascontiguousarray(rows[:, nc_ - 1]))                     # [npad]
    p.data = np.concatenate(dtab + [np.asarray(ints, dtype=np.int32).view(np.float64)]) \
        if ints else np.concatenate(dtab)
    p.ioff_doubles = doff


# ---------------------------------------------------------------------------------------------
# emission
# ---------------------------------------------------------------------------------------------
_FN1L = {k: v.replace("EXMC_GEN_", "EXMC_GENL_") for k, v in cg._FN1.items()}


def _fuse_plan(gr, nodes, pinned):
    """Contraction at emission (the lane layout's own numeric contract, like the fma chains of the
    hand-written kernels): a product with a single consumer that is a sum or a difference is
    emitted as one fused multiply-add. -> {consumer: (form, side, product)}, the set of absorbed
    products, and the pinned products nobody else reads (fused into their accumulation)."""
    uses = {}
    for i in nodes:
        for a in gr.ops[i][1:]:
            uses[a] = uses.get(a, 0) + 1
    plan, gone = {}, set()
    for i in nodes:
        op = gr.ops[i]
        if op[0] not in ("add", "sub"):
            continue
        for side in (1, 0):
            m = op[1 + side]
            if (m in nodes and gr.ops[m][0] == "mul" and uses.get(m, 0) == 1 and m not in pinned
                    and m not in gone and not gr.const[m]):
                plan[i] = (op[0], side, m)
                gone.add(m)
                break
    acc_mul = set(m for m in pinned if m in nodes and gr.ops[m][0] == "mul" and uses.get(m, 0) == 0
                  and not gr.const[m])
    return plan, gone, acc_mul


def _node_text(gr, i, plan, ref):
    """The expression of node i: a fused multiply-add where the plan has one, else its operator."""
    if i not in plan:
        return cg._expr_text(gr.ops[i][0], [ref(x) for x in gr.ops[i][1:]], _FN1L)
    kind, side, m = plan[i]
    a, b = (ref(x) for x in gr.ops[m][1:])
    other = ref(gr.ops[i][2 - side])
    if kind == "add":
        return "EXMC_GEN_FMA(%s, %s, %s)" % (a, b, other)
    if side == 1:                               # other - a * b
        return "EXMC_GEN_FMA(-(%s), %s, %s)" % (a, b, other)
    return "EXMC_GEN_FMA(%s, %s, -(%s))" % (a, b, other)     # a * b - other


class _UniformText:
    """The statements of the uniform part. Chain-scalar transcendentals are the same instruction
    stream whatever their argument: the logs (exps, reciprocals) of one dependency level are
    evaluated together, argument i by lane i of the group, and broadcast back (exmc_device.hpp
    lane_batch) -- each value by exactly the operations of the plain call, so the host checker's
    loop gives the same bits."""
    BATCH = {"log": "LOG", "exp": "EXP", "log1p": "LOG1P", "rcp": "RCP"}

    def __init__(self, p):
        g = p.g
        self.p, self.n_batches = p, 0           # batches are numbered through all regions
        self.nodes = set(i for i in p.live if not g.const[i] and g.ops[i][0] not in _LEAVES and i not in p.uf_of)
        pinned = set([p.scalar_lp] + list(p.ug.values()) + list(p.shared.boundary)
                     + [x for c in p.chains for x in (c.head, c.sigma)])
        self.plan, self.gone, _ = _fuse_plan(g, self.nodes, pinned)

    def ref(self, i):
        g = self.p.g
        op = g.ops[i]
        if op[0] == "lit":
            return cg._lit_text(op[1])
        if op[0] == "red":
            return "s[%d]" % op[1]
        if op[0] == "wred":
            return "w[%d]" % op[1]
        if op[0] == "scn":
            return "sc%d" % op[1]
        if g.const[i]:
            return "EXMC_GEN_LT(%d)" % self.p.shared.uc_of[("node", i)]
        return "u%d" % i

    def batch_kind(self, i):
        op = self.p.g.ops[i]
        if op[0] in ("log", "exp", "log1p"):
            return op[0]
        if op[0] == "div" and self.p.g.lit_value(op[1]) == 1.0:
            return "rcp"
        return None

    def stmts(self, lo, hi, late=None):
        """The nodes lo <= i < hi; late: only those after (True) / before (False) the spread sums."""
        p, g, ref, batch_kind = self.p, self.p.g, self.ref, self.batch_kind
        out = []
        if lo == 0 and not late:     # the shared variables: broadcast reads of the position strip
            out.extend("  const double u%d = EXMC_GEN_SH(%d);" % (i, g.ops[i][1])
                       for i in sorted(p.live) if g.ops[i][0] == "q")
        region = [i for i in sorted(self.nodes)
                  if lo <= i < hi and (late is None or (i in p.after_w) == late)]
        level = {}
        for i in region:
            lv = max([level.get(a, 0) for a in g.ops[i][1:]] or [0])
            level[i] = lv + (1 if batch_kind(i) else 0)
        for lv in range(0, max(level.values(), default=0) + 1):
            groups = {}
            for i in region:
                if level[i] == lv and batch_kind(i):
                    groups.setdefault(batch_kind(i), []).append(i)
            for kind in sorted(groups):
                ids = groups[kind]
                for c0 in range(0, len(ids), min(p.G, 16)):
                    chunk = ids[c0:c0 + min(p.G, 16)]
                    args = [ref(g.ops[i][2] if kind == "rcp" else g.ops[i][1]) for i in chunk]
                    if len(chunk) == 1:
                        i = chunk[0]
                        out.append("  const double u%d = %s;" % (i, _node_text(g, i, {}, ref)))
                        continue
                    b = "b%d" % self.n_batches
                    self.n_batches += 1
                    out.append("  double %s[%d] = {%s};" % (b, len(chunk), ", ".join(args)))
                    out.append("  EXMC_GEN_BATCH_%s(%d, %s);" % (self.BATCH[kind], len(chunk), b))
                    out.extend("  const double u%d = %s[%d];" % (i, b, j) for j, i in enumerate(chunk))
            for i in region:
                if level[i] == lv and not batch_kind(i) and i not in self.gone:
                    out.append("  const double u%d = %s;" % (i, _node_text(g, i, self.plan, ref)))
        return out


def _header_lines(p):
    """The lane layout's #define block and the head of the lane function. -> lines, EXMC_GEN_WG"""
    G, DPL, families, data = p.G, p.DPL, p.families, p.data
    L = []
    L.append("/* lane layout (exmc_amd/codegen_lanes.py): %d lanes per chain, %d dimensions per lane;"
             % (G, DPL))
    L.append(" * %d famil%s of repeated terms (%s units), %d uniform term%s. lt = [%d uniform constants]"
             % (len(families), "y" if len(families) == 1 else "ies",
                " + ".join(str(f.n) for f in families) or "0", len(p.scalar_units),
                "" if len(p.scalar_units) == 1 else "s", p.NUC))
    L.append(" * [per-unit columns][int32: gather indices, owner lists]; EXMC_GEN_SH(i) = double i of the")
    L.append(" * chain's LDS strip: [position (d)][0.0][adjoint strips]. */")
    L.append("#define EXMC_GEN_LANES %d" % G)
    L.append("#define EXMC_GEN_DPL %d" % DPL)
    L.append("#define EXMC_GEN_LSH %d" % p.lsh)
    L.append("#define EXMC_GEN_NS %d" % p.NS)
    L.append("#define EXMC_GEN_NW %d   /* sums of the spread part of the uniform terms (0: none) */" % p.NW)
    L.append("#define EXMC_GEN_NLT %d" % data.size)
    L.append("#define EXMC_GEN_NELL %d   /* ints of a lane's owner list */" % max(1, p.NELL))
    L.append("#define EXMC_GEN_ELL_OFF %d   /* ... of lane l at ((const int*)lt)[EXMC_GEN_ELL_OFF + l * EXMC_GEN_NELL] */"
             % (2 * p.ioff_doubles + p.ell_base))
    L.append("#define EXMC_GEN_WAVES_PER_SIMD %d" % p.waves_per_simd)
    # the sampling kernel as workgroups of eight wavefronts around ONE LDS image of the tables (exmc_nuts.hpp
    # nuts_kernel_wg): for a layout of several chains per wavefront with two waves per SIMD whose tables are too
    # large to sit beside a one-wave workgroup (exmc_models.hpp EXMC_GEN_TABLE_IN_LDS) and fit beside eight tree
    # stacks, the ziggurat tables and eight sets of strips in a compute unit's 160 KB
    wg_lds = 8 * ((5 * DPL + 3) * 64 * 8 + (64 // G) * p.lsh * 8) + 768 * 8 + 8 + int(data.size) * 8
    wg = int(G < 64 and p.waves_per_simd == 2 and data.size > 2048 and wg_lds <= 160 * 1024)
    L.append("#define EXMC_GEN_WG %d   /* 1: the plug-in carries the workgroup form of the sampling kernel too */" % wg)
    L.append("")
    L.append("#define EXMC_GEN_IOFF %d   /* the int32 tables start at double EXMC_GEN_IOFF of lt */" % p.ioff_doubles)
    L.append("")
    if p.chains:
        L.extend(_scan_host_defaults(p.chains))
    L.append("#else   /* EXMC_GEN_LANES_SECTION: the lane function itself. Included once per table placement")
    L.append("       * with EXMC_GEN_LANES_NAME, EXMC_GEN_LT(i) (double i of the table) and EXMC_GEN_IT(i) (int32 i")
    L.append("       * of its index part) defined by the includer: global memory, or an LDS image of it */")
    L.append("EXMC_GEN_FN double EXMC_GEN_LANES_NAME(const double* lt, const int* el, int l, double* g EXMC_GEN_CTX_DECL) {")
    L.append("  EXMC_GEN_SH(%d) = 0.0;" % p.D)      # the zero cell
    return L, wg


def _loop_head(p, f, split):
    """A family's loop over the lane's slots up to the unit's loads: un, v<p> (gathered variables),
    c<c> (table columns). -> lines, blocked (which closing _loop_tail writes).
    A unit's table row and gathered variables are loads the unit's arithmetic waits for, and a
    lone wave per SIMD has nothing else to issue meanwhile (radon: 15 slots x ~800 clocks of L2
    latency per leapfrog against ~900 vector instructions). Short rows are therefore fetched
    for a block of slots at once -- the indices, then the variables, then the arithmetic."""
    G = p.G
    g0, ng = ("EXMC_GEN_G0", "EXMC_GEN_NG") if split else ("0", "1")   # (the groups of the wavefront
    nc, ngat = len(f.cols), len(f.gather)                                #  share a family in the one-chain warmup)
    B = max(1, min(f.S, PREFETCH_DOUBLES[p.waves_per_simd] // max(1, nc + ngat)))
    blocked = B > 1 and (nc + ngat) > 0
    L = []
    if blocked:
        L.append("  for (int jb = 0; %s + jb * %s < %d; jb += %d) {" % (g0, ng, f.S, B))
        L.append("    int un_[%d];" % B)
        if nc:
            L.append("    double c_[%d][%d];" % (B, nc))
        if ngat:
            L.append("    int ix_[%d][%d];" % (B, ngat))
            L.append("    double v_[%d][%d];" % (B, ngat))
        L.append("    for (int j = 0; j < %d; j++) {" % B)
        L.append("      const int sl = %s + (jb + j) * %s;" % (g0, ng))
        L.append("      const int un = sl * %d + l;" % G)
        L.append("      un_[j] = (sl < %d && un < %d) ? un : -1;" % (f.S, f.n))
        L.append("      const int uc = un_[j] < 0 ? 0 : un;")
        for c in range(nc):
            if f.paired and c + 1 < nc and not (c & 1):   # a pair: ONE 16-byte load (EXMC_GEN_LT2: aligned)
                L.append("      { const exmc_gen_d2 cc_ = EXMC_GEN_LT2(%d + uc * 2); c_[j][%d] = cc_.x; c_[j][%d] = cc_.y; }"
                         % (f.cpos[c][0], c, c + 1))
            elif not (f.paired and (c & 1)):
                L.append("      c_[j][%d] = EXMC_GEN_LT(%d + uc * %d);" % (c, f.cpos[c][0], f.cpos[c][1]))
        for q in range(ngat):
            L.append("      ix_[j][%d] = EXMC_GEN_IT(%d + uc);" % (q, f.ioff + q * f.npad))
        L.append("    }")
        if ngat:
            L.append("    for (int j = 0; j < %d; j++) {" % B)
            for q in range(ngat):
                L.append("      v_[j][%d] = EXMC_GEN_SH(ix_[j][%d]);" % (q, q))
            L.append("    }")
        L.append("    for (int j = 0; j < %d; j++) {" % B)
        L.append("    const int un = un_[j];")
        L.append("    if (un >= 0) {")
        for q in range(ngat):
            L.append("    const double v%d = v_[j][%d];" % (q, q))
        for c in range(nc):
            L.append("    const double c%d = c_[j][%d];" % (c, c))
    else:
        L.append("  for (int sl = %s; sl < %d; sl += %s) {" % (g0, f.S, ng))
        L.append("    const int un = sl * %d + l;" % G)
        if f.n < f.npad:
            L.append("    if (un < %d) {" % f.n)
        for q in range(ngat):
            L.append("    const double v%d = EXMC_GEN_SH(EXMC_GEN_IT(%d + un));" % (q, f.ioff + q * f.npad))
        for c in range(nc):
            if f.paired and c + 1 < nc and not (c & 1):   # a pair: ONE 16-byte load (EXMC_GEN_LT2: aligned)
                L.append("    const exmc_gen_d2 cc%d = EXMC_GEN_LT2(%d + un * 2);" % (c, f.cpos[c][0]))
                L.append("    const double c%d = cc%d.x;" % (c, c))
                L.append("    const double c%d = cc%d.y;" % (c + 1, c))
            elif not (f.paired and (c & 1)):
                L.append("    const double c%d = EXMC_GEN_LT(%d + un * %d);" % (c, f.cpos[c][0], f.cpos[c][1]))
    return L, blocked


def _loop_tail(f, blocked):
    if blocked:
        return ["    }", "    }", "  }"]
    return ["    }", "  }"] if f.n < f.npad else ["  }"]


def _emit_family(p, uref, f, title, arr, slot_of, tag, split=False):
    """The loop of family f: per unit the template's value and adjoints, accumulated into arr[] by
    slot_of (None: the value, j: the adjoint of boundary node j) and written to the adjoint strips.
    tag names what is evaluated once in front of the loop; split: see _loop_head."""
    T = f.T
    t_nodes = set(i for i in f.live if not T.const[i] and T.ops[i][0] not in _LEAVES)
    # what does not change from unit to unit (a function of uniform values and uniform constants
    # only: the reciprocal of a shared scale) is evaluated once, in front of the loop
    fixed = {}
    for i in sorted(f.live):
        op = T.ops[i]
        if op[0] in ("lit", "uc", "ext"):
            fixed[i] = True
        elif op[0] in ("col", "gat"):
            fixed[i] = False
        elif i in f.col_of:
            fixed[i] = f.col_of[i][0] == "uc"
        else:
            fixed[i] = all(fixed.get(a, False) for a in op[1:])
    hoisted = set(i for i in t_nodes if fixed[i])

    def tref(i):
        op = T.ops[i]
        if op[0] == "lit":
            return cg._lit_text(op[1])
        if op[0] == "uc":
            return "EXMC_GEN_LT(%d)" % op[1]
        if i in f.col_of:
            kind, k = f.col_of[i]
            return "EXMC_GEN_LT(%d)" % k if kind == "uc" else "c%d" % k
        if op[0] == "ext":
            return uref(p.shared.boundary[op[1]])
        if op[0] == "gat":
            return "v%d" % op[1]
        return ("%s_%d" % (tag, i)) if i in hoisted else ("t%d" % i)
    gat_adj = [a for a in f.gat_adj if a is not None]
    t_plan, t_gone, t_accmul = _fuse_plan(T, t_nodes, set([f.troot] + list(f.ext_adj.values()) + gat_adj))
    L = ["  /* %s: %d units, %d per lane */" % (title, f.n, f.S)]
    for i in sorted(hoisted):
        if i not in t_gone:
            L.append("  const double %s_%d = %s;" % (tag, i, _node_text(T, i, t_plan, tref)))
    head, blocked = _loop_head(p, f, split)
    L.extend(head)
    n_use = {}
    for x in [f.troot] + list(f.ext_adj.values()):
        n_use[x] = n_use.get(x, 0) + 1
    t_accmul = set(m for m in t_accmul if n_use.get(m, 0) == 1 and m not in gat_adj)

    def accumulate(slot, node):
        if node in t_accmul:
            a, b = (tref(x) for x in T.ops[node][1:])
            return "    %s[%d] = EXMC_GEN_FMA(%s, %s, %s[%d]);" % (arr, slot, a, b, arr, slot)
        return "    %s[%d] = %s[%d] + %s;" % (arr, slot, arr, slot, tref(node))
    for i in sorted(t_nodes):
        if not (i in t_gone or i in t_accmul or i in hoisted):
            L.append("    const double t%d = %s;" % (i, _node_text(T, i, t_plan, tref)))
    L.append(accumulate(slot_of[None], f.troot))
    for j in sorted(f.ext_adj):
        L.append(accumulate(slot_of[j], f.ext_adj[j]))
    for q in range(len(f.gather)):
        if f.strip[q] >= 0:
            L.append("    EXMC_GEN_SH(%d + un) = %s;" % (f.strip[q], tref(f.gat_adj[q])))
    return L + _loop_tail(f, blocked)


def _spread_lines(p, ut):
    """The spread sums of the uniform part, their butterfly, and what of the uniform part needs them."""
    if not p.ufams:
        return []
    L = ["  double w[EXMC_GEN_NW];", "  for (int j = 0; j < EXMC_GEN_NW; j++) w[j] = 0.0;"]
    for fi, f in enumerate(p.ufams):
        slots = dict(f.w_of)
        slots[None] = f.w0
        L.extend(_emit_family(p, ut.ref, f, "spread sum %d of the uniform part" % fi, "w", slots, "hw%d" % fi))
    L.append("  EXMC_GEN_ALLSUM_W(w);")
    for f in p.ufams:
        if f.const_part:
            L.append("  const double u%d = w[%d] + EXMC_GEN_LT(%d);"
                     % (f.out, f.w0, p.shared.uc_of[("val", f.cpart.hex())]))
        else:
            L.append("  const double u%d = w[%d];" % (f.out, f.w0))
    return L + ut.stmts(0, p.n_split, late=True)


def _scan_forward_lines(p, uref):
    L = []
    for ci, c in enumerate(p.chains):
        L.append("  /* scan chain %d: %s .. %s = %s + prefix sums of %s * z (%d increments, %d slots) */"
                 % (ci, c.ids[0], c.ids[-1], c.head_id, c.sigma_id, c.m, c.N))
        L.append("  double xw%d[%d];" % (ci, c.N))
        L.append("  for (int k = 0; k < %d; k++) {" % c.N)
        L.append("    const int e = l + 64 * k;")
        L.append("    xw%d[k] = (e == 0) ? %s : ((e <= %d) ? %s * EXMC_GEN_SH(EXMC_GEN_IT(%d + e)) : 0.0);"
                 % (ci, uref(c.head), c.m, uref(c.sigma), c.zoff))
        L.append("  }")
        L.append("  EXMC_GEN_SCAN_FWD(%d, xw%d, %d, %d, %s, %s, %d);"
                 % (c.N, ci, c.m, c.zoff, uref(c.head), uref(c.sigma), c.w0))
    return L


def _scan_backward_lines(p, uref):
    L = []
    if p.chains:
        L.append("  EXMC_GEN_FENCE();   /* the families' cells of the walk values */")
    for ci, c in enumerate(p.chains):
        L.append("  /* scan chain %d, adjoint: A_e = sum over u >= e of dlogp/ds_u; z_e gets %s * A_e, %s the sum"
                 % (ci, c.sigma_id, c.sigma_id))
        L.append("   * of z_e A_e, %s A_0 */" % c.head_id)
        L.append("  double aw%d[%d];" % (ci, c.N))
        L.append("  for (int k = 0; k < %d; k++) {" % c.N)
        L.append("    double acc = 0.0;")
        if c.W > 0:
            L.append("    for (int j = 0; j < %d; j++) acc = acc + EXMC_GEN_SH(el[%d + k * %d + j]);" % (c.W, c.eoff, c.W))
        L.append("    aw%d[k] = acc;" % ci)
        L.append("  }")
        L.append("  double sc%d, sc%d;" % (2 * ci, 2 * ci + 1))
        L.append("  EXMC_GEN_SCAN_BWD(%d, aw%d, %d, %d, %s, %d, %d, %d, sc%d, sc%d);"
                 % (c.N, ci, c.m, c.zoff, uref(c.sigma), c.eoff, c.W, c.ga0, 2 * ci, 2 * ci + 1))
    return L


def _gradient_lines(p, uref):
    """Per slot of the lane: the owner's sum of strip cells plus the uniform part's entry."""
    L = []
    for k in range(p.DPL):
        L.append("  {")
        L.append("    const int dim = l + %d;" % (k * p.G))
        L.append("    double acc = 0.0;")
        if p.width[k] > 0:
            L.append("    for (int j = 0; j < %d; j++) acc = acc + EXMC_GEN_SH(el[%d + j]);" % (p.width[k], p.ell_off[k]))
        sel = "0.0"
        for i in sorted(p.ug, reverse=True):
            if i // p.G == k:
                sel = "(dim == %d) ? %s : (%s)" % (i, uref(p.ug[i]), sel)
        L.append("    const double ugs = %s;" % sel)
        L.append("    g[%d] = acc + ugs;" % k)
        L.append("    (void)dim;")
        L.append("  }")
    return L


def _emit_text(p):
    """The text of the lane layout, in the order the lane function runs: the uniform part, the spread
    sums, the forward scans, the family loops and their butterfly, the backward scans, the
    uniform part's gradient, the owners' sums. -> text, EXMC_GEN_WG, number of batches"""
    ut = _UniformText(p)
    L, wg = _header_lines(p)
    L.extend(ut.stmts(0, p.n_split, late=False))
    L.extend(_spread_lines(p, ut))
    L.extend(_scan_forward_lines(p, ut.ref))
    L.append("  double s[EXMC_GEN_NS];")
    L.append("  for (int j = 0; j < EXMC_GEN_NS; j++) s[j] = 0.0;")
    for fi, f in enumerate(p.families):
        slots = dict(p.acc_of)
        slots[None] = 0
        L.extend(_emit_family(p, ut.ref, f, "family %d" % fi, "s", slots, "hf%d" % fi, split=True))
    L.append("  EXMC_GEN_ALLSUM(s);")
    L.append("  EXMC_GEN_XGROUP(s);   /* EXMC_GEN_NG > 1: the groups' sums, group 0 first */")
    L.extend(_scan_backward_lines(p, ut.ref))
    L.extend(ut.stmts(p.n_split, len(p.g.ops)))
    L.append("  EXMC_GEN_FENCE();")
    L.extend(_gradient_lines(p, ut.ref))
    L.append("  (void)el; (void)lt;")
    L.append("  return %s + s[0];" % ut.ref(p.scalar_lp))
    L.append("}")
    L.append("#endif")
    return "\n".join(L) + "\n", wg, ut.n_batches


def _generate(g, term_roots, custom_roots, D, G, waves_per_simd, chains, sh_base):
    """One attempt at the layout with the scan chains `chains` (generate): plan, templates, the
    uniform part (which raises _WalkRead), owner lists, table, text."""
    p = _Layout(g, D, G, waves_per_simd, chains, sh_base)
    p.families, p.scalar_units = plan(g, term_roots, custom_roots, D, G)
    p.shared = _Shared(g)
    p.lsh = sh_base          # LDS strip: [q (D)] [zero cell] [walks, walk adjoints] [adjoint strips ...]
    for f in p.families:
        p.lsh = _build_template(g, G, f, p.shared, p.lsh)
    _uniform_part(p)
    _owner_lists(p)
    _table_layout(p)
    text, wg, n_batches = _emit_text(p)
    scans = [dict(head=c.head_id, sigma=c.sigma_id, first=c.ids[0], last=c.ids[-1], increments=c.m, slots=c.N)
             for c in chains]
    return dict(text=text, data=p.data, lanes=G, dpl=p.DPL, lsh=p.lsh, n_families=len(p.families), scan_chains=scans,
                family_sizes=[f.n for f in p.families], n_scalar_units=len(p.scalar_units),
                spread_sizes=[f.n for f in p.ufams], n_spread_sums=p.NW, n_batches=n_batches,
                n_reduced=p.NS, n_boundary=len(p.shared.boundary), gather_width=p.width, wg=wg)
