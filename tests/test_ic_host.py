"""CPU tests of model comparison: the host statement (tests/host/ic_host_checker.c) against the
reference's formulas (lib/exmc/model_comparison.ex) and numpy statements of each kind's likelihood;
compare/1's ordering; the C header and its export list."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ic_checker as IC
from exmc_amd import _lib, models
from exmc_amd import model_comparison as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "exmc_hip_compare.h")


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    fin = np.isfinite(a) & np.isfinite(b)
    ok = same | (fin & (np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1e-300)))
    assert ok.all(), (a[~ok], b[~ok])


@pytest.mark.parametrize("S,N,Cn,seed", [(50, 7, 8, 1), (3, 5, 1, 2), (200, 3, 700, 3), (1, 4, 2, 4)])
def test_host_statement_equals_reference_formulas(S, N, Cn, seed):
    rng = np.random.default_rng(seed)
    ll = rng.normal(-3.0, 2.0, size=(S, N, Cn))
    _close(IC.stats_from_ll(ll), IC.reference_stats(ll), 1e-12)


def test_host_statement_on_many_chunks():
    # 140 000 samples: chunks of 64 * ceil(140000 / 65536) = 192 samples
    S, Cn = 700, 200
    assert IC.lib().ic_chunk(S * Cn) == 192
    rng = np.random.default_rng(5)
    ll = rng.normal(-1.0, 0.5, size=(S, 2, Cn))
    _close(IC.stats_from_ll(ll), IC.reference_stats(ll), 1e-12)


def hostile():
    rng = np.random.default_rng(11)
    S, Cn = 40, 6
    cols = []
    base = rng.normal(-2.0, 1.0, size=(S, Cn))
    m = base.copy(); m[0, 0] = -np.inf; cols.append(m)            # a leading -inf
    m = base.copy(); m[5, 3] = -np.inf; m[7, 1] = -np.inf; cols.append(m)
    cols.append(np.full((S, Cn), -1.25))                          # all equal
    cols.append(700.0 + rng.normal(0, 3.0, size=(S, Cn)))          # near exp's overflow
    cols.append(-700.0 + rng.normal(0, 3.0, size=(S, Cn)))
    cols.append(1e300 * rng.uniform(0.5, 1.0, size=(S, Cn)))       # huge magnitudes
    cols.append(-1e300 * rng.uniform(0.5, 1.0, size=(S, Cn)))
    m = base.copy(); m[9, 2] = np.nan; cols.append(m)             # NaN
    cols.append(np.full((S, Cn), -np.inf))                         # all -inf
    return np.stack(cols, axis=1)


def test_host_statement_on_hostile_matrices():
    ll = hostile()
    got = IC.stats_from_ll(ll)
    N = ll.shape[1]
    for i in range(N):
        v = [float(x) for x in ll[:, i, :].reshape(-1)]
        if any(math.isnan(x) for x in v):
            assert np.isnan(got[:, i]).all(), i
            continue
        if all(x == -math.inf for x in v):
            # the reference's max - max is NaN here; the online form gives the limits
            assert got[0, i] == -math.inf and got[2, i] == -math.inf, got[:, i]
            continue
        lppd = IC.log_mean_exp(v)
        if any(x == -math.inf for x in v):
            # -ll has a +inf: exp(-ll) has an infinite mean, elpd_loo_i = -inf (the reference: inf - inf)
            assert got[2, i] == -math.inf and got[3, i] == math.inf, got[:, i]
            _close(got[0, i], lppd, 1e-12)
            continue
        elpd = -IC.log_mean_exp([-x for x in v])
        var = IC.variance(v)
        _close(got[0, i], lppd, 1e-12)
        _close(got[2, i], elpd, 1e-12)
        _close(got[3, i], lppd - elpd, 1e-9 if abs(lppd) > 1e3 else 1e-12)
        if abs(v[0]) < 1e200:
            _close(got[1, i], var, 1e-10)
        else:
            assert got[1, i] == var or (math.isinf(got[1, i]) and math.isinf(var)), (got[1, i], var)
    assert (got[1, 2] == 0.0) and got[0, 2] == -1.25 and got[2, 2] == -1.25


def _kind_blob(kind, rng):
    if kind == models.SIMPLE:
        return np.asarray(models.SIMPLE_Y)
    if kind == models.EIGHT_SCHOOLS:
        return np.asarray(models.EIGHT_SCHOOLS_Y + models.EIGHT_SCHOOLS_SIGMA)
    if kind in (models.SV, models.SV_NCP):
        return models.sv_returns()
    if kind == models.LOGISTIC:
        return models.logistic().data
    return models.radon().data


LANCZOS = [0.99999999999980993, 676.5203681218851, -1259.1392167224028, 771.32342877765313,
           -176.61502916214059, 12.507343278686905, -0.13857109526572012, 9.9843695780195716e-6,
           1.5056327351493116e-7]


def _lanczos(x):
    """math.ex:27-52, the kinds' lgamma: Lanczos g = 7 with the coefficients as f32 tensors"""
    c = [float(np.float32(v)) for v in LANCZOS]
    ag = c[0] + sum(c[i] / (x + i - 1) for i in range(1, 9))
    t = x + 6.5
    return float(np.float32(0.5 * math.log(2 * math.pi))) + (x - 0.5) * math.log(t) - t + math.log(ag)


def _numpy_terms(kind, blob, q):
    """numpy/libm statements of each kind's per-datum likelihood (no exmc_detmath)"""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    l2p = f32(math.log(f32(2 * math.pi)))
    if kind == models.SIMPLE:
        s = max(math.exp(np.clip(q[1], -200, 200)), f32(1e-30))
        z = (blob - q[0]) / s
        return -0.5 * (z * z + (l2p + 2 * math.log(s)))
    if kind == models.EIGHT_SCHOOLS:
        y, sg = blob[:8], blob[8:]
        z = (y - (q[0] + math.exp(q[1]) * q[2:10])) / sg
        return -0.5 * (z * z + (l2p + 2 * np.log(sg)))
    if kind in (models.SV, models.SV_NCP):
        nu = math.exp(q[101])
        if kind == models.SV_NCP:
            s = np.cumsum(np.concatenate([[q[0]], math.exp(q[100]) * q[1:100]]))
        else:
            s = q[:100]
        lg = _lanczos((nu + 1) / 2) - _lanczos(nu / 2)
        z = blob * np.exp(-s)
        return lg - 0.5 * math.log(nu * float(np.float32(math.pi))) - s - (nu + 1) / 2 * np.log1p(z * z / nu)
    if kind == models.LOGISTIC:
        N = blob.size // 21
        X, y = blob[:N * 20].reshape(N, 20), blob[N * 20:]
        p = 1 / (1 + np.exp(-(q[0] + X @ q[1:])))
        pc = np.clip(p, f32(1e-7), 1 - f32(1e-7))
        return y * np.log(pc) + (1 - y) * np.log(1 - pc)
    J = 85
    N = (blob.size - 171) // 2
    u, cs, fl = blob[:J], blob[J:2 * J + 1].astype(int), blob[2 * J + 1:2 * J + 1 + N]
    y = blob[2 * J + 1 + N:]
    county = np.repeat(np.arange(J), np.diff(cs))
    alpha = q[J] + q[J + 1] * u + math.exp(q[J + 2]) * q[:J]
    sy = math.exp(q[J + 3])
    z = (y - (alpha[county] + q[J + 4] * fl)) / sy
    return -0.5 * (z * z + (l2p + 2 * math.log(sy)))


KINDS = [models.SIMPLE, models.EIGHT_SCHOOLS, models.SV, models.SV_NCP, models.LOGISTIC, models.RADON]


@pytest.mark.parametrize("kind", KINDS)
def test_host_terms_equal_numpy_likelihoods(kind):
    rng = np.random.default_rng(kind)
    blob = _kind_blob(kind, rng)
    d = {models.SIMPLE: 2, models.EIGHT_SCHOOLS: 10, models.SV: 102, models.SV_NCP: 102,
         models.LOGISTIC: 21, models.RADON: 90}[kind]
    for _ in range(5):
        q = rng.normal(0.0, 0.3, size=d)
        if kind in (models.SV, models.SV_NCP):
            q[100], q[101] = math.log(0.15) + 0.3 * rng.normal(), math.log(10.0) + 0.3 * rng.normal()
            q[:100] = rng.normal(-2.0, 0.3, size=100) if kind == models.SV else q[:100]
            if kind == models.SV_NCP:
                q[0] = -2.0
        got = IC.terms(kind, blob, q)
        np.testing.assert_allclose(got, _numpy_terms(kind, blob, q), rtol=1e-12, atol=1e-13)


def test_compare_orders_like_the_reference():
    a = dict(waic=10.0, elpd_waic=-5.0, p_waic=1.0, se=0.5, n_obs=3)
    b = dict(waic=4.0, elpd_waic=-2.0, p_waic=1.0, se=0.25, n_obs=3)
    c = dict(waic=10.0, elpd_waic=-5.0, p_waic=2.0, se=0.75, n_obs=3)
    out = MC.compare([("a", a), ("b", b), ("c", c)])
    assert [r["label"] for r in out] == ["b", "a", "c"]       # sort_by is stable
    assert [r["d_elpd"] for r in out] == [0.0, -3.0, -3.0]
    assert out[0] == dict(label="b", ic=4.0, elpd=-2.0, se=0.25, d_elpd=0.0)
    lo = MC.compare([("x", dict(loo=3.0, elpd_loo=-1.5, p_loo=0.1, se=0.0, n_obs=1)),
                     ("y", dict(loo=1.0, elpd_loo=-0.5, p_loo=0.1, se=0.0, n_obs=1))])
    assert [r["label"] for r in lo] == ["y", "x"] and lo[1]["d_elpd"] == -1.0


def test_totals_use_the_reference_formulas():
    lppd, pw = [-1.0, -2.5, -0.25], [0.5, 0.125, 1.0]
    r = MC.waic_totals(lppd, pw)
    elpd = sum(lppd) - sum(pw)
    ep = [a - b for a, b in zip(lppd, pw)]
    assert r["elpd_waic"] == elpd and r["waic"] == -2 * elpd and r["n_obs"] == 3
    assert r["se"] == math.sqrt(3 * IC.variance(ep))
    r = MC.loo_totals([-1.0], [0.5])
    assert r["se"] == 0.0 and r["loo"] == 2.0


def test_compare_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "exmc_hip_compare.h"\nint main(void){int (*f)(const exmc_hip_model*) = exmc_hip_model_n_data; return f != 0;}\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def declared(path=HDR):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(exmc_hip_\w+)\s*\(", txt)))


def test_compare_exports_equal_the_header():
    assert sorted(_lib.COMPARE_EXPORTS) == declared()
    assert not set(_lib.COMPARE_EXPORTS) & set(_lib.EXPORTS)


def test_every_handle_entry_point_of_the_header_is_in_the_state_catalogue():
    import test_gpu_ic_handle_state as HS
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    decls = re.findall(r"\b(exmc_hip_\w+)\s*\(([^)]*)\)", txt)
    handle = {n for n, p in decls if re.search(r"\bexmc_hip_model\s*\*", p)}
    covered = {n for names in HS.ENTRY_POINTS.values() for n in names}
    assert handle and handle <= covered, handle - covered


def test_radon_spec_maps_datums_back_to_the_callers_order():
    spec = models.radon()
    u, start, fl, y = models.radon_data()
    N = len(y)
    order = spec.datum_order
    assert sorted(order) == list(range(N))
    np.testing.assert_array_equal(spec.data[171 + N:], y[order])
