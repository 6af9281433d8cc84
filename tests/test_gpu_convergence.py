"""The convergence diagnostics across chains on the device (exmc_amd/csrc/exmc_convergence.hpp,
include/exmc_hip_convergence.h): all six rows byte for byte against tests/convergence_statement.py, at every
size at which the implementation takes another path, with every blocking of the dimensions, on the
degenerate columns a stuck or broken sampler produces, through the _host form, the Python call and a
generated model's plug-in library; and every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

import convergence_statement as CS
from exmc_amd import _lib, diagnostics, models, sampler

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)

# the sizes at which the implementation changes path (exmc_convergence.hpp): the pooled pairs of a
# dimension are sorted by one workgroup in LDS while their power of two P <= kConvTile = 4096, by the
# device-wide stages above; the tie runs are scanned in tiles of 1024 positions
LDS_SORT_LARGEST = (64, 1, 64)      # N = 4096 = P: the largest LDS sort
DEVICE_SORT_SMALLEST = (66, 1, 64)  # N = 4224, P = 8192: the smallest device-wide sort
ONE_RUN_TILE = (16, 2, 64)          # N = 1024: exactly one tile of the run scan
TWO_RUN_TILES = (18, 2, 57)         # N = 1026: a second tile of two positions

SHAPES = [(8, 1, 1), (101, 3, 5), (40, 10, 64), (80, 2, 70), (600, 1, 128), LDS_SORT_LARGEST,
          DEVICE_SORT_SMALLEST, ONE_RUN_TILE, TWO_RUN_TILES]

_cache = {}


def trace(S, D, Cn):
    """AR(1) series with chain-dependent correlation and a small chain-dependent offset, as
    tests/test_gpu_diagnostics.py makes them; with its statement, computed once"""
    key = (S, D, Cn)
    if key not in _cache:
        rng = np.random.default_rng(S + D)
        x = np.zeros((S, D, Cn))
        rho = rng.uniform(0.0, 0.95, size=(D, Cn))
        e = rng.normal(size=(S, D, Cn))
        x[0] = e[0]
        for i in range(1, S):
            x[i] = rho * x[i - 1] + e[i]
        x += 0.2 * rng.normal(size=(1, D, Cn))
        x = np.ascontiguousarray(x)
        want = CS.convergence(x)
        x.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (x, want)
    return _cache[key]


@pytest.fixture(scope="module")
def comp(hip):
    return sampler.compile(models.eight_schools())


def device_call(cm, x, scratch=0):
    S, D, Cn = x.shape
    xd = torch.tensor(x, device="cuda")
    out = torch.full((6, D), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    cm.check(cm.L.exmc_hip_convergence(cm.h, xd.data_ptr(), S, D, Cn, scratch, out.data_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def report(got, want):
    return "\n".join("%-10s got %r\n%-10s want %r" % (n, g, "", w) for n, g, w in zip(CS.ROWS, got, want))


@pytest.mark.parametrize("S,D,Cn", SHAPES)
def test_six_rows_equal_the_statement_byte_for_byte(comp, S, D, Cn):
    x, want = trace(S, D, Cn)
    got = device_call(comp, x)
    assert same_bits(got, want), report(got, want)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    assert comp.L.exmc_hip_last_kernel_ms(comp.h) > 0


@pytest.mark.parametrize("scratch,per_block", [(1, 1), (400_000, 2), (600_000, 3)])
def test_the_blocking_of_the_dimensions_does_not_show(comp, scratch, per_block):
    """(40, 10, 64) takes about 188 KB of scratch a dimension: `scratch` bytes hold `per_block` dimensions
    (1 byte: never fewer than one; three to a block leaves a last block of one)."""
    x, want = trace(40, 10, 64)
    got = device_call(comp, x, scratch)
    assert same_bits(got, want), report(got, want)


def test_host_form_and_python_call(comp):
    S, Cn = 24, 6
    x, want = trace(S, comp.d, Cn)
    host = np.ascontiguousarray(x.transpose(2, 0, 1))       # [C][S][d]
    out = np.full((6, comp.d), -7.0)
    comp.check(comp.L.exmc_hip_convergence_host(comp.h, host.ctypes.data_as(DP), S, comp.d, Cn, 0,
                                                out.ctypes.data_as(DP)))
    assert same_bits(out, want), report(out, want)
    for src in (host, torch.tensor(x, device="cuda")):
        rows = diagnostics.convergence(comp, src)
        assert list(rows) == list(CS.ROWS) + ["rhat"]
        assert same_bits(np.array([rows[k] for k in CS.ROWS]), want)
        assert same_bits(rows["rhat"], np.maximum(want[0], want[1]))
    names = ["v%d" % i for i in range(comp.d)]
    named = diagnostics.convergence(comp, host, names=names, scratch_bytes=1)
    assert list(named) == names
    assert all(named["v3"][k] == want[i, 3] for i, k in enumerate(CS.ROWS))
    with pytest.raises(ValueError):
        diagnostics.convergence(comp, host, names=names[:-1])
    with pytest.raises(ValueError):
        diagnostics.convergence(comp, torch.tensor(x, device="cuda").float())


def degenerate(S):
    rng = np.random.default_rng(900 + S)
    D, Cn = 9, 12
    x = rng.normal(size=(S, D, Cn))
    x[:, 0, 0] = 3.25                                         # constant
    x[:, 0, 1] = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)   # perfectly anti-correlated
    x[:, 0, 2] = np.where(np.arange(S) < S // 2, 0.0, 1.0)    # a step: the split halves disagree
    x[S // 2, 0, 3] = 1e300                                   # one outlier
    x[:, 0, 4] *= 1e-310                                      # denormal scale
    x[:, 0, 5] = np.where(np.arange(S) % 3 == 0, 0.0, -0.0)   # signed zeros only
    x[S // 3, 1, 0] = np.inf
    x[S // 3, 1, 1] = -np.inf
    x[0, 2, 3] = np.nan                                       # a NaN first
    x[S // 4, 3, 2] = np.nan                                  # a NaN in the middle
    x[2 * (S // 2) - 1, 4, 4] = np.nan                        # a NaN in the last draw that is used
    x[:, 5, :] = 7.0                                          # a whole dimension constant across chains
    x[:, 6, :] = np.arange(Cn)[None, :]                       # constant within chains, different between them
    x[:, 7, :] = np.where(rng.uniform(size=(S, Cn)) < 0.5, 0.0, -0.0)   # signed zeros only: one run of ties
    x[:, 8, :] = np.where(rng.uniform(size=(S, Cn)) < 0.3, 1.0, -1.0)   # two values: two long runs
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("S", [8, 64, 333])
def test_degenerate_columns_equal_the_statement(comp, S):
    """The columns of test_ess_and_rhat_kernels_on_degenerate_series_bit_exact, pooled per dimension: the
    statement's bits, NaN for NaN."""
    x = degenerate(S)
    want = CS.convergence(x)
    got = device_call(comp, x)
    assert same_bits(got, want), report(got, want)
    for dim in (2, 3, 4, 5, 7):
        assert np.all(np.isnan(got[:, dim])), dim
    assert np.all(np.isfinite(got[:4, 1])) and np.all(np.isnan(got[4:, 1]))   # an infinity spoils the mean only
    if S % 2:   # a NaN in the draw an odd S leaves out does not count
        x[S - 1, 0, 0] = np.nan
        assert same_bits(device_call(comp, x), want)


def test_refusals(comp):
    x, _ = trace(8, 1, 1)
    xd = torch.tensor(x, device="cuda")
    out = torch.zeros((6, 1), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    f, X, OUT, h = comp.L.exmc_hip_convergence, xd.data_ptr(), out.data_ptr(), comp.h
    assert f(h, X, 8, 1, 1, 0, OUT) == _lib.OK
    bad = [(None, X, 8, 1, 1, 0, OUT), (h, None, 8, 1, 1, 0, OUT), (h, X, 8, 1, 1, 0, None), (h, X, 7, 1, 1, 0, OUT),
           (h, X, 8, 0, 1, 0, OUT), (h, X, 8, 1, 0, 0, OUT), (h, X, -8, 1, 1, 0, OUT),
           (h, X, 1 << 21, 1, 1 << 11, 0, OUT),      # N = 2^32
           (h, X, 1 << 20, 1, 1 << 11, 0, OUT)]      # N = 2^31, one above the largest
    for args in bad:
        assert f(*args) == _lib.ERR_BADARG, args[2:6]
    host, o = np.zeros((1, 8, 1)), np.zeros((6, 1))
    g, H, O = comp.L.exmc_hip_convergence_host, host.ctypes.data_as(DP), o.ctypes.data_as(DP)
    assert g(h, H, 8, 1, 1, 0, O) == _lib.OK
    for args in [(None, H, 8, 1, 1, 0, O), (h, None, 8, 1, 1, 0, O), (h, H, 8, 1, 1, 0, None), (h, H, 7, 1, 1, 0, O),
                 (h, H, 8, 0, 1, 0, O), (h, H, 8, 1, 0, 0, O), (h, H, 1 << 21, 1, 1 << 11, 0, O)]:
        assert g(*args) == _lib.ERR_BADARG, args[2:6]
    assert b"convergence" in comp.L.exmc_hip_last_error()


def test_a_generated_models_library_has_it(comp):
    from exmc_amd import codegen
    gen = sampler.compile(codegen.compile_ir(codegen.eight_schools_ir()))
    try:
        assert gen.L is not comp.L
        for name in _lib.CONVERGENCE_EXPORTS:
            getattr(gen.L, name)
        x, want = trace(101, 3, 5)          # model-free: the trace's d, not the model's
        got = device_call(gen, x)
        assert same_bits(got, want), report(got, want)
        rows = diagnostics.convergence(gen, torch.tensor(x, device="cuda"))
        assert same_bits(rows["ess_tail"], want[3])
    finally:
        gen.close()
