"""exmc_hip_ppc reduces exactly the replicates exmc_hip_posterior_predictive draws: the two kernels share
their walk over the trace (pp_seed, pp_stage and the LDS carve-up of exmc_amd/csrc/exmc_predictive.hpp), and
this holds them to it on the device alone. The replicates yrep [S][N][C] come from the device's
posterior_predictive at the same seed and chain_lo, the statement of the reductions
(tests/ppc_statement.py) is applied to them, and the raw outputs of exmc_hip_ppc and the finished numbers
of exmc_amd.predictive.ppc equal the result byte for byte.

The shapes are the smallest at which the shared walk can go wrong: 65 chains (the second workgroup has one
live lane and one tile row), 2 draws (the accumulators of the second are reloaded); eight_schools has one
partial group of datums, sv two groups with the second partial and 102 dimensions, where ppc_kernel's LDS
(ppc_lds_bytes(102) = 94720 bytes) is above 64 KB and predictive_kernel's (pp_lds_bytes(102) = 61440) is
not; chain_lo = 3 moves the seeds of both kernels alike."""
import numpy as np
import pytest
import torch

import ppc_statement as PPC
import predictive_inputs as PI
import test_gpu_ppc as TPPC
import test_gpu_predictive as TP
from exmc_amd import models
from exmc_amd import predictive as PP

pytestmark = pytest.mark.gpu

CASES = [(models.EIGHT_SCHOOLS, 10, 8, 65, 2, 0), (models.SV, 102, 100, 65, 2, 0), (models.EIGHT_SCHOOLS, 10, 8, 65, 2, 3)]


@pytest.mark.parametrize("kind,d,N,Cn,S,chain_lo", CASES)
def test_ppc_reduces_the_replicates_predictive_draws(kind, d, N, Cn, S, chain_lo, hip):
    seed = 23
    x = PI.draws(kind, S, Cn)
    assert x.shape == (S, d, Cn)
    cm = TP.comp(kind)
    xd = torch.from_numpy(x).cuda()
    yrep, names = PP.posterior_predictive(cm, xd, seed=seed, chain_lo=chain_lo)
    yrep = yrep.cpu().numpy()
    assert yrep.shape == (S, N, Cn) and np.isfinite(yrep).all()
    want = PPC.run(yrep, TPPC.observed(kind))
    assert want["sums"].shape == (2, N, 2)

    raw = TPPC.device_call(cm, x, seed, chain_lo)
    TPPC.assert_raw_equal(raw, want)             # sums, counts, chain_counts, tstat, t_obs
    assert raw["m0"] == want["m0"]

    py = PP.ppc(cm, xd, seed=seed, chain_lo=chain_lo, tstat=True)
    assert py["names"] == names
    assert py["tstat"].cpu().numpy().tobytes() == want["tstat"].tobytes()
    for k in ("mean", "var", "p_lt", "p_eq", "pit"):
        assert py[k].tobytes() == want[k].tobytes(), k
    assert np.array([py["t_obs"][k] for k in PP.PPC_STATS]).tobytes() == want["t_obs"].tobytes()
    assert np.array([py["p_value"][k] for k in PP.PPC_STATS]).tobytes() == want["p_value"].tobytes()
    if chain_lo:   # the offset reaches the replicates: another chain_lo, other sums
        other = TPPC.device_call(cm, x, seed, 0)
        assert other["sums"].tobytes() != raw["sums"].tobytes()
