// exmc_gen_pointwise.hpp -- the per-datum log-likelihood terms of a generated model over a device trace
// (exmc_amd/codegen.py generate(pointwise=True); C ABI include/exmc_hip_pointwise.h; DESIGN.md "Model
// comparison", per-datum terms of generated models).
//
// One lane owns one sample k = s C + c of the trace [S][d][C], chain fastest: its loads of the position
// and its stores ll[s][i - i0][c] are then coalesced over chains. (exmc_ic.hpp assigns a lane to a DATUM:
// the kinds' terms are one text for all datums; here every datum has a text of its own, so the lanes of a
// wavefront run the same datum at 64 samples.) The terms are the generated functions exmc_gen_pw_* over
// the folded constants of the handle's image, general exmc_detmath.h arithmetic, no contraction: the same
// text compiled for the host is the checker.
#pragma once

#include "exmc_models.hpp"

#ifdef EXMC_GEN_POINTWISE
namespace exmc {

constexpr int kGenPwBlock = 256;

struct GenPwParams {
  const double* c;      // dev [EXMC_GEN_PW_NCONST]: exmc_gen_pw_fold of the model's data
  const double* draws;  // dev [S][d][C]
  double* ll;           // dev [S][nb][C]
  int S, C;
  int i0, nb;           // the datums [i0, i0 + nb)
};

// kN = EXMC_GEN_PW_N, the model's datums: the kernel is a template like the other model-dependent kernels
// of a plug-in (exmc_plugin_kernels.inc instantiates it in a part of its own), and a block of datums that
// is not inside [0, kN) writes nothing. A function of the generated text that meets [i0, i0 + nb) computes
// all its datums and stores those inside: one datum per block costs the arithmetic of its group.
template <int kN>
__global__ void __launch_bounds__(kGenPwBlock) gen_pointwise_kernel(GenPwParams P) {
  const long long n = (long long)P.S * P.C;
  const long long k = (long long)blockIdx.x * kGenPwBlock + threadIdx.x;
  if (k >= n) return;   // the ragged last wavefront
  if (P.i0 < 0 || P.nb < 1 || P.nb > kN - P.i0) return;
  const long long s = k / P.C;
  const int c = (int)(k - s * P.C);
  const size_t C = (size_t)P.C;
  const double* qp = P.draws + (size_t)s * EXMC_GEN_D * C + c;
  double* op = P.ll + (size_t)s * P.nb * C + c;
  exmc_gen_pw_eval(P.c, P.i0, P.i0 + P.nb, qp, C, op, C);
}

}  // namespace exmc
#endif
