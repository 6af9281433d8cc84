// exmc_common.hip — the model-free unit of every library: the entry points of include/exmc_hip.h
// that name no model type, with their kernels. The native-tree seam (exmc_native_tree.hpp), the
// fused-chain hook and the diagnostics launches behind exmc_hip_ess / _ess_bulk / _rhat
// (exmc_diag.hpp) and exmc_hip_convergence (exmc_convergence.hpp), exmc_hip_last_error,
// exmc_hip_device_count. Built once to exmc_common.o and linked
// into libexmc_hip.so (exmc_amd/build.py) and every plug-in (codegen.py build_plugin) next to that
// library's exmc_hip.hip. It never sees the model handle, whose layout differs between plug-ins.
#include "exmc_host.hpp"

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

#include "exmc_convergence.hpp"
#include "exmc_diag.hpp"
#include "exmc_native_tree.hpp"

using namespace exmc;
using namespace exmc::host;

namespace {
thread_local std::string g_last_error;   // the one last-error string of the library
}  // namespace

namespace exmc {
namespace host __attribute__((visibility("hidden"))) {

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int select_device(int device) {
  const int ndev = exmc_hip_device_count();
  if (ndev <= 0)
    return fail(EXMC_ERR_NO_DEVICE, "no HIP device visible: libexmc_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(EXMC_ERR_BADARG, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  return EXMC_OK;
}

// one lane per series up to lag 15, then a wavefront per unfinished series (ess_tail_kernel needs
// the series in LDS; longer ones stay with their lane to the end)
int launch_ess(hipStream_t stream, DevBuf& work, const double* src, int n_draws, int d, int n_chains,
               double* ess_dev) {
  const size_t series = (size_t)d * n_chains;
  const dim3 grid((unsigned)((series + kEssBlock - 1) / kEssBlock));
  const size_t lds = (size_t)n_draws * 8;
  if (lds > 160 * 1024) {
    hipLaunchKernelGGL(ess_series_kernel, grid, dim3(kEssBlock), 0, stream, src, n_draws, d, n_chains,
                       ess_dev, (int*)nullptr, (EssTailItem*)nullptr);
    HIP_TRY(hipGetLastError());
    return EXMC_OK;
  }
  int rc = work.ensure(16 + series * sizeof(EssTailItem));
  if (rc) return rc;
  int* count = (int*)work.p;
  EssTailItem* items = (EssTailItem*)((char*)work.p + 16);
  HIP_TRY(hipMemsetAsync(count, 0, 16, stream));
  hipLaunchKernelGGL(ess_series_kernel, grid, dim3(kEssBlock), 0, stream, src, n_draws, d, n_chains,
                     ess_dev, count, items);
  HIP_TRY(hipGetLastError());
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)ess_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  const unsigned tail_blocks = (unsigned)(series < 2048 ? series : 2048);
  hipLaunchKernelGGL(ess_tail_kernel, dim3(tail_blocks), dim3(64), lds, stream, src, n_draws, d,
                     n_chains, ess_dev, (const int*)count, (const EssTailItem*)items);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

int rank_scores_lds(int n_draws) {
  if ((size_t)n_draws * 8 > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)rank_scores_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, n_draws * 8));
  return EXMC_OK;
}

int launch_rank_scores(hipStream_t stream, const double* draws, int n_draws, int d, int n_chains,
                       double* scores) {
  const size_t series = (size_t)d * n_chains, lds = (size_t)n_draws * 8;
  int P = 2;
  while (P < n_draws) P <<= 1;
  const char* re = std::getenv("EXMC_HIP_RANK_SORT");   // 0: the counting kernel (A/B runs, tests)
  if (P <= kRankSortMaxP && !(re && re[0] == '0')) {
    // ranks by sorting the series in LDS (exmc_diag.hpp rank_scores_sort_kernel)
    hipLaunchKernelGGL(rank_scores_sort_kernel, dim3((unsigned)series), dim3(256), (size_t)P * 12, stream,
                       draws, n_draws, P, d, n_chains, scores);
  } else {
    hipLaunchKernelGGL(rank_scores_kernel, dim3((unsigned)series), dim3(256), lds, stream,
                       draws, n_draws, d, n_chains, scores);
  }
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

int launch_rhat(hipStream_t stream, const double* draws, int n_draws, int d, int n_chains, double* stats,
                double* rhat_dev) {
  const unsigned slices = (unsigned)((2 * n_chains + 255) / 256);
  hipLaunchKernelGGL(rhat_kernel, dim3((unsigned)d, slices), dim3(256), 0, stream, draws, n_draws, d,
                     n_chains, stats, rhat_dev, 0);
  hipLaunchKernelGGL(rhat_kernel, dim3((unsigned)d), dim3(64), 0, stream, draws, n_draws, d, n_chains,
                     stats, rhat_dev, 1);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

}  // namespace host
}  // namespace exmc

// exmc_hip_convergence (include/exmc_hip_convergence.h): the dimensions in blocks whose working set
// fits `scratch_bytes`, every block through the kernels of exmc_convergence.hpp in order. The scratch
// lives for the call: the stream has drained before it is freed.
namespace {

struct ConvCarver {
  char* base;
  size_t used = 0;
  template <class T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + used) : nullptr;
    used += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

// the arrays of a block of nb dimensions, carved from `base` (null: only the size is wanted)
size_t conv_carve(ConvBlk& g, char* base) {
  ConvCarver c{base};
  const size_t nb = (size_t)g.nb;
  g.keys = c.take<double>(nb * g.P);
  g.idx = c.take<unsigned>(nb * g.P);
  g.z = c.take<double>(nb * g.N);
  g.zf = c.take<double>(nb * g.N);
  g.tile_first = c.take<int>(nb * g.n_tiles);
  g.tile_last = c.take<int>(nb * g.n_tiles);
  g.carry_start = c.take<int>(nb * g.n_tiles);
  g.carry_end = c.take<int>(nb * g.n_tiles);
  g.qs = c.take<double>(nb * 3);
  g.nanpart = c.take<int>(nb * kConvNanSlices);
  g.mom = c.take<double>(nb * kConvSeries * 2 * g.M);
  g.acov = c.take<double>(nb * kConvEss * g.M * kConvLags);
  g.state = c.take<ConvState>(nb * kConvEss);
  return c.used;
}

// the pooled order of every dimension of the block, then the scores of its ranks into `scores`
int conv_rank(hipStream_t stream, const ConvBlk& g, int fold, double* scores) {
  const unsigned nb = (unsigned)g.nb;
  hipLaunchKernelGGL(pooled_ess_fill_kernel, dim3((g.P + kConvBlock - 1) / kConvBlock, nb), dim3(kConvBlock), 0, stream, g,
                     fold);
  const unsigned T = g.P < (unsigned)kConvTile ? g.P : (unsigned)kConvTile;
  const size_t lds = (size_t)T * 12;
  hipLaunchKernelGGL(pooled_ess_sort_local_kernel, dim3(g.P / T, nb), dim3(kConvBlock), lds, stream, g, T, 2ull,
                     (unsigned long long)T);
  for (unsigned long long k = 2ull * T; k <= g.P; k <<= 1) {   // only above one tile: the device-wide sort
    for (unsigned j = (unsigned)(k >> 1); j >= T; j >>= 1)
      hipLaunchKernelGGL(pooled_ess_sort_global_kernel, dim3((g.P / 2 + kConvBlock - 1) / kConvBlock, nb), dim3(kConvBlock),
                         0, stream, g, k, j);
    hipLaunchKernelGGL(pooled_ess_sort_local_kernel, dim3(g.P / T, nb), dim3(kConvBlock), lds, stream, g, T, k, k);
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(pooled_ess_runs_kernel, dim3((unsigned)g.n_tiles, nb), dim3(kConvBlock), 0, stream, g, 0,
                     (double*)nullptr);
  hipLaunchKernelGGL(pooled_ess_carry_kernel, dim3((nb + 63) / 64), dim3(64), 0, stream, g);
  hipLaunchKernelGGL(pooled_ess_runs_kernel, dim3((unsigned)g.n_tiles, nb), dim3(kConvBlock), 0, stream, g, 1, scores);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

}  // namespace

namespace exmc {
namespace host __attribute__((visibility("hidden"))) {

int launch_convergence(hipStream_t stream, hipEvent_t start, const double* draws, int n_draws, int d,
                       int n_chains, size_t scratch_bytes, double* out_dev) {
  ConvBlk g{};
  g.draws = draws;
  g.D = d;
  g.C = n_chains;
  g.n = n_draws / 2;
  g.M = 2 * n_chains;
  g.N = g.M * g.n;   // the caller has checked that it fits
  g.P = 2;
  while (g.P < (unsigned)g.N) g.P <<= 1;
  g.n_tiles = (int)(((long long)g.N + kConvRunTile - 1) / kConvRunTile);
  g.nb = 1;
  const size_t per_dim = conv_carve(g, nullptr);
  size_t nb = scratch_bytes / per_dim;
  nb = nb < 1 ? 1 : (nb > (size_t)d ? (size_t)d : nb);
  if (nb > 32768) nb = 32768;   // a block's dimensions are a grid's y
  g.nb = (int)nb;
  CallBuf buf;
  int rc = buf.alloc(conv_carve(g, nullptr));
  if (rc) return rc;
  HIP_TRY(hipEventRecord(start, stream));   // the caller's timing covers the launches, not the allocation
  const int nb_full = g.nb;
  for (int dim0 = 0; dim0 < d && !rc; dim0 += nb_full) {
    g.dim0 = dim0;
    g.nb = (d - dim0 < nb_full) ? (d - dim0) : nb_full;
    conv_carve(g, (char*)buf.p);   // a shorter last block is carved more tightly, inside the same buffer
    const unsigned ub = (unsigned)g.nb;
    HIP_TRY(hipMemsetAsync(g.state, 0, (size_t)g.nb * kConvEss * sizeof(ConvState), stream));
    hipLaunchKernelGGL(pooled_ess_nan_kernel, dim3(kConvNanSlices, ub), dim3(kConvBlock), 0, stream, g);
    rc = conv_rank(stream, g, 0, g.z);
    if (rc) break;
    hipLaunchKernelGGL(pooled_ess_quantile_kernel, dim3((ub + 63) / 64), dim3(64), 0, stream, g);
    rc = conv_rank(stream, g, 1, g.zf);
    if (rc) break;
    hipLaunchKernelGGL(pooled_ess_moments_kernel, dim3((unsigned)((g.M + kConvBlock - 1) / kConvBlock), ub, kConvSeries),
                       dim3(kConvBlock), 0, stream, g);
    // every block of lags is launched; a (dimension, series) that has met its cut leaves at once. The
    // last block holds the pair at which `2 j + 1 <= n - 1` fails, so every series ends.
    for (int l0 = 0; l0 <= g.n; l0 += kConvLags) {
      hipLaunchKernelGGL(pooled_ess_acov_kernel, dim3((unsigned)((g.M + 63) / 64), ub, kConvEss), dim3(64), 0, stream, g, l0);
      hipLaunchKernelGGL(pooled_ess_decide_kernel, dim3(ub * kConvEss), dim3(64), 0, stream, g, l0);
    }
    hipLaunchKernelGGL(pooled_ess_finish_kernel, dim3((ub + 63) / 64), dim3(64), 0, stream, g, out_dev);
    if (hipGetLastError() != hipSuccess) rc = fail(EXMC_ERR_HIP, "convergence: a launch failed");
  }
  const hipError_t e = hipStreamSynchronize(stream);   // before the scratch goes
  if (!rc && e != hipSuccess) rc = fail(EXMC_ERR_HIP, std::string("convergence: ") + hipGetErrorString(e));
  return rc;
}

}  // namespace host
}  // namespace exmc

extern "C" {

const char* exmc_hip_last_error(void) { return g_last_error.c_str(); }

int exmc_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// The NIF's incremental trajectory interface, batched (include/exmc_hip.h; kernels in
// exmc_native_tree.hpp). Blocking calls on the null stream: the interface is a compatibility
// seam (one call per doubling), not a throughput path.
// ------------------------------------------------------------------------------------------
struct exmc_hip_traj {
  int device = 0, C = 0, d = 0;
  DevBuf state;
  TrajDev T{};
};

namespace {

// carve a TrajDev out of one allocation: 9 vectors [C][d], 3 scalars [C], 4 int32 [C]
size_t traj_bytes(int C, int d) { return ((size_t)9 * C * d + 3 * (size_t)C) * 8 + 4 * (size_t)C * 4; }
TrajDev traj_view(void* base, int C, int d) {
  TrajDev t;
  double* b = (double*)base;
  const size_t v = (size_t)C * d;
  t.qL = b; t.pL = b + v; t.gL = b + 2 * v; t.qR = b + 3 * v; t.pR = b + 4 * v; t.gR = b + 5 * v;
  t.qP = b + 6 * v; t.gP = b + 7 * v; t.rho = b + 8 * v;
  b += 9 * v;
  t.logpP = b; t.lsw = b + C; t.acc = b + 2 * (size_t)C;
  int32_t* ib = (int32_t*)(b + 3 * (size_t)C);
  t.n = ib; t.depth = ib + C; t.div = ib + 2 * (size_t)C; t.turn = ib + 3 * (size_t)C;
  return t;
}


// uploads of one subtree call: the four state arrays, inv_mass and the per-chain scalars
struct SubtreeUpload {
  DevBuf buf;
  SubtreeParams P{};
  int fill(int C, int d, const double* all_q, const double* all_p, const double* all_logp,
           const double* all_g, int n_states, const double* inv_mass, const double* jlp0,
           const int32_t* depth, const int32_t* go_right, const uint64_t* seeds) {
    if (C < 1 || d < 1 || n_states < 1 || !all_q || !all_p || !all_logp || !all_g || !inv_mass ||
        !jlp0 || !depth || !go_right || !seeds)
      return fail(EXMC_ERR_BADARG, "bad arguments");
    for (int c = 0; c < C; c++)
      if (depth[c] >= kFtLevels || (depth[c] >= 0 && ((size_t)1 << depth[c]) > (size_t)n_states))
        return fail(EXMC_ERR_BADARG, "depth needs more pre-computed states than were passed");
    const size_t st = (size_t)C * n_states * d, sc = (size_t)C * n_states;
    const size_t nd = 3 * st + sc + d + C /*jlp0*/ + C /*seeds*/ + (size_t)C * (kFtLevels + 2) * d;
    int rc = buf.ensure(nd * 8 + 2 * (size_t)C * 4);
    if (rc) return rc;
    double* b = buf.as<double>();
    auto up = [&](const void* src, size_t n_doubles) -> const double* {
      double* dst = b;
      if (hipMemcpy(dst, src, n_doubles * 8, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
      b += n_doubles;
      return dst;
    };
    P.n_chains = C; P.d = d; P.n_states = n_states;
    P.all_q = up(all_q, st); P.all_p = up(all_p, st); P.all_g = up(all_g, st);
    P.all_logp = up(all_logp, sc);
    P.inv_mass = up(inv_mass, d); P.jlp0 = up(jlp0, C);
    P.seeds = (const uint64_t*)up(seeds, C);
    P.scratch = b; b += (size_t)C * (kFtLevels + 2) * d;
    int32_t* ib = (int32_t*)b;
    if (!P.all_q || !P.all_p || !P.all_g || !P.all_logp || !P.inv_mass || !P.jlp0 || !P.seeds ||
        hipMemcpy(ib, depth, (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(ib + C, go_right, (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess)
      return fail(EXMC_ERR_HIP, "upload failed");
    P.depth = ib; P.go_right = ib + C;
    return EXMC_OK;
  }
};

// scratch of exmc_hip_leapfrog_chain_normal_host (see there), one per device, never freed
struct ChainScratch {
  std::mutex mu;
  void* dev = nullptr;
  void* host = nullptr;
};
constexpr size_t kChainScratchBytes = (size_t)8 << 20;
constexpr int kChainScratchDevices = 16;
constexpr size_t kChainZeroCopyBytes = (size_t)1 << 20;   // rows the kernel writes straight into the staging buffer
ChainScratch g_chain_scratch[kChainScratchDevices];

int down(void* dst, const void* src, size_t bytes) {
  if (!dst) return EXMC_OK;
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return EXMC_OK;
}

}  // namespace

extern "C" {

int exmc_hip_traj_create(int device, int C, int d, const double* q, const double* p,
                         const double* grad, const double* logp, exmc_hip_traj** out) {
  if (!out || C < 1 || d < 1 || !q || !p || !grad || !logp) return fail(EXMC_ERR_BADARG, "bad arguments");
  *out = nullptr;
  int rc = select_device(device);
  if (rc) return rc;
  exmc_hip_traj* t = new exmc_hip_traj();
  t->device = device; t->C = C; t->d = d;
  rc = t->state.ensure(traj_bytes(C, d));
  if (rc) { delete t; return rc; }
  t->T = traj_view(t->state.p, C, d);
  const size_t v = (size_t)C * d * 8;
  hipError_t e = hipMemset(t->state.p, 0, traj_bytes(C, d));   // lsw, acc, n, depth, div, turn = 0
  // Trajectory::new (types.rs:136-152): both endpoints and the proposal are the start state, rho = p
  const double* src[9] = {q, p, grad, q, p, grad, q, grad, p};
  double* dst[9] = {t->T.qL, t->T.pL, t->T.gL, t->T.qR, t->T.pR, t->T.gR, t->T.qP, t->T.gP, t->T.rho};
  for (int i = 0; i < 9 && e == hipSuccess; i++) e = hipMemcpy(dst[i], src[i], v, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(t->T.logpP, logp, (size_t)C * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    t->state.release();
    delete t;
    return fail(EXMC_ERR_HIP, std::string("traj_create: ") + hipGetErrorString(e));
  }
  *out = t;
  return EXMC_OK;
}

void exmc_hip_traj_destroy(exmc_hip_traj* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  t->state.release();
  delete t;
}

int exmc_hip_traj_get_endpoint_host(exmc_hip_traj* t, const int32_t* go_right, double* q, double* p,
                                    double* grad) {
  if (!t || !go_right || !q || !p || !grad) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(t->device));
  const size_t row = (size_t)t->d * 8;
  for (int c = 0; c < t->C; c++) {
    const size_t o = (size_t)c * t->d;
    const bool r = go_right[c] != 0;
    HIP_TRY(hipMemcpy(q + o, (r ? t->T.qR : t->T.qL) + o, row, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(p + o, (r ? t->T.pR : t->T.pL) + o, row, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(grad + o, (r ? t->T.gR : t->T.gL) + o, row, hipMemcpyDeviceToHost));
  }
  return EXMC_OK;
}

int exmc_hip_traj_build_and_merge_host(exmc_hip_traj* t, const double* all_q, const double* all_p,
                                       const double* all_logp, const double* all_grad,
                                       int n_states, const double* inv_mass, const double* jlp0,
                                       const int32_t* depth, const int32_t* go_right,
                                       const uint64_t* seeds) {
  if (!t) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(t->device));
  SubtreeUpload u;
  int rc = u.fill(t->C, t->d, all_q, all_p, all_logp, all_grad, n_states, inv_mass, jlp0, depth,
                  go_right, seeds);
  if (rc == EXMC_OK) {
    u.P.T = t->T;
    hipLaunchKernelGGL(traj_build_and_merge_kernel, dim3((unsigned)((t->C + 63) / 64)), dim3(64), 0,
                       0, u.P);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = fail(EXMC_ERR_HIP, std::string("build_and_merge: ") + hipGetErrorString(e));
  }
  u.buf.release();
  return rc;
}

int exmc_hip_traj_is_terminated_host(exmc_hip_traj* t, int32_t* out) {
  if (!t || !out) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(t->device));
  std::vector<int32_t> dv(t->C), tn(t->C);
  HIP_TRY(hipMemcpy(dv.data(), t->T.div, (size_t)t->C * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tn.data(), t->T.turn, (size_t)t->C * 4, hipMemcpyDeviceToHost));
  for (int c = 0; c < t->C; c++) out[c] = (dv[c] || tn[c]) ? 1 : 0;   // types.rs:160-162
  return EXMC_OK;
}

int exmc_hip_traj_get_result_host(exmc_hip_traj* t, double* q, double* logp, double* grad,
                                  int32_t* n_steps, int32_t* divergent, double* accept_sum,
                                  int32_t* depth) {
  if (!t) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(t->device));
  const size_t v = (size_t)t->C * t->d * 8, s8 = (size_t)t->C * 8, s4 = (size_t)t->C * 4;
  int rc = down(q, t->T.qP, v);
  if (!rc) rc = down(grad, t->T.gP, v);
  if (!rc) rc = down(logp, t->T.logpP, s8);
  if (!rc) rc = down(accept_sum, t->T.acc, s8);
  if (!rc) rc = down(n_steps, t->T.n, s4);
  if (!rc) rc = down(divergent, t->T.div, s4);
  if (!rc) rc = down(depth, t->T.depth, s4);
  return rc;
}

int exmc_hip_build_subtree_host(int device, int C, int d, const double* all_q, const double* all_p,
                                const double* all_logp, const double* all_grad, int n_states,
                                const double* inv_mass, const double* jlp0, const int32_t* depth,
                                const int32_t* going_right, const uint64_t* seeds, double* q_left,
                                double* p_left, double* grad_left, double* q_right, double* p_right,
                                double* grad_right, double* q_prop, double* logp_prop,
                                double* grad_prop, double* log_sum_weight, int32_t* n_steps,
                                int32_t* divergent, double* accept_sum, int32_t* turning,
                                int32_t* subtree_depth, double* rho) {
  int rc = select_device(device);
  if (rc) return rc;
  SubtreeUpload u;
  rc = u.fill(C, d, all_q, all_p, all_logp, all_grad, n_states, inv_mass, jlp0, depth, going_right,
              seeds);
  DevBuf outb;
  if (rc == EXMC_OK) rc = outb.ensure(traj_bytes(C, d));
  if (rc == EXMC_OK) {
    u.P.out = traj_view(outb.p, C, d);
    hipError_t e = hipMemset(outb.p, 0, traj_bytes(C, d));
    if (e == hipSuccess) {
      hipLaunchKernelGGL(build_subtree_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, 0, u.P);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = fail(EXMC_ERR_HIP, std::string("build_subtree: ") + hipGetErrorString(e));
  }
  if (rc == EXMC_OK) {
    const TrajDev& o = u.P.out;
    const size_t v = (size_t)C * d * 8, s8 = (size_t)C * 8, s4 = (size_t)C * 4;
    const std::pair<void*, const void*> vec[9] = {{q_left, o.qL}, {p_left, o.pL}, {grad_left, o.gL},
                                                  {q_right, o.qR}, {p_right, o.pR}, {grad_right, o.gR},
                                                  {q_prop, o.qP}, {grad_prop, o.gP}, {rho, o.rho}};
    for (int i = 0; i < 9 && !rc; i++) rc = down(vec[i].first, vec[i].second, v);
    if (!rc) rc = down(logp_prop, o.logpP, s8);
    if (!rc) rc = down(log_sum_weight, o.lsw, s8);
    if (!rc) rc = down(accept_sum, o.acc, s8);
    if (!rc) rc = down(n_steps, o.n, s4);
    if (!rc) rc = down(divergent, o.div, s4);
    if (!rc) rc = down(turning, o.turn, s4);
    if (!rc) rc = down(subtree_depth, o.depth, s4);
  }
  u.buf.release();
  outb.release();
  return rc;
}

// B2' (tree.ex:613-653): see leapfrog_chain_normal_kernel. Blocking, on the null stream, like the other
// handle-less seams: the reference's hook uploads, dispatches and downloads per call as well. The hook exists
// to cut the cost of a DISPATCH (tree.ex:613-619), so a call of ordinary size pays for no allocation: a scratch
// per device (device buffer + page-locked staging, kChainScratchBytes each, made on first use and kept), ONE
// packed upload (q, p, inv_mass) and ONE packed download (the three row sets and logp) -- and up to 1 MB of rows no
// copy at all (the kernel works on the staging buffer itself). Calls on a device are
// serialised by its scratch's lock (they share the null stream anyway). Larger batches allocate and free.
int exmc_hip_leapfrog_chain_normal_host(int device, int C, int d, const double* q, const double* p,
                                        const double* inv_mass, int k, double signed_eps, double mu,
                                        double sigma, double* q_chain, double* p_chain,
                                        double* grad_chain, double* logp_chain) {
  if (C < 1 || d < 1 || d > kChainNormalMaxD || k < 0 || !q || !p || !inv_mass)
    return fail(EXMC_ERR_BADARG, "leapfrog_chain_normal: need n_chains >= 1, 1 <= d <= 256, k >= 0 and q, p, inv_mass");
  int rc = select_device(device);
  if (rc) return rc;
  if (k == 0) return EXMC_OK;
  const size_t vec = (size_t)C * d, rows = (size_t)C * k * d, lps = (size_t)C * k;
  const size_t n_in = 2 * vec + (size_t)d, n_out = 3 * rows + lps;
  const bool cached = (n_in + n_out) * 8 <= kChainScratchBytes && device < kChainScratchDevices;
  ChainScratch* sc = cached ? &g_chain_scratch[device] : nullptr;
  std::unique_lock<std::mutex> lock;
  DevBuf buf;
  double* dbase = nullptr;
  double* hbase = nullptr;
  if (sc) {
    lock = std::unique_lock<std::mutex>(sc->mu);
    if (!sc->dev) HIP_TRY(hipMalloc(&sc->dev, kChainScratchBytes));
    if (!sc->host) HIP_TRY(hipHostMalloc(&sc->host, kChainScratchBytes, hipHostMallocDefault));
    dbase = (double*)sc->dev;
    hbase = (double*)sc->host;
  } else {
    rc = buf.ensure((n_in + n_out) * 8);
    if (rc) return rc;
    dbase = (double*)buf.p;
  }
  ChainNormalParams P{};
  P.q = dbase; P.p = dbase + vec; P.inv_mass = dbase + 2 * vec;
  P.d = d; P.k = k; P.n_chains = C;
  P.eps = signed_eps; P.mu = mu; P.sigma = sigma;
  P.tiny32 = f32r(1.0e-30);
  P.log2pi32 = log2pi32();
  P.q_chain = dbase + n_in;
  P.p_chain = P.q_chain + rows;
  P.g_chain = P.p_chain + rows;
  P.logp_chain = P.g_chain + rows;
  hipError_t e;
  auto stage_in = [&] {
    std::memcpy(hbase, q, vec * 8);
    std::memcpy(hbase + vec, p, vec * 8);
    std::memcpy(hbase + 2 * vec, inv_mass, (size_t)d * 8);
  };
  auto copy_out = [&] {
    const double* o = hbase + n_in;
    if (q_chain) std::memcpy(q_chain, o, rows * 8);
    if (p_chain) std::memcpy(p_chain, o + rows, rows * 8);
    if (grad_chain) std::memcpy(grad_chain, o + 2 * rows, rows * 8);
    if (logp_chain) std::memcpy(logp_chain, o + 3 * rows, lps * 8);
    return EXMC_OK;
  };
  // a call of ordinary size (the reference's: one chain, K = 32) moves so little that the two copies cost more
  // than the kernel: it reads its inputs from, and writes its rows to, the page-locked staging directly (the
  // buffer is device-accessible; the kernel's end makes the rows visible to the host) -- no copy kernels at all
  const bool zero_copy = hbase && n_out * 8 <= kChainZeroCopyBytes;
  if (zero_copy) {
    stage_in();
    P.q = hbase; P.p = hbase + vec; P.inv_mass = hbase + 2 * vec;
    P.q_chain = hbase + n_in;
    P.p_chain = P.q_chain + rows;
    P.g_chain = P.p_chain + rows;
    P.logp_chain = P.g_chain + rows;
    hipLaunchKernelGGL(leapfrog_chain_normal_kernel, dim3((unsigned)C), dim3(64), 0, 0, P);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) return fail(EXMC_ERR_HIP, std::string("leapfrog_chain_normal: ") + hipGetErrorString(e));
    return copy_out();
  }
  if (hbase) {
    stage_in();
    e = hipMemcpy(dbase, hbase, n_in * 8, hipMemcpyHostToDevice);
  } else {
    e = hipMemcpy(dbase, q, vec * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dbase + vec, p, vec * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dbase + 2 * vec, inv_mass, (size_t)d * 8, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(leapfrog_chain_normal_kernel, dim3((unsigned)C), dim3(64), 0, 0, P);
    e = hipGetLastError();
  }
  if (hbase) {
    // the blocking copy waits for the kernel (same stream)
    if (e == hipSuccess) e = hipMemcpy(hbase + n_in, P.q_chain, n_out * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(EXMC_ERR_HIP, std::string("leapfrog_chain_normal: ") + hipGetErrorString(e));
    return copy_out();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) rc = fail(EXMC_ERR_HIP, std::string("leapfrog_chain_normal: ") + hipGetErrorString(e));
  if (!rc) rc = down(q_chain, P.q_chain, rows * 8);
  if (!rc) rc = down(p_chain, P.p_chain, rows * 8);
  if (!rc) rc = down(grad_chain, P.g_chain, rows * 8);
  if (!rc) rc = down(logp_chain, P.logp_chain, lps * 8);
  buf.release();
  return rc;
}

int exmc_hip_build_full_tree_host(int device, int C, int d, const double* q0, const double* p0,
                                  const double* g0, const double* logp0, const double* fwd_q,
                                  const double* fwd_p, const double* fwd_logp, const double* fwd_g,
                                  int n_fwd, const double* bwd_q, const double* bwd_p,
                                  const double* bwd_logp, const double* bwd_g, int n_bwd,
                                  const double* inv_mass, const double* jlp0, int max_depth,
                                  const uint64_t* seeds, double* q_out, double* logp_out,
                                  double* g_out, int32_t* n_steps, int32_t* divergent,
                                  double* accept_sum, int32_t* depth) {
  if (C < 1 || d < 1 || n_fwd < 0 || n_bwd < 0 || max_depth < 0 || max_depth > kFtLevels ||
      !q0 || !p0 || !g0 || !logp0 || !inv_mass || !jlp0 || !seeds || !q_out || !logp_out ||
      !g_out || !n_steps || !divergent || !accept_sum || !depth ||
      (n_fwd > 0 && (!fwd_q || !fwd_p || !fwd_logp || !fwd_g)) ||
      (n_bwd > 0 && (!bwd_q || !bwd_p || !bwd_logp || !bwd_g)))
    return fail(EXMC_ERR_BADARG, "bad arguments");   // NifResult badarg (lib.rs)
  int rc = select_device(device);
  if (rc) return rc;
  const size_t vec = (size_t)C * d, fw = (size_t)C * n_fwd * d, bw = (size_t)C * n_bwd * d;
  // one device arena: inputs, scratch, outputs (doubles), then int32 outputs
  const size_t n_in = 3 * vec + C + 3 * fw + (size_t)C * n_fwd + 3 * bw + (size_t)C * n_bwd + d + C + C;
  const size_t n_scr = (size_t)C * (kFtLevels + 3) * d;
  const size_t n_out = 2 * vec + 2 * (size_t)C;
  const size_t total = (n_in + n_scr + n_out) * 8 + 3 * (size_t)C * 4;
  DevBuf arena;
  rc = arena.ensure(total);
  if (rc) return rc;
  double* b = arena.as<double>();
  FullTreeParams P;
  P.n_chains = C; P.d = d; P.n_fwd = n_fwd; P.n_bwd = n_bwd; P.max_depth = max_depth;
  std::vector<std::pair<const void*, size_t>> ups;
  auto put = [&](const double* src, size_t n) {
    double* dst = b;
    if (n) ups.push_back({src, n});
    b += n;
    return (const double*)dst;
  };
  P.q0 = put(q0, vec); P.p0 = put(p0, vec); P.g0 = put(g0, vec); P.logp0 = put(logp0, C);
  P.fwd_q = put(fwd_q, fw); P.fwd_p = put(fwd_p, fw); P.fwd_g = put(fwd_g, fw);
  P.fwd_logp = put(fwd_logp, (size_t)C * n_fwd);
  P.bwd_q = put(bwd_q, bw); P.bwd_p = put(bwd_p, bw); P.bwd_g = put(bwd_g, bw);
  P.bwd_logp = put(bwd_logp, (size_t)C * n_bwd);
  P.inv_mass = put(inv_mass, d); P.jlp0 = put(jlp0, C);
  P.seeds = (const uint64_t*)put((const double*)seeds, C);
  {
    double* dst = arena.as<double>();
    for (auto& u : ups) {
      if (hipMemcpy(dst, u.first, u.second * 8, hipMemcpyHostToDevice) != hipSuccess) {
        arena.release();
        return fail(EXMC_ERR_HIP, "upload failed");
      }
      dst += u.second;
    }
  }
  P.scratch = b; b += n_scr;
  P.out_q = b; b += vec;
  P.out_g = b; b += vec;
  P.out_logp = b; b += C;
  P.out_accept_sum = b; b += C;
  int32_t* ib = (int32_t*)b;
  P.out_n_steps = ib; P.out_divergent = ib + C; P.out_depth = ib + 2 * (size_t)C;
  hipLaunchKernelGGL(full_tree_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, 0, P);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(q_out, P.out_q, vec * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(g_out, P.out_g, vec * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(logp_out, P.out_logp, (size_t)C * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(accept_sum, P.out_accept_sum, (size_t)C * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(n_steps, P.out_n_steps, (size_t)C * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(divergent, P.out_divergent, (size_t)C * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(depth, P.out_depth, (size_t)C * 4, hipMemcpyDeviceToHost);
  arena.release();
  if (e != hipSuccess) return fail(EXMC_ERR_HIP, std::string("build_full_tree: ") + hipGetErrorString(e));
  return EXMC_OK;
}

}  // extern "C"
