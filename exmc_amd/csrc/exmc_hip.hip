// exmc_hip.hip — the model-dependent half of the C ABI (include/exmc_hip.h): the handle, the layout
// dispatch, sampling, warmup, model comparison. The entry points that name no model type -- the
// native-tree seam, the fused-chain hook, the diagnostics launches, exmc_hip_last_error and
// exmc_hip_device_count -- and their kernels are exmc_common.hip, which every library links
// (exmc_host.hpp is the seam between the two). Every leapfrog, log-density, gradient, tree merge
// and U-turn test runs in the HIP kernels, and so does the warmup of lib/exmc/nuts/sampler.ex
// (window schedule, dual averaging, Welford mass matrix: warmup_kernel, exmc_nuts.hpp; the
// host-driven form behind EXMC_HIP_HOST_WARMUP=1 restates the adaptation in plain C++ here). There
// is no CPU fallback: without a HIP device every compute entry point returns EXMC_ERR_NO_DEVICE.
#include "../../include/exmc_hip.h"
#include "../../include/exmc_hip_compare.h"
#include "../../include/exmc_hip_pathfinder.h"
#include "../../include/exmc_hip_advi.h"
#include "../../include/exmc_hip_smc.h"
#include "../../include/exmc_hip_smc_bridge.h"
#include "../../include/exmc_hip_fit_psis.h"
#include "../../include/exmc_hip_predictive.h"
#include "../../include/exmc_hip_ppc.h"
#include "../../include/exmc_hip_loo_pit.h"
#include "../../include/exmc_hip_convergence.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/exmc_zig_tables.h"
#include "exmc_kernels.hpp"
#include "exmc_host.hpp"
#include "exmc_layout_host.hpp"
#include "exmc_ic.hpp"
#include "exmc_psis.hpp"
#include "exmc_psis_ratio.hpp"

using namespace exmc;
using namespace exmc::host;

#ifdef EXMC_PLUGIN_SPLIT
// a plug-in built in parts (exmc_plugin_part.hip): the four heavy kernels are compiled in translation
// units of their own, in parallel; here they are only declared
namespace exmc {
#include "exmc_plugin_kernels.inc"
}
#endif

namespace {

#if EXMC_PROFILE_SECTIONS
hipError_t print_sections(const char* what, double ms) {
  unsigned long long h[16], z[16] = {0};
  hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(g_prof), sizeof(h));
  if (e != hipSuccess) return e;
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof(z));
  if (e != hipSuccess) return e;
  static const char* nm[9] = {"transition_start", "doubling_start", "leapfrog+model", "leaf",
                              "ascend", "outer_merge", "transition_done", "tree_prefix", "loop"};
  unsigned long long tot = 0;
  for (int i = 0; i < 9; i++) tot += h[i];
  fprintf(stderr, "[exmc prof] %s %.3f ms, passes (sum over waves) %llu, cycles %llu\n", what, ms, h[9], tot);
  for (int i = 0; i < 9; i++)
    if ((i != 7 || h[7]) && h[9])   // tree_prefix: once per transition, outside the passes (M::kTreePrefix)
      fprintf(stderr, "[exmc prof]   %-18s %6.1f%%  %8.1f cycles/pass\n", nm[i],
              100.0 * (double)h[i] / (double)tot, (double)h[i] / (double)h[9]);
  if (h[10])
    fprintf(stderr, "[exmc prof]   integrator wave: %llu units, %.1f cycles/unit compute, %.1f barrier wait, %.1f other\n",
            h[10], (double)h[11] / (double)h[10], (double)h[12] / (double)h[10], (double)h[13] / (double)h[10]);
#if EXMC_PROFILE_SECTIONS >= 2
  // the marks inside "transition start" (= 2) or inside the trace sink (= 3): exmc_nuts.hpp g_prof_sub
  unsigned long long s[8], sz[8] = {0};
  e = hipMemcpyFromSymbol(s, HIP_SYMBOL(g_prof_sub), sizeof(s));
  if (e != hipSuccess) return e;
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_prof_sub), sz, sizeof(sz));
  if (e != hipSuccess) return e;
#if EXMC_PROFILE_SECTIONS == 2
  static const char* sn[5] = {"start: window draw", "start: long-way rounds", "start: stepping loop",
                              "start: momentum_from_variates", "start: mass_ke"};
  const int ns = 5;
#else
  static const char* sn[3] = {"done: draws store", "done: stat stores", "done: cursor steps"};
  const int ns = 3;
#endif
  for (int i = 0; i < ns; i++)
    if (h[9])
      fprintf(stderr, "[exmc prof]   %-30s %6.2f%%  %8.1f cycles/pass\n", sn[i],
              100.0 * (double)s[i] / (double)tot, (double)s[i] / (double)h[9]);
  if (EXMC_PROFILE_SECTIONS == 2)
    fprintf(stderr, "[exmc prof]   long-way rounds (sum over waves) %llu, wave-transitions %llu\n", s[5], s[6]);
#endif
  return hipSuccess;
}
#endif


const uint64_t kZigKi[256] = EXMC_ZIG_KI_INIT;
const double kZigWi[256] = EXMC_ZIG_WI_INIT;
const double kZigFi[256] = EXMC_ZIG_FI_INIT;


// ---- launching the model-dependent kernels --------------------------------------------------
// libexmc_hip.so and one-unit plug-ins: the kernel is an instantiation of this translation unit,
// launched through its host stub. A plug-in built in parts with -DEXMC_PLUGIN_MODULES (the default
// of exmc_amd/codegen.py build_plugin since round 4): the model-dependent kernels are compiled
// DEVICE-ONLY, one code object per part, embedded in the library as data (exmc_blob_table, written
// by the build next to this unit) and loaded with hipModuleLoadData on first use; a launch looks the
// kernel up by its device-side mangled name and goes through hipModuleLaunchKernel. No host pass is
// spent on the parts and no host stub exists for these kernels -- SURVEY section 8 row f3's "IR ->
// kernel via a run-time compiled code object", with hipcc's device pass in the role of hiprtc.
#ifdef EXMC_PLUGIN_MODULES
extern "C" const unsigned char* const exmc_blob_table[];   // start_0, end_0, start_1, end_1, ..., null
struct ModSet {
  int device = -1;
  std::vector<hipModule_t> mods;
  std::unordered_map<std::string, hipFunction_t> fns;
};
std::mutex g_mod_mu;
std::vector<ModSet*> g_modsets;

// the function `name` of this plug-in's code objects on `device` (the current device of the caller)
hipError_t mod_function(int device, const char* name, hipFunction_t* out) {
  std::lock_guard<std::mutex> lock(g_mod_mu);
  ModSet* ms = nullptr;
  for (ModSet* x : g_modsets)
    if (x->device == device) ms = x;
  if (!ms) {
    ms = new ModSet;
    ms->device = device;
    for (int i = 0; exmc_blob_table[2 * i] != nullptr; i++) {
      hipModule_t mod = nullptr;
      const hipError_t e = hipModuleLoadData(&mod, exmc_blob_table[2 * i]);
      if (e != hipSuccess) {
        for (hipModule_t m_ : ms->mods) (void)hipModuleUnload(m_);
        delete ms;
        return e;
      }
      ms->mods.push_back(mod);
    }
    g_modsets.push_back(ms);
  }
  auto it = ms->fns.find(name);
  if (it != ms->fns.end()) {
    *out = it->second;
    return hipSuccess;
  }
  // (a kernel lives in one of the code objects: the lookups in the others fail, and the runtime
  // remembers the last failure -- it is not the caller's error, whichever way the search ends)
  hipFunction_t found = nullptr;
  for (hipModule_t mod : ms->mods) {
    hipFunction_t f = nullptr;
    if (hipModuleGetFunction(&f, mod, name) == hipSuccess && f) {
      found = f;
      break;
    }
  }
  (void)hipGetLastError();
  if (!found) return hipErrorInvalidDeviceFunction;
  ms->fns.emplace(name, found);
  *out = found;
  return hipSuccess;
}

template <class... A>
hipError_t mod_launch(int device, const char* name, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                      A... args) {
  hipFunction_t f = nullptr;
  const hipError_t e = mod_function(device, name, &f);
  if (e != hipSuccess) return e;
  void* params[] = {(void*)&args...};
  return hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)lds, stream,
                               params, nullptr);
}
// (the kernel arguments are passed by value exactly as the kernel declares them: every call site
// hands over the parameter structs themselves)
#define EXMC_KLAUNCH(dev, kernel, grid, block, lds, stream, ...)   HIP_TRY(mod_launch((dev), __builtin_get_device_side_mangled_name kernel, (grid), (block), (lds), (stream), __VA_ARGS__))
// dynamic LDS above 64 KB needs no opt-in for a module function on this runtime; a launch that asks
// for more than the device has fails in hipModuleLaunchKernel
#define EXMC_KMAXLDS(kernel, bytes)   do {                                } while (0)
#else
#define EXMC_KLAUNCH(dev, kernel, grid, block, lds, stream, ...)   hipLaunchKernelGGL(kernel, (grid), (block), (lds), (stream), __VA_ARGS__)
#define EXMC_KMAXLDS(kernel, bytes)   HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)))
#endif

}  // namespace

struct exmc_hip_model {
  int kind = 0, d = 0, device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double last_ms = 0.0;
  EightSchoolsConsts es{};
  SimpleConsts sp{};
  SVConsts sv{};
  LogisticConsts lg{};
  RadonConsts rd{};
#ifdef EXMC_CUSTOM_HEADER
  CustomConsts cu{};
  const double* pw = nullptr;   // a model generated with per-datum terms: their folded constants in the image
#endif
  DevBuf data;      // model data kept in HBM (logistic X,y; radon u,starts,floor,y)
  DevBuf zig;       // ki[256] u64, wi[256], fi[256]
  DevBuf flat;      // perm[D], rank[D] (int32) when the kernel order is not the reference's flat order
  bool flat_set = false;
  DevBuf tuning;    // inv_mass[D], sqrt_inv_mass[D]
  DevBuf ms_mass;   // exmc_hip_multi_step's inv_mass[D]: the caller's, never the resident chains'
  DevBuf state;     // q[D][C], g[D][C], logp[C], rng[2][C]
  DevBuf stack;
  DevBuf misc;      // [0] eps_out, [1..2] counters (u64), [3] trace scratch word, [8..8+D) init_q
  DevBuf trace;     // staging for host-trace entry points
  DevBuf io;        // staging for host vectors
  DevBuf scores;    // ess_bulk: the rank-normalised copy of the caller's trace
  DevBuf dense;     // opts[:dense_mass]: cov[D][D], chol[D][D] while a dense mass is in force
  // lane layouts (LaneDenseModel): the same two matrices with their columns permuted to kernel
  // dimensions, [D][GD] each, built from the host copies for the lane count of the launch; the
  // warmup kernel's global workspace; rank of each kernel dimension in the flat vector
  DevBuf densep, densews;
  DevBuf migboard;  // chain migration board of the sampling kernel (exmc_nuts.hpp)
  // push-style stream: page-locked host memory [progress word | trace of the run in flight]
  void* pin_host = nullptr;
  size_t pin_bytes = 0;
  std::atomic<bool> stream_in_flight{false};
  int densep_gd = 0;
  std::vector<double> h_dense;
  std::vector<int32_t> h_rank;
  DevBuf esswork;   // ESS: [count | EssTailItem...] of the series that go on to ess_tail_kernel
  bool dense_on = false;
  int state_chains = 0;
  // resident chains (exmc_hip_chains_init / _advance, exmc_hip_stream_begin / _next / _start) and
  // the call that created them: only that owner's continuation calls advance them
  int res_C = 0, res_lanes = 0, res_max_depth = 10;
  int res_owner = 0;   // kResNone / kResChains / kResStream
  double res_eps = 0.0;
  int simds = 1024;   // 4 x the device's compute units (MI355X: 256 CUs)
};

namespace {

enum { kResNone = 0, kResChains = 1, kResStream = 2 };

ChainState state_view(exmc_hip_model* m, int C) {
  ChainState s;
  double* b = m->state.as<double>();
  s.q = b;
  s.g = b + (size_t)m->d * C;
  s.logp = b + (size_t)2 * m->d * C;
  s.rng = (uint64_t*)(b + (size_t)2 * m->d * C + C);
  return s;
}
size_t state_bytes(int d, int C) { return ((size_t)2 * d * C + (size_t)3 * C) * 8; }

int ensure_state(exmc_hip_model* m, int C) {
  m->res_C = 0;  // whoever re-lays-out the state buffer evicts the resident chains
  int rc = m->state.ensure(state_bytes(m->d, C));
  if (rc) return rc;
  m->state_chains = C;
  return EXMC_OK;
}

int upload_tuning(exmc_hip_model* m, const double* inv_mass) {
  std::vector<double> h(2 * (size_t)m->d);
  for (int i = 0; i < m->d; i++) {
    h[i] = inv_mass[i];
    h[m->d + i] = std::sqrt(inv_mass[i]);  // :math.sqrt(inv_m), sampler.ex:397
  }
  int rc = m->tuning.ensure(h.size() * 8);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(m->tuning.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return EXMC_OK;
}

// ---- model/lanes dispatch: the layouts of exmc_layouts.inc ------------------------------------
enum { kRoleSample = 1, kRoleWarmup = 2, kRoleDense = 4, kRoleStream = 8 };

template <class M_, int G_, int LDSL_, int kRoles = 0>
struct Tag {
  using M = M_;
  static constexpr int G = G_;
  static constexpr int LDSL = LDSL_;  // tree-stack levels kept in LDS by nuts_kernel
  static constexpr bool kStream = (kRoles & kRoleStream) != 0;   // stream-push and independent kernels
};

// LDS budget per one-wave workgroup: 4096 chains x G=16 lanes = 1024 workgroups = 4 per CU of
// 160 KB; sv at 2048 chains x 64 lanes = 8 per CU.
// kOneChain: the launches of the shared one-chain warmup (chain init, warmup kernels), which take
// the EXMC_ONE_CHAIN rows too
template <bool kOneChain = false, class F>
int dispatch(exmc_hip_model* m, int lanes, F&& f) {
#define EXMC_ONE_CHAIN(K, L, M, G, LDSL, mem, roles) \
  if constexpr (kOneChain) if (m->kind == K && lanes == L) return f(Tag<M, G, LDSL>{}, m->mem);
#define EXMC_LAYOUT(K, L, M, LDSL, mem, roles, ...) \
  if (m->kind == K && lanes == L) return f(Tag<M, L, LDSL, roles>{}, m->mem);
#include "exmc_layouts.inc"
  return fail(EXMC_ERR_UNSUPPORTED, "model kind / lanes_per_chain combination not compiled in");
}

// the layouts that carry a dense mass matrix: a whole chain in one lane, or a row with a dense model
bool dense_layout_ok(const exmc_hip_model* m, int lanes) {
  bool ok = lanes == 1;
#define EXMC_LAYOUT(K, L, M, LDSL, mem, roles, DL, ...) \
  ok = ok || (m->kind == K && lanes == L && !std::is_void_v<__VA_ARGS__>);
#include "exmc_layouts.inc"
  return ok;
}

// the kind's lanes for a role: those of its first row with the role, else 1
int role_lanes(int kind, int role) {
#define EXMC_ONE_CHAIN(K, L, M, G, LDSL, mem, roles) \
  if (kind == K && ((roles) & role)) return L;
#define EXMC_LAYOUT(K, L, M, LDSL, mem, roles, ...) \
  if (kind == K && ((roles) & role)) return L;
#include "exmc_layouts.inc"
  return 1;
}

// the sampling layout behind a one-chain form at `lanes`, else `lanes`
int sampling_lanes(int kind, int lanes) {
#define EXMC_ONE_CHAIN(K, L, M, G, LDSL, mem, roles) \
  if (kind == K && lanes == L) return G;
#define EXMC_LAYOUT(...)
#include "exmc_layouts.inc"
  return lanes;
}

// covp[s GD + i] = cov[rank(i)][s], cholp[j GD + i] = chol[j][rank(i)], zero columns past D
// (exmc_device.hpp LaneDense), for the GD = lanes x dimensions-per-lane of the launch
int ensure_densep(exmc_hip_model* m, int GD) {
  if (m->densep_gd == GD) return EXMC_OK;
  const int d = m->d;
  if (m->h_dense.size() != 2 * (size_t)d * d) return fail(EXMC_ERR_BADARG, "no dense mass is set");
  std::vector<double> h(2 * (size_t)d * GD, 0.0);
  const double* cov = m->h_dense.data();
  const double* chol = cov + (size_t)d * d;
  for (int s = 0; s < d; s++)
    for (int i = 0; i < d; i++) {
      const int r = m->h_rank.empty() ? i : m->h_rank[i];
      h[(size_t)s * GD + i] = cov[(size_t)r * d + s];
      h[(size_t)d * GD + (size_t)s * GD + i] = chol[(size_t)s * d + r];
    }
  int rc = m->densep.ensure(h.size() * 8);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(m->densep.p, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  m->densep_gd = GD;
  return EXMC_OK;
}

// dispatch for the launches whose mass-dependent operations depend on the dense mode
template <bool kOneChain = false, class F>
int dispatch_mass(exmc_hip_model* m, int lanes, bool dense, F&& f) {
#ifndef EXMC_DEV_ONLY   // kernel-work builds carry no dense variant
#define EXMC_LAYOUT(K, L, M, LDSL, mem, roles, DL, ...)                                 \
  if constexpr (!std::is_void_v<__VA_ARGS__>)                                          \
    if (dense && m->kind == K && lanes == L) return f(Tag<__VA_ARGS__, L, DL>{}, m->mem);
#include "exmc_layouts.inc"
#endif
  return dispatch<kOneChain>(m, lanes, f);
}

int default_lanes(int kind) { return role_lanes(kind, kRoleSample); }

int resolve_lanes(const exmc_hip_model* m, int lanes) { return lanes > 0 ? lanes : default_lanes(m->kind); }

dim3 grid_for(int n_chains, int lanes, int block) {
  size_t threads = (size_t)n_chains * lanes;
  return dim3((unsigned)((threads + block - 1) / block));
}

constexpr int kBlock = 64;

FlatOrder flat_order(exmc_hip_model* m) {
  FlatOrder f;
  if (m->flat_set) {
    f.perm = m->flat.as<int32_t>();
    f.rank = m->flat.as<int32_t>() + m->d;
  }
  return f;
}

// perm[r] = kernel dimension of flat entry r; identity clears the table
int set_flat_order(exmc_hip_model* m, const int32_t* perm) {
  const int d = m->d;
  std::vector<int32_t> h(2 * (size_t)d, -1);
  bool identity = true;
  for (int r = 0; r < d; r++) {
    if (perm[r] < 0 || perm[r] >= d || h[d + perm[r]] >= 0)
      return fail(EXMC_ERR_BADARG, "flat order is not a permutation of 0..d-1");
    h[r] = perm[r];
    h[d + perm[r]] = r;
    identity = identity && perm[r] == r;
  }
  m->h_rank.assign(h.begin() + d, h.end());
  m->densep_gd = 0;
  if (identity) {
    m->flat_set = false;
    return EXMC_OK;
  }
  int rc = m->flat.ensure(h.size() * 4);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(m->flat.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  m->flat_set = true;
  return EXMC_OK;
}

const uint64_t* zig_ki(exmc_hip_model* m) { return m->zig.as<uint64_t>(); }
const double* zig_wi(exmc_hip_model* m) { return m->zig.as<double>() + 256; }
const double* zig_fi(exmc_hip_model* m) { return m->zig.as<double>() + 512; }
RngArgs rng_args(exmc_hip_model* m) { return RngArgs{zig_ki(m), zig_wi(m), zig_fi(m), EXMC_NOR_R}; }

// one_chain: the start of the shared warmup (a generated lane layout may have its one-chain form)
int launch_init(exmc_hip_model* m, int lanes, int C, int chain_lo, uint64_t seed,
                const double* init_q_host, bool one_chain = false) {
  const double* init_dev = nullptr;
  if (init_q_host) {
    double* dst = m->misc.as<double>() + 8;
    HIP_TRY(hipMemcpyAsync(dst, init_q_host, (size_t)m->d * 8, hipMemcpyHostToDevice, m->stream));
    init_dev = dst;
  }
  InitParams P;
  P.st = state_view(m, C);
  P.n_chains = C;
  P.chain_lo = chain_lo;
  P.base_seed = seed;
  P.init_q = init_dev;
  P.zig_ki = zig_ki(m); P.zig_wi = zig_wi(m); P.zig_fi = zig_fi(m);
  P.nor_r = EXMC_NOR_R;
  P.flat = flat_order(m);
  auto launch = [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    const size_t xlds = aux_lds_bytes<typename T::M>();
    EXMC_KLAUNCH(m->device, (init_chains_kernel<typename T::M, T::G>), grid_for(C, T::G, kBlock),
                 dim3(kBlock), xlds, m->stream, P, mc);
    HIP_TRY(hipGetLastError());
    return (int)EXMC_OK;
  };
  return one_chain ? dispatch<true>(m, lanes, launch) : dispatch(m, lanes, launch);
}

// dense: run under the dense mass installed on the handle (m->dense) instead of m->tuning's diagonal
int launch_nuts(exmc_hip_model* m, bool dense, int lanes, int C, int n_draws, int draw_offset, double eps,
                int max_depth, TraceDev tr, bool timed, int* progress = nullptr) {
  if (max_depth < 1 || max_depth > kMaxLevels) return fail(EXMC_ERR_BADARG, "max_tree_depth out of range");
  return dispatch_mass(m, lanes, dense, [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    using M = typename T::M;
    dim3 grid = grid_for(C, T::G, kNutsBlock);
    size_t nthreads = (size_t)grid.x * kNutsBlock;
    constexpr int kSpill = (kMaxLevels > T::LDSL) ? (kMaxLevels - T::LDSL) : 1;
    int rc = m->stack.ensure((size_t)kSpill * nuts_nslot<M>() * nthreads * 8);
    if (rc) return rc;
    NutsParams P;
    P.st = state_view(m, C);
    P.n_chains = C;
    P.n_draws = n_draws;
    P.draw_offset = draw_offset;
    P.eps = eps;
    P.max_depth = max_depth;
    P.inv_mass = m->tuning.as<double>();
    P.sqrt_inv_mass = m->tuning.as<double>() + m->d;
    P.tr = tr;
    P.stack = m->stack.as<double>();
    P.counters = (unsigned long long*)(m->misc.as<double>() + 1);
    P.scratch = m->misc.as<double>() + 3;
    P.zig_ki = zig_ki(m); P.zig_wi = zig_wi(m); P.zig_fi = zig_fi(m);
    P.nor_r = EXMC_NOR_R;
    P.flat = flat_order(m);
    P.progress = progress;
    P.mig = nullptr;
    {
      const char* pe = std::getenv("EXMC_HIP_PRIO");   // 0: leave the arbiter's oldest-first order alone
      P.prio = (pe && pe[0] == '0') ? 0 : 1;
    }
    P.simds = m->simds;
    if (progress) {
      if constexpr (T::kStream) {
        if (timed) HIP_TRY(hipEventRecord(m->ev0, m->stream));
        const size_t lds_s = nuts_lds_bytes<M, T::LDSL, M::kNutsZigInLds>();
        EXMC_KLAUNCH(m->device, (nuts_kernel<M, T::G, T::LDSL, false, true>), grid, dim3(kNutsBlock), lds_s,
                     m->stream, P, mc);
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(m->ev1, m->stream));
        return (int)EXMC_OK;
      } else {
        return fail(EXMC_ERR_UNSUPPORTED, "a push-style stream runs in the model kind's default layout, diagonal mass");
      }
    }
    if constexpr (M::kMigrate) {
      // worth it when the launch puts two chains on a SIMD (more waves than the 1024 SIMDs) and
      // runs long enough to have a tail; EXMC_HIP_MIGRATE=0 / 1 forces it off / on
      const char* me = std::getenv("EXMC_HIP_MIGRATE");
      const bool on = me ? (me[0] == '1') : ((int)grid.x > (m->simds > 0 ? m->simds : 1024) && n_draws >= 100);
      if (on) {
        const size_t nb = mig_board_ints(grid.x) * sizeof(int);
        rc = m->migboard.ensure(nb);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(m->migboard.p, 0, nb, m->stream));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)m->migboard.p, C, 1, m->stream));   // board[0] = chains left
        P.mig = m->migboard.as<int>();
      }
    }
    if (dense) {
      if (T::G != 1 && !M::kRowDense && !M::kLaneDense)
        return fail(EXMC_ERR_UNSUPPORTED, "no dense mass matrix for this model at this lanes_per_chain");
      P.dm.cov = m->dense.as<double>();
      P.dm.chol = m->dense.as<double>() + (size_t)m->d * m->d;
      if constexpr (M::kLaneDense) {
        constexpr int GD = T::G * M::DPL;
        rc = ensure_densep(m, GD);
        if (rc) return rc;
        P.dm.covp = m->densep.as<double>();
        P.dm.cholp = m->densep.as<double>() + (size_t)m->d * GD;
      }
    }
    if constexpr (M::kPipeNutsLevels > 0) {
      // wave pairs (tree + integrator), fewer stack levels in LDS to make room for the mailbox.
      // Opt-in (EXMC_HIP_NUTS_PIPE=1): bit-identical, but the two waves alternate more than they overlap
      // (a doubling starts from the decision of the previous one), DESIGN section 5 --
      // eight_schools 4096 x 1000: 15.3 ms against 14.6 ms for one wave per SIMD.
      const char* pe = std::getenv("EXMC_HIP_NUTS_PIPE");
      if (pe && pe[0] == '1') {
        constexpr int PL = M::kPipeNutsLevels;
        constexpr int kSpillP = (kMaxLevels > PL) ? (kMaxLevels - PL) : 1;
        rc = m->stack.ensure((size_t)kSpillP * nuts_nslot<M>() * nthreads * 8);
        if (rc) return rc;
        P.stack = m->stack.as<double>();
        if (timed) HIP_TRY(hipEventRecord(m->ev0, m->stream));
        const size_t lds_p = nuts_lds_bytes<M, PL>() + pipe_lds_doubles<M::DPL>() * 8;
        EXMC_KLAUNCH(m->device, (nuts_kernel<M, T::G, PL, true>), grid, dim3(2 * kNutsBlock), lds_p,
                     m->stream, P, mc);
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(m->ev1, m->stream));
        return (int)EXMC_OK;
      }
    }
    if constexpr (M::kWgWaves > 0 && !M::kLaneDense && !M::kRowDense) {
      // Workgroups of kWgWaves wavefronts around one LDS image of the model's data (exmc_nuts.hpp
      // nuts_kernel_wg). Worth it as soon as some SIMD has to hold two wavefronts anyway (more waves
      // than SIMDs); below that every wavefront has a SIMD to itself in the one-wave form and a
      // workgroup per compute unit would leave units idle. EXMC_HIP_NUTS_WG=0 / 1 forces either form.
      constexpr int W = M::kWgWaves, WL = M::kWgLdsLevels;
      const char* we = std::getenv("EXMC_HIP_NUTS_WG");
      const size_t waves = grid.x;
      const bool on = we ? (we[0] == '1') : ((int)waves > (m->simds > 0 ? m->simds : 1024));
      if (on && !dense && M::wg_ok(mc)) {
        const dim3 wgrid((unsigned)((waves + W - 1) / W));
        const size_t wthreads = (size_t)wgrid.x * W * kNutsBlock;
        constexpr int kSpillW = (kMaxLevels > WL) ? (kMaxLevels - WL) : 1;
        rc = m->stack.ensure((size_t)kSpillW * nuts_nslot<M>() * wthreads * 8);
        if (rc) return rc;
        P.stack = m->stack.as<double>();
        const size_t lds_w = nuts_wg_lds_bytes<M, WL, W>();
        static_assert(nuts_wg_lds_bytes<M, WL, W>() <= 160 * 1024, "one workgroup per compute unit");
        EXMC_KMAXLDS((nuts_kernel_wg<M, T::G, WL, W>), lds_w);
        if (timed) HIP_TRY(hipEventRecord(m->ev0, m->stream));
        EXMC_KLAUNCH(m->device, (nuts_kernel_wg<M, T::G, WL, W>), wgrid, dim3(W * kNutsBlock), lds_w,
                     m->stream, P, mc);
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(m->ev1, m->stream));
        return (int)EXMC_OK;
      }
    }
    if (timed) HIP_TRY(hipEventRecord(m->ev0, m->stream));
    const size_t lds_bytes = nuts_lds_bytes<M, T::LDSL, M::kNutsZigInLds>();
    if (lds_bytes > 64 * 1024)   // the lane layouts' dense mass keeps M^-1 in LDS
      EXMC_KMAXLDS((nuts_kernel<M, T::G, T::LDSL>), lds_bytes);
    EXMC_KLAUNCH(m->device, (nuts_kernel<M, T::G, T::LDSL>), grid, dim3(kNutsBlock), lds_bytes,
                 m->stream, P, mc);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(m->ev1, m->stream));
    if (P.mig && std::getenv("EXMC_HIP_MIGRATE_STATS")) {
      int h[4];
      HIP_TRY(hipMemcpyAsync(h, P.mig, sizeof(h), hipMemcpyDeviceToHost, m->stream));
      HIP_TRY(hipStreamSynchronize(m->stream));
      fprintf(stderr, "[exmc migrate] chains left %d, moved %d, hosts %d\n", h[0], h[2], h[3]);
    }
    return (int)EXMC_OK;
  });
}

int reset_counters(exmc_hip_model* m) {
  HIP_TRY(hipMemsetAsync(m->misc.as<double>() + 1, 0, 16, m->stream));
  return EXMC_OK;
}
int read_counters(exmc_hip_model* m, int64_t* lf, int32_t* div) {
  unsigned long long h[2];
  HIP_TRY(hipMemcpyAsync(h, m->misc.as<double>() + 1, 16, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (lf) *lf = (int64_t)h[0];
  if (div) *div = (int32_t)h[1];
  return EXMC_OK;
}

int finish_timing(exmc_hip_model* m) {
  HIP_TRY(hipEventSynchronize(m->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, m->ev0, m->ev1));
  m->last_ms = ms;
#ifdef EXMC_XCC_PROBE
  if (const char* path = std::getenv("EXMC_WAVE_PROBE_OUT")) {
    static std::vector<double> h(4096 * 5);
    HIP_TRY(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_wave_probe), h.size() * 8));
    if (FILE* f = std::fopen(path, "w")) {   // rewritten after every timed launch: the last one stays
      std::fprintf(f, "%.3f\n", ms);
      for (int i = 0; i < 4096; i++)   // workgroup, placement, shader clocks, leapfrogs, wall start, wall end
        std::fprintf(f, "%d %.0f %.0f %.0f %.0f %.0f\n", i, h[i * 5], h[i * 5 + 1], h[i * 5 + 2], h[i * 5 + 3], h[i * 5 + 4]);
      std::fclose(f);
    }
  }
#endif
#if EXMC_PROFILE_SECTIONS
  HIP_TRY(print_sections("nuts", ms));
#endif
  return EXMC_OK;
}

// The scratch of a _host form: consecutive typed slices of one device buffer and of their host mirror,
// behind the caller's trace where the form takes one. take() describes the slices (8-byte types first),
// alloc() or alloc_with_trace() makes the buffer, dev() points into it, download() fills the mirror of the
// slices and host() points into that. (The layout loops are exmc_layout_host.hpp.)
struct Scratch {
  template <class T>
  struct Slice { size_t off; };
  CallBuf buf;
  std::vector<char> mirror;
  size_t front = 0, bytes = 0;   // of the trace, of the slices
  template <class T>
  Slice<T> take(size_t n) {
    const Slice<T> s{bytes};
    bytes += n * sizeof(T);
    return s;
  }
  int alloc() { return buf.alloc(front + bytes); }
  // ... with the caller's trace [C][S][d] in the device layout [S][d][C] in front: trace()
  int alloc_with_trace(const double* draws_host, int S, int d, int C) {
    std::vector<double> h((size_t)S * d * C);
    chains_last(draws_host, h.data(), S, d, C);
    front = h.size() * 8;
    int rc = alloc();
    if (rc) return rc;
    HIP_TRY(hipMemcpy(buf.p, h.data(), front, hipMemcpyHostToDevice));
    return EXMC_OK;
  }
  const double* trace() const { return buf.as<double>(); }
  int download() {
    mirror.resize(bytes);
    HIP_TRY(hipMemcpy(mirror.data(), buf.as<char>() + front, bytes, hipMemcpyDeviceToHost));
    return EXMC_OK;
  }
  template <class T>
  T* dev(Slice<T> s) const { return (T*)(buf.as<char>() + front + s.off); }
  template <class T>
  const T* host(Slice<T> s) const { return (const T*)(mirror.data() + s.off); }
};

struct TraceLayout {
  size_t off_draws, off_logp, off_depth, off_nsteps, off_div, off_acc, off_energy, total;
};
TraceLayout trace_layout(int S, int d, int C) {
  TraceLayout L;
  size_t o = 0;
  L.off_draws = o; o += (size_t)S * d * C * 8;
  L.off_logp = o; o += (size_t)S * C * 8;
  L.off_acc = o; o += (size_t)S * C * 8;
  L.off_energy = o; o += (size_t)S * C * 8;
  L.off_depth = o; o += (size_t)S * C * 4;
  L.off_nsteps = o; o += (size_t)S * C * 4;
  L.off_div = o; o += (size_t)S * C * 4;
  L.total = (o + 7) & ~(size_t)7;
  return L;
}
TraceDev trace_view(void* base, const TraceLayout& L) {
  char* b = (char*)base;
  TraceDev t;
  t.draws = (double*)(b + L.off_draws);
  t.logp = (double*)(b + L.off_logp);
  t.accept_prob = (double*)(b + L.off_acc);
  t.energy = (double*)(b + L.off_energy);
  t.tree_depth = (int32_t*)(b + L.off_depth);
  t.n_steps = (int32_t*)(b + L.off_nsteps);
  t.divergent = (int32_t*)(b + L.off_div);
  return t;
}

TraceDev to_dev(const exmc_hip_trace& t) {
  return TraceDev{t.draws, t.logp, t.tree_depth, t.n_steps, t.divergent, t.accept_prob, t.energy};
}
exmc_hip_trace to_abi(const TraceDev& t) {
  return exmc_hip_trace{t.draws, t.logp, t.tree_depth, t.n_steps, t.divergent, t.accept_prob, t.energy};
}

// copy a device-layout staging trace to the caller's host trace ([chain][draw][dim])
int download_trace(exmc_hip_model* m, const TraceLayout& L, int S, int C, exmc_hip_trace out) {
  std::vector<char> h(L.total);
  HIP_TRY(hipMemcpyAsync(h.data(), m->trace.p, L.total, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  TraceDev t = trace_view(h.data(), L);
  if (out.draws) transpose_trace_vec(t.draws, out.draws, S, m->d, C);
  if (out.logp) transpose_trace_scalar(t.logp, out.logp, S, C);
  if (out.accept_prob) transpose_trace_scalar(t.accept_prob, out.accept_prob, S, C);
  if (out.energy) transpose_trace_scalar(t.energy, out.energy, S, C);
  if (out.tree_depth) transpose_trace_scalar(t.tree_depth, out.tree_depth, S, C);
  if (out.n_steps) transpose_trace_scalar(t.n_steps, out.n_steps, S, C);
  if (out.divergent) transpose_trace_scalar(t.divergent, out.divergent, S, C);
  return EXMC_OK;
}

// n draws of the one chain in m->state (sample/3 after its warmup, the pull-style stream) into the
// staging trace and on to the caller's; *div: the draws' divergences
int sample_one_chain(exmc_hip_model* m, bool dense, int lanes, int n, double eps, int max_depth,
                     exmc_hip_trace tr, int32_t* div) {
  TraceLayout L = trace_layout(n, m->d, 1);
  int rc = m->trace.ensure(L.total);
  if (rc) return rc;
  rc = reset_counters(m);
  if (rc) return rc;
  rc = launch_nuts(m, dense, lanes, 1, n, 0, eps, max_depth, trace_view(m->trace.p, L), true);
  if (rc) return rc;
  rc = finish_timing(m);
  if (rc) return rc;
  rc = read_counters(m, nullptr, div);
  if (rc) return rc;
  return download_trace(m, L, n, 1, tr);
}

// ---- host-side adaptation: step_size.ex:13-50, mass_matrix.ex:40-97, sampler.ex:764-785 ----
struct DualAvg {
  double log_epsilon, log_epsilon_bar, h_bar, mu;
  int m;
  double gamma, t0, kappa, target;
  // exp/log through the numeric contract (exmc_detmath.h), m^-kappa as exp(-kappa*log(m)):
  // the same arithmetic warmup_kernel performs on the device.
  void init(double epsilon, double target_accept) {
    log_epsilon = exmc_log(epsilon);
    log_epsilon_bar = exmc_log(epsilon);
    h_bar = 0.0;
    mu = exmc_log(10.0 * epsilon);
    m = 0;
    gamma = 0.05; t0 = 10.0; kappa = 0.75;
    target = target_accept;
  }
  void update(double accept_stat) {
    const int mm = m + 1;
    const double eta = 1.0 / (mm + t0);
    const double hb = (1.0 - eta) * h_bar + eta * (target - accept_stat);
    const double le = mu - std::sqrt((double)mm) / gamma * hb;
    const double mk = exmc_exp(-kappa * exmc_log((double)mm));
    const double leb = mk * le + (1.0 - mk) * log_epsilon_bar;
    m = mm; h_bar = hb; log_epsilon = le; log_epsilon_bar = leb;
  }
  double current() const { return exmc_exp(log_epsilon); }
  double finalize() const { return exmc_exp(log_epsilon_bar); }
};

struct WelfordDiag {
  int n = 0, d = 0;
  std::vector<double> mean, m2;
  void init(int dim) { n = 0; d = dim; mean.assign(dim, 0.0); m2.assign(dim, 0.0); }
  void update(const double* q) {
    const int nn = n + 1;
    for (int i = 0; i < d; i++) {
      const double delta = q[i] - mean[i];
      const double nm = mean[i] + delta / ((double)nn * 1.0);
      const double d2 = q[i] - nm;
      m2[i] = m2[i] + delta * d2;
      mean[i] = nm;
    }
    n = nn;
  }
  void finalize(double* inv_mass) const {
    if (n < 3) {
      for (int i = 0; i < d; i++) inv_mass[i] = 1.0;
      return;
    }
    const double alpha = 5.0 / (n + 5.0);
    for (int i = 0; i < d; i++) {
      double var = m2[i] / ((double)(n - 1) * 1.0);
      var = std::fmax(var, 1.0e-6);
      inv_mass[i] = (1.0 - alpha) * var + alpha * 1.0e-3;
    }
  }
};

std::vector<std::pair<int, int>> build_windows(int from, int to, int base) {
  std::vector<std::pair<int, int>> w;
  if (to - from <= 0) return w;
  int cur = from;
  double size = base;
  while (cur < to) {
    const int remaining = to - cur;
    const int actual = ((double)remaining <= size * 1.5) ? remaining : (int)size;
    w.push_back({cur, cur + actual});
    cur += actual;
    size *= 2;
  }
  return w;
}

// One warmup transition of chain 0 on the GPU; returns accept stat, divergence flag, new q.
struct WarmupStep {
  double accept;
  int divergent;
};

int warmup_transition(exmc_hip_model* m, int lanes, double eps, int max_depth, std::vector<double>& qhost,
                      WarmupStep* out) {
  // mini trace: draws [d], accept [1], divergent (int32) in the next 8 bytes
  const int d = m->d;
  int rc = m->trace.ensure((size_t)(d + 2) * 8);
  if (rc) return rc;
  TraceDev tr{};
  tr.draws = m->trace.as<double>();
  tr.accept_prob = m->trace.as<double>() + d;
  tr.divergent = (int32_t*)(m->trace.as<double>() + d + 1);
  rc = launch_nuts(m, false, lanes, 1, 1, 0, eps, max_depth, tr, false);
  if (rc) return rc;
  std::vector<double> h(d + 2);
  HIP_TRY(hipMemcpyAsync(h.data(), m->trace.p, (size_t)(d + 2) * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  qhost.assign(h.begin(), h.begin() + d);
  out->accept = h[d];
  int32_t dv;
  std::memcpy(&dv, &h[d + 1], 4);
  out->divergent = dv;
  return EXMC_OK;
}

int find_eps(exmc_hip_model* m, int lanes, double* eps) {
  FindEpsParams P;
  P.st = state_view(m, 1);
  P.n_chains = 1;
  P.inv_mass = m->tuning.as<double>();
  P.sqrt_inv_mass = m->tuning.as<double>() + m->d;
  P.log_half = std::log(0.5);
  P.eps_out = m->misc.as<double>();
  P.zig_ki = zig_ki(m); P.zig_wi = zig_wi(m); P.zig_fi = zig_fi(m);
  P.nor_r = EXMC_NOR_R;
  P.flat = flat_order(m);
  int rc = dispatch(m, lanes, [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    const size_t lds_bytes = nuts_lds_bytes<typename T::M, 0>();
    EXMC_KLAUNCH(m->device, (find_eps_kernel<typename T::M, T::G>), dim3(1), dim3(kNutsBlock), lds_bytes,
                 m->stream, P, mc);
    HIP_TRY(hipGetLastError());
    return (int)EXMC_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(eps, m->misc.p, 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return EXMC_OK;
}

// run_warmup (sampler.ex:537-762) on the single-chain state already initialised in m->state
int run_warmup(exmc_hip_model* m, int lanes, exmc_hip_opts o, exmc_hip_tuning* tun,
               const exmc_hip_tuning* start = nullptr) {
  const int d = m->d, W = o.num_warmup;
  std::vector<double> im(d, 1.0), qh(d);
  if (start) im.assign(start->inv_mass, start->inv_mass + d);
  int rc = upload_tuning(m, im.data());
  if (rc) return rc;
  double eps = 1.0;
  if (start) eps = start->epsilon;   // warm start: no initial search (sampler.ex:180-194)
  else rc = find_eps(m, lanes, &eps);
  if (rc) return rc;
  int divergences = 0;
  auto finish = [&](double e) {
    tun->epsilon = e;
    for (int i = 0; i < d; i++) tun->inv_mass[i] = im[i];
    tun->warmup_divergences = divergences;
    return (int)EXMC_OK;
  };
  if (W == 0) return finish(eps);
  const int init_buffer = (75 < W / 3) ? 75 : W / 3;
  const int adapt_end = W - 50;
  DualAvg da;
  da.init(eps, o.target_accept);
  WarmupStep ws;
  for (int i = 0; i < init_buffer; i++) {
    rc = warmup_transition(m, lanes, da.current(), o.max_tree_depth, qh, &ws);
    if (rc) return rc;
    divergences += ws.divergent;
    da.update(ws.accept);
  }
  eps = da.current();
  if (adapt_end <= init_buffer) return finish(da.finalize());
  for (auto win : build_windows(init_buffer, adapt_end, 25)) {
    WelfordDiag wf;
    wf.init(d);
    da.init(eps, o.target_accept);
    for (int i = win.first; i < win.second; i++) {
      const int cap = (i < 200) ? (o.max_tree_depth < 8 ? o.max_tree_depth : 8) : o.max_tree_depth;
      rc = warmup_transition(m, lanes, da.current(), cap, qh, &ws);
      if (rc) return rc;
      divergences += ws.divergent;
      da.update(ws.accept);
      if (!ws.divergent) wf.update(qh.data());
    }
    wf.finalize(im.data());
    rc = upload_tuning(m, im.data());
    if (rc) return rc;
    rc = find_eps(m, lanes, &eps);
    if (rc) return rc;
  }
  da.init(eps, o.target_accept);
  for (int i = adapt_end; i < W; i++) {
    rc = warmup_transition(m, lanes, da.current(), o.max_tree_depth, qh, &ws);
    if (rc) return rc;
    divergences += ws.divergent;
    da.update(ws.accept);
  }
  return finish(da.finalize());
}

// run_warmup (sampler.ex:537-762) in one launch: warmup_kernel keeps dual averaging, Welford and
// the step-size searches on the device; the host only lays out the window schedule.
int run_warmup_device(exmc_hip_model* m, int lanes, exmc_hip_opts o, exmc_hip_tuning* tun,
                      const exmc_hip_tuning* start = nullptr, double* cov_out = nullptr,
                      double* chol_out = nullptr) {
  const bool dense = cov_out != nullptr;
  if (o.max_tree_depth < 1 || o.max_tree_depth > kMaxLevels)
    return fail(EXMC_ERR_BADARG, "max_tree_depth out of range");
  const int d = m->d, W = o.num_warmup;
  WarmupParams P;
  P.st = state_view(m, 1);
  P.num_warmup = W;
  P.max_depth = o.max_tree_depth;
  P.target_accept = o.target_accept;
  P.log_half = std::log(0.5);
  P.init_buffer = (75 < W / 3) ? 75 : W / 3;
  P.adapt_end = W - 50;
  // dense windows are max(25, 10 d) long at the start (sampler.ex:682)
  auto wins = build_windows(P.init_buffer, P.adapt_end, dense ? std::max(25, 10 * d) : 25);
  if (wins.size() > 32) return fail(EXMC_ERR_BADARG, "num_warmup needs more than 32 windows");
  P.dense = dense ? 1 : 0;
  P.dense_ws = nullptr;
  P.n_windows = (int)wins.size();
  for (int k = 0; k < 32; k++) {
    P.win_start[k] = k < P.n_windows ? wins[k].first : -1;
    P.win_end[k] = k < P.n_windows ? wins[k].second : -1;
  }
  P.zig_ki = zig_ki(m); P.zig_wi = zig_wi(m); P.zig_fi = zig_fi(m);
  P.nor_r = EXMC_NOR_R;
  P.flat = flat_order(m);
  P.eps0 = 0.0;
  P.inv_mass0 = P.sqrt_inv_mass0 = nullptr;
  if (start) {   // warm start: previous inverse mass and step size, no initial search
    int rcs = upload_tuning(m, start->inv_mass);
    if (rcs) return rcs;
    P.eps0 = start->epsilon;
    P.inv_mass0 = m->tuning.as<double>();
    P.sqrt_inv_mass0 = m->tuning.as<double>() + d;
  }
  const size_t n_out = (size_t)(8 + d) + (dense ? 2 * (size_t)d * d : 0);
  int rc = m->io.ensure(n_out * 8);
  if (rc) return rc;
  P.out = m->io.as<double>();
  rc = dispatch_mass<true>(m, lanes, dense, [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    using M = typename T::M;
    constexpr int kSpill = (kMaxLevels > T::LDSL) ? (kMaxLevels - T::LDSL) : 1;
    // Replicas: the chain is deterministic and the chip is otherwise idle, so the same warmup runs
    // in `reps` workgroups at once and the first one to finish publishes the result. The time of
    // a one-workgroup kernel depends on the CU it lands on (16.6 to 24.6 ms for the same
    // eight_schools launch over the CUs of one XCD); the race takes the fastest CU of the draw.
    const char* re = std::getenv("EXMC_HIP_WARMUP_REPLICAS");
    int reps = re ? std::atoi(re) : 32;
    reps = reps < 1 ? 1 : (reps > 256 ? 256 : reps);
    if (dense && T::G != 1 && !M::kRowDense && !M::kLaneDense)
      return fail(EXMC_ERR_UNSUPPORTED, "no dense mass matrix for this model at this lanes_per_chain");
    if constexpr (M::kLaneDense) {
      reps = 1;   // one global workspace
      int r3 = m->densews.ensure(LaneDenseWs<T::G, M::DPL, M::D>::doubles() * 8);
      if (r3) return r3;
      P.dense_ws = m->densews.as<double>();
    }
    P.stack_stride = (size_t)kSpill * nuts_nslot<M>() * kNutsBlock;
    int r2 = m->stack.ensure(P.stack_stride * 8 * (size_t)reps);
    if (r2) return r2;
    P.stack = m->stack.as<double>();
    P.race = nullptr;
    if (reps > 1) {
      P.race = (int*)(m->misc.as<double>() + 4);
      HIP_TRY(hipMemsetAsync(P.race, 0, 8, m->stream));
    }
    size_t lds_bytes = nuts_lds_bytes<M, T::LDSL>();
    P.stage_model = 0;
    if (M::kStageDoubles > 0 && lds_bytes + (size_t)M::kStageDoubles * 8 <= 160 * 1024 && M::stage_ok(mc)) {
      P.stage_model = 1;
      lds_bytes += (size_t)M::kStageDoubles * 8;
    }
    // two-wave form (tree wave + integrator wave, exmc_nuts.hpp PipeBox) where the model gains
    // from it; EXMC_HIP_WARMUP_PIPE=0 / 1 forces the one-wave / two-wave kernel
    const char* pe = std::getenv("EXMC_HIP_WARMUP_PIPE");
    const bool pipe = !dense && ((pe && pe[0] == '1') || (M::kPipeWarmup && !(pe && pe[0] == '0'))) &&
                      lds_bytes + pipe_lds_doubles<M::DPL>() * 8 <= 160 * 1024;
    if (dense && !M::kLaneDense) lds_bytes += 3 * (size_t)d * d * 8;   // m2, cov, chol behind everything else
    if (lds_bytes > 160 * 1024) return fail(EXMC_ERR_UNSUPPORTED, "dense warmup state does not fit in LDS");
    if constexpr (!M::kLaneDense && !M::kRowDense && M::kHasPipeWarmup) {   // the dense variants have no two-wave form
      if (pipe) {
        lds_bytes += pipe_lds_doubles<M::DPL>() * 8;
        if (lds_bytes > 64 * 1024)
          EXMC_KMAXLDS((warmup_kernel<M, T::G, T::LDSL, true>), lds_bytes);
        HIP_TRY(hipEventRecord(m->ev0, m->stream));
        EXMC_KLAUNCH(m->device, (warmup_kernel<M, T::G, T::LDSL, true>), dim3(reps), dim3(2 * kNutsBlock),
                     lds_bytes, m->stream, P, mc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(m->ev1, m->stream));
        return (int)EXMC_OK;
      }
    }
    if (lds_bytes > 64 * 1024)
      EXMC_KMAXLDS((warmup_kernel<M, T::G, T::LDSL>), lds_bytes);
    HIP_TRY(hipEventRecord(m->ev0, m->stream));
    EXMC_KLAUNCH(m->device, (warmup_kernel<M, T::G, T::LDSL>), dim3(reps), dim3(kNutsBlock), lds_bytes,
                 m->stream, P, mc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev1, m->stream));
    return (int)EXMC_OK;
  });
  if (rc) return rc;
  std::vector<double> h(n_out);
  HIP_TRY(hipMemcpyAsync(h.data(), m->io.p, h.size() * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  rc = finish_timing(m);
  if (rc) return rc;
#if EXMC_PROFILE_SECTIONS
  HIP_TRY(print_sections("warmup", m->last_ms));
  fprintf(stderr, "[exmc prof]   warmup leapfrogs %.0f\n", h[2]);
#endif
#ifdef EXMC_XCC_PROBE
  fprintf(stderr, "[xcc probe] warmup ran on xcc/cu/se %d, %.3f ms  shader clocks %.0f  wall ticks %.0f\n",
          (int)h[2], m->last_ms, h[3 + d], h[4 + d]);
#endif
  tun->epsilon = h[0];
  tun->warmup_divergences = (int)h[1];
  for (int i = 0; i < d; i++) tun->inv_mass[i] = h[3 + i];
  if (dense) {
    if (!(h[0] > 0.0)) return fail(EXMC_ERR_BADARG, "dense warmup: a window covariance was not positive definite");
    std::memcpy(cov_out, h.data() + 3 + d, (size_t)d * d * 8);
    std::memcpy(chol_out, h.data() + 3 + d + (size_t)d * d, (size_t)d * d * 8);
  }
  return EXMC_OK;
}

// one launch: every chain of [chain_lo, chain_hi) adapts and samples on its own (indep_kernel); the
// layouts with kRoleStream carry it (sample_chains(..., vectorized: false))
int launch_independent(exmc_hip_model* m, int lanes, int C, exmc_hip_opts o, TraceDev tr, double* tune_dev) {
  if (o.max_tree_depth < 1 || o.max_tree_depth > kMaxLevels)
    return fail(EXMC_ERR_BADARG, "max_tree_depth out of range");
  const int W = o.num_warmup;
  IndepParams P;
  P.st = state_view(m, C);
  P.n_chains = C;
  P.num_warmup = W;
  P.num_samples = o.num_samples;
  P.max_depth = o.max_tree_depth;
  P.target_accept = o.target_accept;
  P.log_half = std::log(0.5);
  P.init_buffer = (75 < W / 3) ? 75 : W / 3;
  P.adapt_end = W - 50;
  auto wins = build_windows(P.init_buffer, P.adapt_end, 25);
  if (wins.size() > 32) return fail(EXMC_ERR_BADARG, "num_warmup needs more than 32 windows");
  P.n_windows = (int)wins.size();
  for (int k = 0; k < 32; k++) {
    P.win_start[k] = k < P.n_windows ? wins[k].first : -1;
    P.win_end[k] = k < P.n_windows ? wins[k].second : -1;
  }
  P.tr = tr;
  P.tune_out = tune_dev;
  P.counters = (unsigned long long*)(m->misc.as<double>() + 1);
  P.zig_ki = zig_ki(m); P.zig_wi = zig_wi(m); P.zig_fi = zig_fi(m);
  P.nor_r = EXMC_NOR_R;
  P.flat = flat_order(m);
  return dispatch(m, lanes, [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    using M = typename T::M;
    if constexpr (T::kStream) {
      dim3 grid = grid_for(C, T::G, kNutsBlock);
      const size_t nthreads = (size_t)grid.x * kNutsBlock;
      constexpr int kSpill = (kMaxLevels > T::LDSL) ? (kMaxLevels - T::LDSL) : 1;
      int rc = m->stack.ensure((size_t)kSpill * nuts_nslot<M>() * nthreads * 8);
      if (rc) return rc;
      P.stack = m->stack.as<double>();
      const size_t lds_bytes = nuts_lds_bytes<M, T::LDSL>();
      if (lds_bytes > 64 * 1024) EXMC_KMAXLDS((indep_kernel<M, T::G, T::LDSL>), lds_bytes);
      HIP_TRY(hipEventRecord(m->ev0, m->stream));
      EXMC_KLAUNCH(m->device, (indep_kernel<M, T::G, T::LDSL>), grid, dim3(kNutsBlock), lds_bytes, m->stream, P, mc);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(m->ev1, m->stream));
      return (int)EXMC_OK;
    } else {
      return fail(EXMC_ERR_UNSUPPORTED, "independent adaptation runs in the model kind's default layout");
    }
  });
}

// Every entry point that touches the handle's buffers, stream or counters goes through here. While
// a push-style stream run is in flight (exmc_hip_stream_start .. _finish) the launch is writing the
// page-locked trace and owns ev0 / ev1 and the counters: everything else is refused until
// exmc_hip_stream_finish has been called (the poller may be a thread of the caller's own).
int check_handle(const exmc_hip_model* m) {
  if (!m) return fail(EXMC_ERR_BADARG, "null model handle");
  return EXMC_OK;
}
int check_model(const exmc_hip_model* m) {
  if (!m) return fail(EXMC_ERR_BADARG, "null model handle");
  if (m->stream_in_flight.load(std::memory_order_acquire))
    return fail(EXMC_ERR_BADARG, "a stream run is in flight on this handle: call exmc_hip_stream_finish first");
  return EXMC_OK;
}

// ---- creating a handle: one function per kind ---------------------------------------------------
// Each checks data / n_data, sets d and the constants, uploads the kind's device data image to
// m->data, and names the free variables in kernel order where the kind fixes them (the flat order
// sorts them as strings, point_map.ex:37). No names: the kernel order is sorted already
// (eight_schools, simple, generated models) or the caller's to state (radon).
using Names = std::vector<std::string>;

int upload_image(exmc_hip_model* m, const std::vector<double>& image) {
  int rc = m->data.ensure(image.size() * 8);
  if (rc) return rc;
  if (hipMemcpy(m->data.p, image.data(), image.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail(EXMC_ERR_HIP, "model data upload failed");
  return EXMC_OK;
}

int create_eight_schools(exmc_hip_model* m, const double* data, int n_data, Names&) {
  if (n_data != 16 || !data) return fail(EXMC_ERR_BADARG, "eight_schools needs y[8],sigma[8]");
  m->d = 10;
  for (int j = 0; j < 8; j++) {
    m->es.y[j] = data[j];
    m->es.sg[j] = data[8 + j];
    m->es.lsg[j] = std::log(data[8 + j]);
  }
  m->es.c_mu = log2pi32() + 2.0 * std::log(5.0);
  m->es.c_hc = f32r(std::log(2.0 / M_PI)) - std::log(5.0);
  m->es.c1 = log2pi32() + 2.0 * 0.0;
  return EXMC_OK;
}

int create_simple(exmc_hip_model* m, const double* data, int n_data, Names&) {
  if (n_data < 1 || n_data > 64 || !data) return fail(EXMC_ERR_BADARG, "simple needs 1..64 observations");
  m->d = 2;
  m->sp.n = n_data;
  for (int i = 0; i < n_data; i++) m->sp.y[i] = data[i];
  m->sp.c_mu = log2pi32() + 2.0 * std::log(5.0);
  m->sp.log2pi32 = log2pi32();
  m->sp.tiny32 = f32r(1.0e-30);
  return EXMC_OK;
}

// sv and sv_ncp: the same data and constants (SVNcp<64> reads SV's); kernel order s_1..s_T (z_t), sigma, nu
int create_sv(exmc_hip_model* m, const double* data, int n_data, Names& names) {
  if (n_data != 100 || !data) return fail(EXMC_ERR_BADARG, "sv is compiled for T = 100 returns");
  m->d = 102;
  static const double lanczos[9] = {0.99999999999980993,  676.5203681218851,     -1259.1392167224028,
                                    771.32342877765313,   -176.61502916214059,   12.507343278686905,
                                    -0.13857109526572012, 9.9843695780195716e-6, 1.5056327351493116e-7};
  for (int i = 0; i < 100; i++) m->sv.r[i] = data[i];
  for (int i = 0; i < 9; i++) m->sv.lanczos[i] = f32r(lanczos[i]);
  m->sv.half_log_2pi32 = f32r(0.5 * std::log(2.0 * M_PI));
  m->sv.log2pi32 = log2pi32();
  m->sv.pi32 = f32r(M_PI);
  m->sv.tiny32 = f32r(1.0e-30);
  m->sv.lam_s = 50.0;
  m->sv.lam_n = f32r(0.1);
  m->sv.log_lam_s32 = f32r(std::log(50.0));
  m->sv.log_lam_n32 = f32r(std::log(f32r(0.1)));
  for (int t = 1; t <= 100; t++) names.push_back("s_" + std::to_string(t));
  names.push_back("sigma");
  names.push_back("nu");
  return EXMC_OK;
}

// data = X[N][20] row-major, y[N]; the image: the data, then the MFMA operands Xa = [1 | X]
// zero-padded to 24 / 32 features and Npad observations; kernel order alpha, beta_1..beta_20
int create_logistic(exmc_hip_model* m, const double* data, int n_data, Names& names) {
  if (!data || n_data < 21 || n_data % 21 != 0) return fail(EXMC_ERR_BADARG, "logistic needs X[N][20], y[N]");
  const int N = n_data / 21, K = 20, Npad = (N + 15) / 16 * 16;
  m->d = 21;
  m->lg.N = N;
  m->lg.Npad = Npad;
  m->lg.c10 = log2pi32() + 2.0 * std::log(10.0);
  m->lg.lo = f32r(1.0e-7);
  m->lg.hi = 1.0 - f32r(1.0e-7);
  std::vector<double> blob(data, data + n_data);
  const size_t off_xat = blob.size(), off_xa32 = off_xat + (size_t)24 * Npad, off_yp = off_xa32 + (size_t)Npad * 32;
  blob.resize(off_yp + Npad, 0.0);
  for (int n = 0; n < N; n++) {
    blob[off_xat + n] = 1.0;
    blob[off_xa32 + (size_t)n * 32] = 1.0;
    for (int j = 0; j < K; j++) {
      const double x = data[(size_t)n * K + j];
      blob[off_xat + (size_t)(1 + j) * Npad + n] = x;
      blob[off_xa32 + (size_t)n * 32 + 1 + j] = x;
    }
    blob[off_yp + n] = data[(size_t)N * K + n];
  }
  int rc = upload_image(m, blob);
  if (rc) return rc;
  const double* base = m->data.as<double>();
  m->lg.X = base;
  m->lg.y = base + (size_t)N * K;
  m->lg.XaT = base + off_xat;
  m->lg.Xa32 = base + off_xa32;
  m->lg.ypad = base + off_yp;
  names.push_back("alpha");
  for (int j = 1; j <= K; j++) names.push_back("beta_" + std::to_string(j));
  return EXMC_OK;
}

// data = u[85], county_start[86], floor[N], y[N] (observations sorted by county); the image: the
// data, then the 64-lane layout's copies of y, floor and county, zero-padded to 17 slots of 64 so
// that lane l fetches slot s at base + 8 (64 s + l) with no clamp: [y | floor | 8 * county]
// (RadonConsts::pobs; the county as the byte offset of its intercept in the kernel's alpha strip)
int create_radon(exmc_hip_model* m, const double* data, int n_data, Names&) {
  const int J = 85;
  if (!data || n_data < 2 * J + 1 || (n_data - (2 * J + 1)) % 2 != 0) return fail(EXMC_ERR_BADARG, "radon needs u[85], start[86], floor[N], y[N]");
  const int N = (n_data - (2 * J + 1)) / 2;
  if ((int)data[J] != 0 || (int)data[2 * J] != N) return fail(EXMC_ERR_BADARG, "radon county offsets do not cover the observations");
  // the 64-lane layout keeps a lane's observations in registers, 16 slots of 64 (exmc_models.hpp)
  if (N > 1024) return fail(EXMC_ERR_UNSUPPORTED, "the radon kind holds at most 1024 observations");
  for (int j = 0; j < J; j++)
    if (data[J + j + 1] < data[J + j]) return fail(EXMC_ERR_BADARG, "radon county offsets must be non-decreasing");
  m->d = J + 5;
  m->rd.log2pi32 = log2pi32();
  m->rd.tiny32 = f32r(1.0e-30);
  m->rd.c_mu10 = log2pi32() + 2.0 * std::log(10.0);
  m->rd.c_n5 = log2pi32() + 2.0 * std::log(5.0);
  m->rd.c1 = log2pi32() + 2.0 * 0.0;
  m->rd.c_hc = f32r(std::log(2.0 / M_PI)) - std::log(2.5);
  constexpr int kRadonPad = Radon<64>::kObsPad;   // the capacity + one slot: every (slot, lane) index is an address
  std::vector<double> blob(data, data + n_data);
  const size_t off_pad = blob.size();
  blob.resize(off_pad + (size_t)3 * kRadonPad, 0.0);
  for (int i = 0; i < N; i++) {
    blob[off_pad + i] = data[2 * J + 1 + N + i];
    blob[off_pad + kRadonPad + i] = data[2 * J + 1 + i];
  }
  for (int j = 0; j < J; j++)
    for (int i = (int)data[J + j]; i < (int)data[J + j + 1]; i++) {
      const uint64_t off8 = 8ull * (uint64_t)j;
      std::memcpy(&blob[off_pad + 2 * kRadonPad + i], &off8, 8);
    }
  int rc = upload_image(m, blob);
  if (rc) return rc;
  const double* base = m->data.as<double>();
  m->rd.u = base;
  m->rd.cs = base + J;
  m->rd.fl = base + 2 * J + 1;
  m->rd.y = base + 2 * J + 1 + N;
  m->rd.pobs = base + off_pad;
  return EXMC_OK;
}

#ifdef EXMC_CUSTOM_HEADER
// a generated model: the image holds everything that depends on the data only, evaluated once (same
// arithmetic as the kernels), then a lane layout's tables, folded when the model was generated
int create_custom(exmc_hip_model* m, const double* data, int n_data, Names&) {
  int kGenData = EXMC_GEN_NDATA;
#ifdef EXMC_GEN_VEC
  kGenData += EXMC_GEN_NVU + 16 * EXMC_GEN_NLR;
#endif
#ifdef EXMC_GEN_LANES
  kGenData += EXMC_GEN_NLT;
#endif
#ifdef EXMC_GEN_POINTWISE
  kGenData += EXMC_GEN_PW_NDATA;
#endif
  if (n_data != kGenData || (n_data > 0 && !data)) return fail(EXMC_ERR_BADARG, "generated model: data length differs from the one it was generated for");
  m->d = EXMC_GEN_D;
#ifdef EXMC_GEN_VEC
  std::vector<double> folded(EXMC_GEN_NCONST + EXMC_GEN_NVC + 16 * EXMC_GEN_NLC);
  {
    const double* vdata = data + EXMC_GEN_NDATA;
    double* vc = folded.data() + EXMC_GEN_NCONST;
    exmc_gen_vfold(vdata, vc);
    for (int l = 0; l < 16; l++)
      exmc_gen_vfold_lane(vc, vdata + EXMC_GEN_NVU + l * EXMC_GEN_NLR,
                          vc + EXMC_GEN_NVC + l * EXMC_GEN_NLC);
  }
#else
  std::vector<double> folded(EXMC_GEN_NCONST);
#endif
#ifdef EXMC_GEN_ONE_LANE
  exmc_gen_fold(data, folded.data());
#endif
#ifdef EXMC_GEN_LANES
  while (folded.size() % 16) folded.push_back(0.0);   // the lane layout's table on a 128-byte boundary (codegen_lanes.py)
#endif
  const size_t n_folded = folded.size();
#ifdef EXMC_GEN_LANES
  folded.insert(folded.end(), data + EXMC_GEN_LOFF, data + EXMC_GEN_LOFF + EXMC_GEN_NLT);
#endif
#ifdef EXMC_GEN_POINTWISE
  // the per-datum terms' own constants, after everything the sampling kernels read
  const size_t pw_at = folded.size();
  folded.resize(pw_at + EXMC_GEN_PW_NCONST);
  exmc_gen_pw_fold(data, folded.data() + pw_at);
#endif
  int rc = upload_image(m, folded);
  if (rc) return rc;
#ifdef EXMC_GEN_POINTWISE
  m->pw = m->data.as<double>() + pw_at;
#endif
  m->cu.c = m->data.as<double>();
  m->cu.vc = m->data.as<double>() + EXMC_GEN_NCONST;
  m->cu.lt = m->data.as<double>() + n_folded;
  return EXMC_OK;
}
#endif

int create_kind(exmc_hip_model* m, const double* data, int n_data, Names& names) {
  switch (m->kind) {
    case EXMC_MODEL_EIGHT_SCHOOLS: return create_eight_schools(m, data, n_data, names);
    case EXMC_MODEL_SIMPLE: return create_simple(m, data, n_data, names);
    case EXMC_MODEL_SV:
    case EXMC_MODEL_SV_NCP: return create_sv(m, data, n_data, names);
    case EXMC_MODEL_LOGISTIC: return create_logistic(m, data, n_data, names);
    case EXMC_MODEL_RADON: return create_radon(m, data, n_data, names);
#ifdef EXMC_CUSTOM_HEADER
    case EXMC_MODEL_CUSTOM: return create_custom(m, data, n_data, names);
#endif
    default: return fail(EXMC_ERR_UNSUPPORTED, "model kind not compiled into libexmc_hip");
  }
}

}  // namespace

// =========================================== C ABI ==========================================
extern "C" {

int exmc_hip_model_create(int kind, int d, const double* data, int n_data, int device,
                          exmc_hip_model** out) {
  if (!out) return fail(EXMC_ERR_BADARG, "out is null");
  *out = nullptr;
  int ndev = exmc_hip_device_count();
  if (ndev <= 0)
    return fail(EXMC_ERR_NO_DEVICE, "no HIP device visible: libexmc_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(EXMC_ERR_BADARG, "device index out of range");
#ifdef EXMC_ONLY_CUSTOM
  if (kind != EXMC_MODEL_CUSTOM)
    return fail(EXMC_ERR_UNSUPPORTED, "this plug-in build carries one generated model (EXMC_MODEL_CUSTOM) only");
#endif
  exmc_hip_model* m = new exmc_hip_model();
  m->kind = kind;
  m->device = device;
  auto bail = [&](int rc) { exmc_hip_model_destroy(m); return rc; };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(EXMC_ERR_HIP, "hipSetDevice failed"));
  if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(EXMC_ERR_HIP, "hipStreamCreate failed"));
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      m->simds = 4 * cus;
  }
  if (hipEventCreate(&m->ev0) != hipSuccess || hipEventCreate(&m->ev1) != hipSuccess)
    return bail(fail(EXMC_ERR_HIP, "hipEventCreate failed"));
  int rc = m->zig.ensure(768 * 8);
  if (rc) return bail(rc);
  rc = m->misc.ensure((8 + EXMC_HIP_MAX_D) * 8);
  if (rc) return bail(rc);
  if (hipMemcpy(m->zig.p, kZigKi, 256 * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->zig.as<double>() + 256, kZigWi, 256 * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->zig.as<double>() + 512, kZigFi, 256 * 8, hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(EXMC_ERR_HIP, "table upload failed"));
  Names names;
  rc = create_kind(m, data, n_data, names);
  if (rc) return bail(rc);
  if (d != 0 && d != m->d) return bail(fail(EXMC_ERR_BADARG, "d does not match the model kind"));
  if (!names.empty()) {   // ids sorted as strings (point_map.ex:37)
    std::vector<int32_t> perm(m->d);
    for (int i = 0; i < m->d; i++) perm[i] = i;
    std::sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return names[a] < names[b]; });
    rc = set_flat_order(m, perm.data());
    if (rc) return bail(rc);
  }
  *out = m;
  return EXMC_OK;
}

int exmc_hip_model_set_flat_order(exmc_hip_model* m, const int32_t* perm, int d) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!perm || d != m->d) return fail(EXMC_ERR_BADARG, "flat order needs d entries");
  HIP_TRY(hipSetDevice(m->device));
  m->res_C = 0;   // resident chains were initialised under the previous order
  return set_flat_order(m, perm);
}

void exmc_hip_model_destroy(exmc_hip_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);   // a stream run may still be writing its page-locked trace
  m->zig.release(); m->tuning.release(); m->ms_mass.release(); m->state.release(); m->stack.release();
  m->misc.release(); m->trace.release(); m->io.release(); m->data.release(); m->flat.release(); m->scores.release(); m->dense.release(); m->esswork.release();
  m->densep.release(); m->densews.release(); m->migboard.release();
  if (m->ev0) (void)hipEventDestroy(m->ev0);
  if (m->ev1) (void)hipEventDestroy(m->ev1);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  if (m->pin_host) (void)hipHostFree(m->pin_host);
  delete m;
}

int exmc_hip_model_dim(const exmc_hip_model* m) { return m ? m->d : -1; }
int exmc_hip_model_default_lanes(const exmc_hip_model* m) { return m ? default_lanes(m->kind) : -1; }

int exmc_hip_model_default_warmup_lanes(const exmc_hip_model* m) { return m ? role_lanes(m->kind, kRoleWarmup) : -1; }
int exmc_hip_model_default_dense_lanes(const exmc_hip_model* m) { return m ? role_lanes(m->kind, kRoleDense) : -1; }
void* exmc_hip_model_stream(const exmc_hip_model* m) { return m ? (void*)m->stream : nullptr; }
double exmc_hip_last_kernel_ms(const exmc_hip_model* m) { return m ? m->last_ms : 0.0; }

int exmc_hip_logp_grad_host(exmc_hip_model* m, const double* q, int C, int lanes, double* logp,
                            double* grad) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!q || C < 1) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  lanes = resolve_lanes(m, lanes);
  const int d = m->d;
  // io: q [d][C], grad [d][C], logp [C]
  int rc = m->io.ensure(((size_t)2 * d * C + C) * 8);
  if (rc) return rc;
  std::vector<double> h((size_t)d * C);
  for (int c = 0; c < C; c++)
    for (int i = 0; i < d; i++) h[(size_t)i * C + c] = q[(size_t)c * d + i];
  double* dq = m->io.as<double>();
  double* dg = dq + (size_t)d * C;
  double* dl = dg + (size_t)d * C;
  HIP_TRY(hipMemcpyAsync(dq, h.data(), h.size() * 8, hipMemcpyHostToDevice, m->stream));
  rc = dispatch(m, lanes, [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    const size_t xlds = aux_lds_bytes<typename T::M>();
    HIP_TRY(hipEventRecord(m->ev0, m->stream));   // exmc_hip_last_kernel_ms: this launch alone
    EXMC_KLAUNCH(m->device, (logp_grad_kernel<typename T::M, T::G>), grid_for(C, T::G, kBlock),
                 dim3(kBlock), xlds, m->stream, (const double*)dq, (int)C, (double*)dl, (double*)dg, mc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev1, m->stream));
    return (int)EXMC_OK;
  });
  if (rc) return rc;
  rc = finish_timing(m);
  if (rc) return rc;
  std::vector<double> hg((size_t)d * C), hl(C);
  HIP_TRY(hipMemcpyAsync(hg.data(), dg, hg.size() * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipMemcpyAsync(hl.data(), dl, (size_t)C * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  for (int c = 0; c < C; c++) {
    if (logp) logp[c] = hl[c];
    if (grad)
      for (int i = 0; i < d; i++) grad[(size_t)c * d + i] = hg[(size_t)i * C + c];
  }
  return EXMC_OK;
}

int exmc_hip_multi_step(exmc_hip_model* m, const double* q, const double* p, const double* g,
                        double eps, const double* inv_mass_host, int n_steps, int n_chains,
                        int lanes, double* all_q, double* all_p, double* all_logp, double* all_g) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!q || !p || !g || !inv_mass_host || n_steps < 0 || n_chains < 1 || !all_q || !all_p ||
      !all_logp || !all_g)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  lanes = resolve_lanes(m, lanes);
  // a buffer of its own: m->tuning is the inverse mass resident chains continue under
  int rc = m->ms_mass.ensure((size_t)m->d * 8);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(m->ms_mass.p, inv_mass_host, (size_t)m->d * 8, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  MultiStepParams P;
  P.q = q; P.p = p; P.g = g;
  P.eps = eps;
  P.inv_mass = m->ms_mass.as<double>();
  P.n_steps = n_steps;
  P.n_chains = n_chains;
  P.all_q = all_q; P.all_p = all_p; P.all_g = all_g; P.all_logp = all_logp;
  return dispatch(m, lanes, [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    HIP_TRY(hipEventRecord(m->ev0, m->stream));
    const size_t xlds = aux_lds_bytes<typename T::M>();
    EXMC_KLAUNCH(m->device, (multi_step_kernel<typename T::M, T::G>), grid_for(n_chains, T::G, kBlock),
                 dim3(kBlock), xlds, m->stream, P, mc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev1, m->stream));
    return finish_timing(m);
  });
}

int exmc_hip_multi_step_host(exmc_hip_model* m, const double* q, const double* p, const double* g,
                             double eps, const double* inv_mass, int n_steps, int C, int lanes,
                             double* all_q, double* all_p, double* all_logp, double* all_g) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!q || !p || !g || !inv_mass || n_steps < 0 || C < 1)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  const int d = m->d;
  const size_t vec = (size_t)d * C, rows = (size_t)n_steps * d * C;
  int rc = m->io.ensure((3 * vec + 3 * rows + (size_t)n_steps * C) * 8);
  if (rc) return rc;
  double* dq = m->io.as<double>();
  double* dp = dq + vec;
  double* dg = dp + vec;
  double* aq = dg + vec;
  double* ap = aq + rows;
  double* ag = ap + rows;
  double* al = ag + rows;
  std::vector<double> h(3 * vec);
  for (int c = 0; c < C; c++)
    for (int i = 0; i < d; i++) {
      h[(size_t)i * C + c] = q[(size_t)c * d + i];
      h[vec + (size_t)i * C + c] = p[(size_t)c * d + i];
      h[2 * vec + (size_t)i * C + c] = g[(size_t)c * d + i];
    }
  HIP_TRY(hipMemcpyAsync(dq, h.data(), h.size() * 8, hipMemcpyHostToDevice, m->stream));
  rc = exmc_hip_multi_step(m, dq, dp, dg, eps, inv_mass, n_steps, C, lanes, aq, ap, al, ag);
  if (rc) return rc;
  std::vector<double> out(3 * rows + (size_t)n_steps * C);
  HIP_TRY(hipMemcpyAsync(out.data(), aq, out.size() * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (all_q) transpose_trace_vec(out.data(), all_q, n_steps, d, C);
  if (all_p) transpose_trace_vec(out.data() + rows, all_p, n_steps, d, C);
  if (all_g) transpose_trace_vec(out.data() + 2 * rows, all_g, n_steps, d, C);
  if (all_logp) transpose_trace_scalar(out.data() + 3 * rows, all_logp, n_steps, C);
  return EXMC_OK;
}

int exmc_hip_transitions_host(exmc_hip_model* m, double* q, double* logp, double* grad,
                              uint64_t* rng, int C, int n_draws, double eps,
                              const double* inv_mass, int max_depth, int lanes,
                              exmc_hip_trace trace) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!q || !logp || !grad || !rng || !inv_mass || C < 1 || n_draws < 0)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  lanes = resolve_lanes(m, lanes);
  const int d = m->d;
  int rc = ensure_state(m, C);
  if (rc) return rc;
  rc = upload_tuning(m, inv_mass);
  if (rc) return rc;
  std::vector<double> hs(state_bytes(d, C) / 8);
  double* hq = hs.data();
  double* hg = hq + (size_t)d * C;
  double* hl = hg + (size_t)d * C;
  uint64_t* hr = (uint64_t*)(hl + C);
  for (int c = 0; c < C; c++) {
    for (int i = 0; i < d; i++) {
      hq[(size_t)i * C + c] = q[(size_t)c * d + i];
      hg[(size_t)i * C + c] = grad[(size_t)c * d + i];
    }
    hl[c] = logp[c];
    hr[c] = rng[2 * (size_t)c];
    hr[(size_t)C + c] = rng[2 * (size_t)c + 1];
  }
  HIP_TRY(hipMemcpyAsync(m->state.p, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, m->stream));
  TraceLayout L = trace_layout(n_draws > 0 ? n_draws : 1, d, C);
  rc = m->trace.ensure(L.total);
  if (rc) return rc;
  rc = reset_counters(m);
  if (rc) return rc;
  // the explicit inv_mass is the whole mass of this call: a dense mass installed on the handle is
  // not read (and stays installed)
  rc = launch_nuts(m, false, lanes, C, n_draws, 0, eps, max_depth, trace_view(m->trace.p, L), true);
  if (rc) return rc;
  rc = finish_timing(m);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(hs.data(), m->state.p, hs.size() * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  for (int c = 0; c < C; c++) {
    for (int i = 0; i < d; i++) {
      q[(size_t)c * d + i] = hq[(size_t)i * C + c];
      grad[(size_t)c * d + i] = hg[(size_t)i * C + c];
    }
    logp[c] = hl[c];
    rng[2 * (size_t)c] = hr[c];
    rng[2 * (size_t)c + 1] = hr[(size_t)C + c];
  }
  if (n_draws > 0) return download_trace(m, L, n_draws, C, trace);
  return EXMC_OK;
}

namespace {
int warmup_impl(exmc_hip_model* m, const double* init_q, exmc_hip_opts o, const exmc_hip_tuning* start,
                exmc_hip_tuning* tuning) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!tuning || o.num_warmup < 0) return fail(EXMC_ERR_BADARG, "bad arguments");
  if (start) {
    if (!(start->epsilon > 0.0)) return fail(EXMC_ERR_BADARG, "warm start needs a positive step size");
    for (int i = 0; i < m->d; i++)
      if (!(start->inv_mass[i] > 0.0)) return fail(EXMC_ERR_BADARG, "warm start needs a positive inverse mass");
  }
  HIP_TRY(hipSetDevice(m->device));
  // a warmup adapts a diagonal mass from its own start: a dense mass installed by an earlier call
  // belongs to that call's tuning (and would otherwise reach the sampling that follows this one)
  m->dense_on = false;
  // lanes_per_chain = 0: the library's layout for the one-chain warmup (logistic, generated lane
  // layouts of fewer than 64 lanes: the whole wavefront), not the sampling default
  int lanes = o.lanes_per_chain > 0 ? o.lanes_per_chain : exmc_hip_model_default_warmup_lanes(m);
  int rc = ensure_state(m, 1);
  if (rc) return rc;
  const char* hw = std::getenv("EXMC_HIP_HOST_WARMUP");
  const bool host_driven = hw && hw[0] == '1';
  // the host-driven form launches the sampling kernels: a one-chain form is not among them, so it
  // runs in its sampling layout (other bits than the default, the same schedule)
  if (host_driven) lanes = sampling_lanes(m->kind, lanes);
  rc = launch_init(m, lanes, 1, 0, o.seed, init_q, !host_driven);
  if (rc) return rc;
  if (start && o.num_warmup == 0) {   // sampler.ex:195-196: nothing to tune
    *tuning = *start;
    tuning->warmup_divergences = 0;
    return EXMC_OK;
  }
  // EXMC_HIP_HOST_WARMUP=1 keeps the adaptation scalars on the host (one launch per
  // transition); the default runs the whole schedule in one kernel. Both give the same bits.
  // (The host-driven form runs in sampling layouts only: not in a generated layout's one-chain form.)
  if (host_driven) return run_warmup(m, lanes, o, tuning, start);
  return run_warmup_device(m, lanes, o, tuning, start);
}
}  // namespace

int exmc_hip_warmup(exmc_hip_model* m, const double* init_q, exmc_hip_opts o,
                    exmc_hip_tuning* tuning) {
  return warmup_impl(m, init_q, o, nullptr, tuning);
}

int exmc_hip_warmup_from(exmc_hip_model* m, const double* init_q, exmc_hip_opts o,
                         const exmc_hip_tuning* warm_start, exmc_hip_tuning* tuning) {
  if (!warm_start) return fail(EXMC_ERR_BADARG, "warm_start is null");
  o.num_warmup = o.num_warmup < 50 ? o.num_warmup : 50;   // short_warmup, sampler.ex:188
  return warmup_impl(m, init_q, o, warm_start, tuning);
}

int exmc_hip_model_set_dense_mass(exmc_hip_model* m, const double* cov, const double* chol, int d) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!cov || !chol || d != m->d) return fail(EXMC_ERR_BADARG, "dense mass needs cov and chol_cov, d x d each");
  for (int i = 0; i < d; i++)
    if (!(chol[(size_t)i * d + i] > 0.0)) return fail(EXMC_ERR_BADARG, "chol_cov needs a positive diagonal");
  HIP_TRY(hipSetDevice(m->device));
  int rc = m->dense.ensure(2 * (size_t)d * d * 8);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(m->dense.p, cov, (size_t)d * d * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->dense.as<double>() + (size_t)d * d, chol, (size_t)d * d * 8, hipMemcpyHostToDevice));
  m->h_dense.assign(cov, cov + (size_t)d * d);
  m->h_dense.insert(m->h_dense.end(), chol, chol + (size_t)d * d);
  m->densep_gd = 0;
  m->dense_on = true;
  m->res_C = 0;
  return EXMC_OK;
}

int exmc_hip_model_clear_dense_mass(exmc_hip_model* m) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (m->dense_on) m->res_C = 0;   // the resident chains ran under the dense mass
  m->dense_on = false;
  return EXMC_OK;
}

int exmc_hip_warmup_dense(exmc_hip_model* m, const double* init_q, exmc_hip_opts o,
                          exmc_hip_tuning* tuning, double* cov, double* chol) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!tuning || !cov || !chol || o.num_warmup < 0) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  const int lanes = resolve_lanes(m, o.lanes_per_chain);
  if (!dense_layout_ok(m, lanes))
    return fail(EXMC_ERR_UNSUPPORTED, "no dense mass matrix for this model at this lanes_per_chain (1; eight_schools and logistic 16; sv and radon 64)");
  m->dense_on = false;   // Phase I runs on the identity diagonal (sampler.ex:560-575)
  int rc = ensure_state(m, 1);
  if (rc) return rc;
  rc = launch_init(m, lanes, 1, 0, o.seed, init_q);
  if (rc) return rc;
  rc = run_warmup_device(m, lanes, o, tuning, nullptr, cov, chol);
  if (rc) return rc;
  return exmc_hip_model_set_dense_mass(m, cov, chol, m->d);   // in force for the sampling that follows
}

int exmc_hip_chains_init(exmc_hip_model* m, const exmc_hip_tuning* tuning, const double* init_q,
                         int n_chains, int chain_lo, int chain_hi, exmc_hip_opts o) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!tuning || n_chains < 1 || chain_lo < 0 || chain_hi > n_chains || chain_hi <= chain_lo)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  const int lanes = resolve_lanes(m, o.lanes_per_chain);
  const int C = chain_hi - chain_lo;
  m->res_C = 0;
  int rc = ensure_state(m, C);
  if (rc) return rc;
  rc = upload_tuning(m, tuning->inv_mass);
  if (rc) return rc;
  rc = launch_init(m, lanes, C, chain_lo, o.seed, init_q);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->res_C = C;
  m->res_owner = kResChains;
  m->res_lanes = lanes;
  m->res_eps = tuning->epsilon;
  m->res_max_depth = o.max_tree_depth;
  return EXMC_OK;
}

int exmc_hip_chains_advance(exmc_hip_model* m, int n_draws, int row_offset, exmc_hip_trace tr,
                            int64_t* leapfrogs, int32_t* divergences) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (m->res_C < 1 || m->res_owner != kResChains)
    return fail(EXMC_ERR_BADARG, "no resident chains: call exmc_hip_chains_init");
  if (n_draws < 0 || row_offset < 0) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  int rc = reset_counters(m);
  if (rc) return rc;
  rc = launch_nuts(m, m->dense_on, m->res_lanes, m->res_C, n_draws, row_offset, m->res_eps, m->res_max_depth,
                   to_dev(tr), true);
  if (rc) return rc;
  rc = finish_timing(m);
  if (rc) return rc;
  return read_counters(m, leapfrogs, divergences);
}

int exmc_hip_sample_chains(exmc_hip_model* m, const exmc_hip_tuning* tuning, const double* init_q,
                           int n_chains, int chain_lo, int chain_hi, exmc_hip_opts o,
                           exmc_hip_trace tr, int64_t* total_leapfrogs,
                           int32_t* total_divergences) {
  if (o.num_samples < 0) return fail(EXMC_ERR_BADARG, "bad arguments");
  int rc = exmc_hip_chains_init(m, tuning, init_q, n_chains, chain_lo, chain_hi, o);
  if (rc) return rc;
  return exmc_hip_chains_advance(m, o.num_samples, 0, tr, total_leapfrogs, total_divergences);
}

int exmc_hip_sample_chains_host(exmc_hip_model* m, const exmc_hip_tuning* tuning,
                                const double* init_q, int n_chains, int chain_lo, int chain_hi,
                                exmc_hip_opts o, exmc_hip_trace tr, int64_t* total_leapfrogs,
                                int32_t* total_divergences) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (chain_hi <= chain_lo || o.num_samples < 0) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  const int C = chain_hi - chain_lo;
  if (o.num_samples == 0) {   // nothing to draw: the chains are initialised, the traces stay empty
    if (total_leapfrogs) *total_leapfrogs = 0;
    if (total_divergences) *total_divergences = 0;
    return exmc_hip_chains_init(m, tuning, init_q, n_chains, chain_lo, chain_hi, o);
  }
  TraceLayout L = trace_layout(o.num_samples, m->d, C);
  int rc = m->trace.ensure(L.total);
  if (rc) return rc;
  rc = exmc_hip_sample_chains(m, tuning, init_q, n_chains, chain_lo, chain_hi, o,
                              to_abi(trace_view(m->trace.p, L)), total_leapfrogs, total_divergences);
  if (rc) return rc;
  return download_trace(m, L, o.num_samples, C, tr);
}

int exmc_hip_sample_host(exmc_hip_model* m, const double* init_q, exmc_hip_opts o,
                         exmc_hip_trace tr, exmc_hip_tuning* tuning_out, int32_t* divergences) {
  return exmc_hip_sample_warm_host(m, init_q, o, nullptr, tr, tuning_out, divergences);
}

int exmc_hip_sample_warm_host(exmc_hip_model* m, const double* init_q, exmc_hip_opts o,
                              const exmc_hip_tuning* warm_start, exmc_hip_trace tr,
                              exmc_hip_tuning* tuning_out, int32_t* divergences) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (o.num_samples < 1) return fail(EXMC_ERR_BADARG, "num_samples must be >= 1");
  // this call runs the DIAGONAL adaptation itself: a dense mass left on the handle by an earlier
  // exmc_hip_warmup_dense / _model_set_dense_mass belongs to that run's tuning, not to this one
  m->dense_on = false;
  exmc_hip_tuning tun;
  // one call, one layout: the warmup runs in the layout the draws are sampled in (sample/3 is one
  // chain from start to end; the shared warmup of sample_chains has a layout of its own)
  const int lanes = resolve_lanes(m, o.lanes_per_chain);
  o.lanes_per_chain = lanes;
  // leaves chain 0's state in m->state
  int rc = warm_start ? exmc_hip_warmup_from(m, init_q, o, warm_start, &tun)
                      : exmc_hip_warmup(m, init_q, o, &tun);
  if (rc) return rc;
  rc = upload_tuning(m, tun.inv_mass);
  if (rc) return rc;
  int32_t div = 0;
  rc = sample_one_chain(m, false, lanes, o.num_samples, tun.epsilon, o.max_tree_depth, tr, &div);
  if (rc) return rc;
  if (divergences) *divergences = div + tun.warmup_divergences;  // stats.divergences, sampler.ex:245
  if (tuning_out) *tuning_out = tun;
  return EXMC_OK;
}

int exmc_hip_sample_independent(exmc_hip_model* m, const double* init_q, int n_chains, int chain_lo,
                                int chain_hi, exmc_hip_opts o, exmc_hip_trace tr, double* tuning_host,
                                int64_t* total_leapfrogs, int32_t* total_divergences) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (n_chains < 1 || chain_lo < 0 || chain_hi > n_chains || chain_hi <= chain_lo || o.num_samples < 0 ||
      o.num_warmup < 0)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  m->dense_on = false;   // every chain runs the diagonal adaptation itself
  const int C = chain_hi - chain_lo, d = m->d;
  const int lanes = resolve_lanes(m, o.lanes_per_chain);
  int rc = ensure_state(m, C);
  if (rc) return rc;
  rc = launch_init(m, lanes, C, chain_lo, o.seed, init_q);   // chain i: seed + 7919 i, as sample/3 seeds chain 0
  if (rc) return rc;
  const size_t n_tune = (size_t)C * (3 + d);
  rc = m->io.ensure(n_tune * 8);
  if (rc) return rc;
  rc = reset_counters(m);
  if (rc) return rc;
  rc = launch_independent(m, lanes, C, o, to_dev(tr), m->io.as<double>());
  if (rc) return rc;
  rc = finish_timing(m);
  if (rc) return rc;
  m->res_C = 0;   // the chains ran with tunings of their own: nothing chains_advance could continue
  if (tuning_host)
    HIP_TRY(hipMemcpy(tuning_host, m->io.p, n_tune * 8, hipMemcpyDeviceToHost));
  return read_counters(m, total_leapfrogs, total_divergences);
}

int exmc_hip_sample_independent_host(exmc_hip_model* m, const double* init_q, int n_chains, int chain_lo,
                                     int chain_hi, exmc_hip_opts o, exmc_hip_trace tr, double* tuning_host,
                                     int64_t* total_leapfrogs, int32_t* total_divergences) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (chain_hi <= chain_lo || o.num_samples < 1) return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  const int C = chain_hi - chain_lo;
  TraceLayout L = trace_layout(o.num_samples, m->d, C);
  int rc = m->trace.ensure(L.total);
  if (rc) return rc;
  rc = exmc_hip_sample_independent(m, init_q, n_chains, chain_lo, chain_hi, o,
                                   to_abi(trace_view(m->trace.p, L)), tuning_host, total_leapfrogs,
                                   total_divergences);
  if (rc) return rc;
  return download_trace(m, L, o.num_samples, C, tr);
}

int exmc_hip_sample_dense_host(exmc_hip_model* m, const double* init_q, exmc_hip_opts o,
                               exmc_hip_trace tr, exmc_hip_tuning* tuning_out, double* cov, double* chol,
                               int32_t* divergences) {
  // Sampler.sample/3 with dense_mass: true (sampler.ex:156, 170-176): the dense warmup, then the
  // warmup chain goes on sampling under the dense mass
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (o.num_samples < 1) return fail(EXMC_ERR_BADARG, "num_samples must be >= 1");
  exmc_hip_tuning tun;
  const int lanes = dense_layout_ok(m, resolve_lanes(m, o.lanes_per_chain)) ? resolve_lanes(m, o.lanes_per_chain) : 1;
  o.lanes_per_chain = lanes;
  int rc = exmc_hip_warmup_dense(m, init_q, o, &tun, cov, chol);   // leaves chain 0's state in m->state
  if (rc) return rc;
  rc = upload_tuning(m, tun.inv_mass);
  if (rc) return rc;
  int32_t div = 0;
  rc = sample_one_chain(m, true, lanes, o.num_samples, tun.epsilon, o.max_tree_depth, tr, &div);
  if (rc) return rc;
  if (divergences) *divergences = div + tun.warmup_divergences;
  if (tuning_out) *tuning_out = tun;
  return EXMC_OK;
}

int exmc_hip_stream_begin(exmc_hip_model* m, const double* init_q, exmc_hip_opts o,
                          exmc_hip_tuning* tuning_out) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  m->dense_on = false;   // the diagonal adaptation follows (see exmc_hip_sample_warm_host)
  exmc_hip_tuning tun;
  o.lanes_per_chain = resolve_lanes(m, o.lanes_per_chain);   // one chain, one layout (as sample/3)
  int rc = exmc_hip_warmup(m, init_q, o, &tun);  // leaves chain 0's state in m->state
  if (rc) return rc;
  rc = upload_tuning(m, tun.inv_mass);
  if (rc) return rc;
  // the warmup chain stays resident and is advanced on demand (same state the one-launch
  // exmc_hip_sample_host continues from)
  m->res_C = 1;
  m->res_owner = kResStream;
  m->res_lanes = resolve_lanes(m, o.lanes_per_chain);
  m->res_eps = tun.epsilon;
  m->res_max_depth = o.max_tree_depth;
  if (tuning_out) *tuning_out = tun;
  return EXMC_OK;
}

int exmc_hip_stream_next_host(exmc_hip_model* m, int n_draws, exmc_hip_trace tr,
                              int32_t* divergences) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (m->res_C != 1 || m->res_owner != kResStream) return fail(EXMC_ERR_BADARG, "no stream: call exmc_hip_stream_begin");
  if (n_draws < 1) return fail(EXMC_ERR_BADARG, "n_draws must be >= 1");
  HIP_TRY(hipSetDevice(m->device));
  int32_t div = 0;
  int rc = sample_one_chain(m, false, m->res_lanes, n_draws, m->res_eps, m->res_max_depth, tr, &div);
  if (rc) return rc;
  if (divergences) *divergences = div;
  return EXMC_OK;
}

namespace {
// the body of exmc_hip_stream_start once the handle is claimed
int stream_start_claimed(exmc_hip_model* m, int n_draws, exmc_hip_trace* view,
                         const volatile int32_t** progress) {
  if (m->res_C != 1 || m->res_owner != kResStream) return fail(EXMC_ERR_BADARG, "no stream: call exmc_hip_stream_begin");
  if (n_draws < 1 || !view || !progress) return fail(EXMC_ERR_BADARG, "bad arguments");
  if (m->dense_on) return fail(EXMC_ERR_UNSUPPORTED, "a push-style stream runs under the diagonal mass");
  HIP_TRY(hipSetDevice(m->device));
  const TraceLayout L = trace_layout(n_draws, m->d, 1);
  const size_t need = 64 + L.total;
  if (m->pin_bytes < need) {
    if (m->pin_host) (void)hipHostFree(m->pin_host);
    m->pin_host = nullptr;
    m->pin_bytes = 0;
    HIP_TRY(hipHostMalloc(&m->pin_host, need, hipHostMallocMapped | hipHostMallocPortable));
    m->pin_bytes = need;
  }
  std::memset(m->pin_host, 0, 64);
  void* dev = nullptr;
  HIP_TRY(hipHostGetDevicePointer(&dev, m->pin_host, 0));
  int rc = reset_counters(m);
  if (rc) return rc;
  rc = launch_nuts(m, false, m->res_lanes, 1, n_draws, 0, m->res_eps, m->res_max_depth,
                   trace_view((char*)dev + 64, L), true, (int*)dev);
  if (rc) return rc;
  // with one chain the device layout [draw][dim][chain] is the host layout [draw][dim]
  *view = to_abi(trace_view((char*)m->pin_host + 64, L));
  *progress = (const volatile int32_t*)m->pin_host;
  return EXMC_OK;
}
}  // namespace

int exmc_hip_stream_start(exmc_hip_model* m, int n_draws, exmc_hip_trace* view,
                          const volatile int32_t** progress) {
  if (check_handle(m)) return EXMC_ERR_BADARG;
  // The claim is the compare-and-swap itself: of two callers racing on one handle (two dirty
  // schedulers of a VM) exactly one goes on, the other is refused before it touches the page-locked
  // trace or launches anything. Every failure below gives the claim back.
  bool idle = false;
  if (!m->stream_in_flight.compare_exchange_strong(idle, true, std::memory_order_acq_rel))
    return fail(EXMC_ERR_BADARG, "a stream run is in flight on this handle: call exmc_hip_stream_finish first");
  const int rc = stream_start_claimed(m, n_draws, view, progress);
  if (rc) {
    (void)hipStreamSynchronize(m->stream);   // whatever was queued before the failure has drained
    m->stream_in_flight.store(false, std::memory_order_release);
  }
  return rc;
}

int exmc_hip_stream_finish(exmc_hip_model* m, int32_t* divergences) {
  if (check_handle(m)) return EXMC_ERR_BADARG;
  if (!m->stream_in_flight.load(std::memory_order_acquire)) return fail(EXMC_ERR_BADARG, "no stream run in flight");
  // the handle stays busy until the launch has drained, whatever the calls below return
  int rc = (hipSetDevice(m->device) == hipSuccess) ? finish_timing(m) : fail(EXMC_ERR_HIP, "hipSetDevice failed");
  int32_t div = 0;
  if (!rc) rc = read_counters(m, nullptr, &div);
  if (rc) (void)hipStreamSynchronize(m->stream);
  m->stream_in_flight.store(false, std::memory_order_release);
  if (rc) return rc;
  if (divergences) *divergences = div;
  return EXMC_OK;
}

int exmc_hip_ess(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                 double* ess_dev) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!draws_dev || !ess_dev || n_draws < 1 || d < 1 || n_chains < 1)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  int rc = launch_ess(m->stream, m->esswork, draws_dev, n_draws, d, n_chains, ess_dev);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);
}

int exmc_hip_ess_bulk(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                      double* ess_dev) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!draws_dev || !ess_dev || n_draws < 1 || d < 1 || n_chains < 1)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  if (n_draws < 4) return exmc_hip_ess(m, draws_dev, n_draws, d, n_chains, ess_dev);   // diagnostics.ex:62
  if ((size_t)n_draws * 8 > 160 * 1024)
    return fail(EXMC_ERR_UNSUPPORTED, "n_draws too large for the LDS rank kernel (max 20480)");
  HIP_TRY(hipSetDevice(m->device));
  int rc = m->scores.ensure((size_t)d * n_chains * (size_t)n_draws * 8);   // the normal scores, [S][D][C]
  if (!rc) rc = rank_scores_lds(n_draws);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  rc = launch_rank_scores(m->stream, draws_dev, n_draws, d, n_chains, m->scores.as<double>());
  if (!rc) rc = launch_ess(m->stream, m->esswork, m->scores.as<double>(), n_draws, d, n_chains, ess_dev);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);
}

int exmc_hip_rhat(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                  double* rhat_dev) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!draws_dev || !rhat_dev || n_draws < 4 || d < 1 || n_chains < 1)
    return fail(EXMC_ERR_BADARG, "bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  int rc = m->io.ensure((size_t)d * 4 * n_chains * 8);   // half-chain means and variances
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  rc = launch_rhat(m->stream, draws_dev, n_draws, d, n_chains, m->io.as<double>(), rhat_dev);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);
}

// include/exmc_hip_convergence.h: the kernels and their scratch are exmc_common.hip's; nothing of the
// handle but its device, stream and events is touched
int exmc_hip_convergence(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                         size_t scratch_bytes, double* out_dev) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!draws_dev || !out_dev || n_draws < 8 || d < 1 || n_chains < 1)
    return fail(EXMC_ERR_BADARG, "convergence: need a trace, an output, n_draws >= 8, d >= 1 and n_chains >= 1");
  if (2LL * n_chains * (n_draws / 2) > 0x7FFFFFFFLL)
    return fail(EXMC_ERR_BADARG, "convergence: more than 2^31 - 1 pooled draws per dimension");
  HIP_TRY(hipSetDevice(m->device));
  int rc = launch_convergence(m->stream, m->ev0, draws_dev, n_draws, d, n_chains,
                              scratch_bytes ? scratch_bytes : (size_t)EXMC_CONVERGENCE_DEFAULT_SCRATCH, out_dev);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);
}

int exmc_hip_convergence_host(exmc_hip_model* m, const double* draws_host, int n_draws, int d, int n_chains,
                              size_t scratch_bytes, double* out_host) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!draws_host || !out_host || n_draws < 8 || d < 1 || n_chains < 1)
    return fail(EXMC_ERR_BADARG, "convergence: need a trace, an output, n_draws >= 8, d >= 1 and n_chains >= 1");
  if (2LL * n_chains * (n_draws / 2) > 0x7FFFFFFFLL)
    return fail(EXMC_ERR_BADARG, "convergence: more than 2^31 - 1 pooled draws per dimension");
  HIP_TRY(hipSetDevice(m->device));
  const size_t n_out = (size_t)EXMC_CONVERGENCE_NOUT * d;
  Scratch sc;
  const auto s_out = sc.take<double>(n_out);
  int rc = sc.alloc_with_trace(draws_host, n_draws, d, n_chains);
  if (!rc) rc = exmc_hip_convergence(m, sc.trace(), n_draws, d, n_chains, scratch_bytes, sc.dev(s_out));
  if (!rc) rc = sc.download();
  if (rc) return rc;
  std::copy(sc.host(s_out), sc.host(s_out) + n_out, out_host);
  return EXMC_OK;
}

}  // extern "C"


// ------------------------------------------------------------------------------------------
// Model comparison (include/exmc_hip_compare.h; kernels in exmc_ic.hpp). The calls read the
// handle's model data and nothing else, launch on its stream and allocate their scratch for the
// call alone: the flat order, a dense mass and resident chains stay as they were.
// ------------------------------------------------------------------------------------------
namespace {

int ic_n_data(const exmc_hip_model* m) {
  switch (m->kind) {
    case EXMC_MODEL_SIMPLE: return m->sp.n;
    case EXMC_MODEL_EIGHT_SCHOOLS: return 8;
    case EXMC_MODEL_SV:
    case EXMC_MODEL_SV_NCP: return 100;
    case EXMC_MODEL_LOGISTIC: return m->lg.N;
    case EXMC_MODEL_RADON: return (int)(m->rd.y - m->rd.fl);
#ifdef EXMC_GEN_POINTWISE
    case EXMC_MODEL_CUSTOM: return EXMC_GEN_PW_N;
#endif
    default: return -1;
  }
}

// [4][N] statistics, the matrix, PSIS-LOO's [3][N], the matrix of a block of datums
enum IcMode { kIcStats, kIcMatrix, kIcPsis, kIcRange };
// the block of kIcRange
struct IcRange {
  int i0, nb;
};

struct IcGrid {
  long long chunk;
  int n_chunks, block, yblocks;
};
IcGrid ic_grid(int S, int C, int N) {
  IcGrid g;
  const long long n = (long long)S * C;
  g.chunk = ic_chunk(n);
  g.n_chunks = (int)((n + g.chunk - 1) / g.chunk);
  g.block = N >= kIcBlock ? kIcBlock : (N + 63) / 64 * 64;
  g.yblocks = (N + g.block - 1) / g.block;
  return g;
}

#ifndef EXMC_ONLY_CUSTOM
// partials [n_chunks][kIcFields][N] -> stats [4][N]
int ic_merge(hipStream_t stream, const double* part, const IcGrid& g, long long n, int N, double* stats) {
  hipLaunchKernelGGL(ic_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, part, g.n_chunks,
                     n, g.chunk, N, stats);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

// ---- PSIS-LOO (exmc_psis.hpp) ----
// the scratch of one call: the tables [Nb][P] of the sorted tails and their smoothed values, the
// per-datum results of the tail kernel and the chunk states, for blocks of at most Nb datums
struct PsisScratch {
  CallBuf keys, idx, xs, meta, part;
  int M = 0, P = 0;
  IcGrid g{};
  int alloc(int S, int C, int Nb) {
    const long long n = (long long)S * C;
    M = psis_tail_len(n);
    P = psis_pow2(M);
    g = ic_grid(S, C, Nb);
    int rc = keys.alloc((size_t)Nb * P * 8);
    if (!rc) rc = idx.alloc((size_t)Nb * P * 4);
    if (!rc) rc = xs.alloc((size_t)Nb * P * 8);
    if (!rc) rc = meta.alloc((size_t)Nb * kPsisMeta * 8);
    if (!rc) rc = part.alloc((size_t)g.n_chunks * kPsisFields * Nb * 8);
    if (rc) return rc;
    // the tail kernel's dynamic LDS sits beside some 20 KB of static LDS: above 64 KB in all it has to
    // be asked for, once per call and outside the timed region
    if (P <= kPsisLdsPairs && psis_tail_lds_bytes(P) > 40 * 1024)
      EXMC_KMAXLDS(psis_tail_kernel<true>, psis_tail_lds_bytes(P));
    return EXMC_OK;
  }
};

// where psis_tail_kernel leaves the tails of the datums it is launched over: rows of P entries (keys, idx,
// xs) and kPsisMeta doubles per datum, from these base pointers
struct PsisTables {
  uint64_t* keys;
  uint32_t* idx;
  double* xs;
  double* meta;
  int M, P;
};
PsisTables psis_tables(const PsisScratch& sc) {
  return {sc.keys.as<uint64_t>(), sc.idx.as<uint32_t>(), sc.xs.as<double>(), sc.meta.as<double>(), sc.M, sc.P};
}

// the tails of ll[S][Nb][C] into the tables (kRatio: of the log ratios lr[S][Nb][C], exmc_psis_ratio.hpp)
template <bool kRatio = false>
int psis_tails(hipStream_t stream, const PsisTables& t, const double* ll, int S, int Nb, int C) {
  if (t.P <= kPsisLdsPairs) {
    const size_t lds = psis_tail_lds_bytes(t.P);
    hipLaunchKernelGGL((psis_tail_kernel<true, kRatio>), dim3((unsigned)Nb), dim3(kPsisBlock), lds, stream, ll, S, Nb,
                       C, t.M, t.P, t.keys, t.idx, t.xs, t.meta);
  } else {
    hipLaunchKernelGGL((psis_tail_kernel<false, kRatio>), dim3((unsigned)Nb), dim3(kPsisBlock), 0, stream, ll, S, Nb,
                       C, t.M, t.P, t.keys, t.idx, t.xs, t.meta);
  }
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

// the three launches over ll[S][Nb][C]; rows out[3][N], this block's datums from i0
int psis_launch(hipStream_t stream, const PsisTables& t, double* part, const double* ll, int S, int Nb, int C, int N,
                int i0, double* out) {
  const long long n = (long long)S * C;
  const IcGrid g = ic_grid(S, C, Nb);
  int rc = psis_tails(stream, t, ll, S, Nb, C);
  if (rc) return rc;
  hipLaunchKernelGGL(psis_weights_kernel, dim3((unsigned)g.n_chunks, (unsigned)g.yblocks), dim3(g.block), 0, stream,
                     ll, S, Nb, C, g.chunk, t.P, t.keys, t.idx, t.xs, t.meta, part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(psis_merge_kernel, dim3((unsigned)((Nb + 255) / 256)), dim3(256), 0, stream, part, g.n_chunks, n,
                     Nb, t.meta, N, i0, out);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

constexpr long long kPsisMaxSamples = 0x7FFFFFFFLL;   // sample indices are 32-bit in the tail tables

// the model's datums in blocks whose matrix ll[S][Nb][C] fits scratch_bytes (one datum at the least)
template <class Src>
int psis_kind(exmc_hip_model* m, const Src& src, const double* draws, int S, int C, int N, size_t scratch_bytes,
              double* out) {
  const size_t per = (size_t)S * C * 8;
  size_t fit = scratch_bytes / per;
  const int Nb = (int)(fit < 1 ? 1 : (fit > (size_t)N ? (size_t)N : fit));
  PsisScratch sc;
  CallBuf ll;
  int rc = sc.alloc(S, C, Nb);
  if (!rc) rc = ll.alloc(per * Nb);
  if (rc) return rc;
  const size_t lds = ic_lds_bytes(m->d);
  if (lds > 64 * 1024) EXMC_KMAXLDS(pointwise_ll_range_kernel<Src>, lds);
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  for (int i0 = 0; i0 < N; i0 += Nb) {
    const int nb = (N - i0 < Nb) ? N - i0 : Nb;
    const IcGrid g = ic_grid(S, C, nb);
    hipLaunchKernelGGL(pointwise_ll_range_kernel<Src>, dim3((unsigned)g.n_chunks, (unsigned)g.yblocks),
                       dim3(g.block), lds, m->stream, src, draws, S, m->d, C, i0, nb, g.chunk, ll.as<double>());
    HIP_TRY(hipGetLastError());
    rc = psis_launch(m->stream, psis_tables(sc), sc.part.as<double>(), ll.as<double>(), S, nb, C, N, i0, out);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);   // waits for the kernels: before the scratch is freed
}

template <class Src>
int ic_launch(exmc_hip_model* m, const Src& src, bool matrix, const double* draws, int S, int C, int N,
              double* out) {
  const IcGrid g = ic_grid(S, C, N);
  const size_t lds = ic_lds_bytes(m->d);
  const dim3 grid((unsigned)g.n_chunks, (unsigned)g.yblocks);
  if (matrix) {
    if (lds > 64 * 1024) EXMC_KMAXLDS(pointwise_ll_kernel<Src>, lds);
    HIP_TRY(hipEventRecord(m->ev0, m->stream));   // the timed region: the kernels alone
    hipLaunchKernelGGL(pointwise_ll_kernel<Src>, grid, dim3(g.block), lds, m->stream, src, draws, S, m->d, C, N,
                       g.chunk, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev1, m->stream));
    return finish_timing(m);
  }
  CallBuf part;
  int rc = part.alloc((size_t)g.n_chunks * kIcFields * N * 8);
  if (rc) return rc;
  if (lds > 64 * 1024) EXMC_KMAXLDS(ic_partials_kernel<Src>, lds);
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  hipLaunchKernelGGL(ic_partials_kernel<Src>, grid, dim3(g.block), lds, m->stream, src, draws, S, m->d, C, N,
                     g.chunk, part.as<double>());
  HIP_TRY(hipGetLastError());
  rc = ic_merge(m->stream, part.as<double>(), g, (long long)S * C, N, out);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);   // waits for the kernels: before `part` is freed
}

// the matrix ll[S][nb][C] of the datums r.i0 .. r.i0 + r.nb - 1: the launch psis_kind makes per block
template <class Src>
int ic_range(exmc_hip_model* m, const Src& src, const double* draws, int S, int C, IcRange r, double* out) {
  const IcGrid g = ic_grid(S, C, r.nb);
  const size_t lds = ic_lds_bytes(m->d);
  if (lds > 64 * 1024) EXMC_KMAXLDS(pointwise_ll_range_kernel<Src>, lds);
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  hipLaunchKernelGGL(pointwise_ll_range_kernel<Src>, dim3((unsigned)g.n_chunks, (unsigned)g.yblocks), dim3(g.block),
                     lds, m->stream, src, draws, S, m->d, C, r.i0, r.nb, g.chunk, out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);
}

// what ic_run does with the kind's source
template <class Src>
int ic_dispatch(exmc_hip_model* m, const Src& src, IcMode mode, size_t scratch_bytes, const double* draws, int S,
                int C, int N, double* out, IcRange r) {
  if (mode == kIcPsis) return psis_kind(m, src, draws, S, C, N, scratch_bytes, out);
  if (mode == kIcRange) return ic_range(m, src, draws, S, C, r, out);
  return ic_launch(m, src, mode == kIcMatrix, draws, S, C, N, out);
}

// the source of the handle's kind, handed to f(src) (ic_run, posterior predictive); simple,
// eight_schools and sv keep their data in the handle's constants, uploaded here for the call: f
// returns when its kernels have run
template <class F>
int ic_with_src(exmc_hip_model* m, F&& f) {
  const double l2p = log2pi32();
  std::vector<double> img;
  if (m->kind == EXMC_MODEL_SIMPLE) img.assign(m->sp.y, m->sp.y + m->sp.n);
  if (m->kind == EXMC_MODEL_EIGHT_SCHOOLS) {
    img.assign(m->es.y, m->es.y + 8);
    img.insert(img.end(), m->es.sg, m->es.sg + 8);
  }
  if (m->kind == EXMC_MODEL_SV || m->kind == EXMC_MODEL_SV_NCP) img.assign(m->sv.r, m->sv.r + 100);
  CallBuf dimg;
  if (!img.empty()) {
    int rc = dimg.alloc(img.size() * 8);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dimg.p, img.data(), img.size() * 8, hipMemcpyHostToDevice));
  }
  switch (m->kind) {
    case EXMC_MODEL_SIMPLE: return f(IcSimpleSrc{dimg.as<double>(), l2p, m->sp.tiny32});
    case EXMC_MODEL_EIGHT_SCHOOLS: return f(IcEightSchoolsSrc{dimg.as<double>(), l2p});
    case EXMC_MODEL_SV:
    case EXMC_MODEL_SV_NCP: {
      IcSvSrc src{};
      src.r = dimg.as<double>();
      for (int i = 0; i < 9; i++) src.lz[i] = m->sv.lanczos[i];
      src.half_log_2pi32 = m->sv.half_log_2pi32;
      src.pi32 = m->sv.pi32;
      src.tiny32 = m->sv.tiny32;
      src.ncp = m->kind == EXMC_MODEL_SV_NCP;
      return f(src);
    }
    case EXMC_MODEL_LOGISTIC: return f(IcLogisticSrc{m->lg.X, m->lg.y, m->lg.lo, m->lg.hi});
    case EXMC_MODEL_RADON:
      return f(IcRadonSrc{m->rd.u, m->rd.cs, m->rd.fl, m->rd.y, m->rd.log2pi32, m->rd.tiny32});
    default: return fail(EXMC_ERR_UNSUPPORTED, "this model kind has no per-datum terms");
  }
}

// predictive_kernel<Src> or ppc_kernel<Src> (exmc_predictive.hpp, exmc_ppc.hpp) with `lds` bytes of
// dynamic LDS: one wavefront per 64 chains, between the handle's events
template <class Src, class Params>
int pp_launch(exmc_hip_model* m, void (*kernel)(Src, Params), size_t lds, const Src& src, const Params& P) {
  if (lds > 64 * 1024) EXMC_KMAXLDS(kernel, lds);
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  hipLaunchKernelGGL(kernel, dim3((unsigned)((P.C + kPpBlock - 1) / kPpBlock)), dim3(kPpBlock), lds, m->stream, src, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);   // waits for the kernel: before the source's data image is freed
}

// posterior predictive replicates of the kind's datums
template <class Src>
int predictive_launch(exmc_hip_model* m, const Src& src, const PredictiveParams& P) {
  return pp_launch(m, predictive_kernel<Src>, pp_lds_bytes(m->d), src, P);
}

// the observed values of the kind's datums in the handle's order (ppc_obs_kernel), on the host
template <class Src>
int ppc_observed(exmc_hip_model* m, const Src& src, int N, double* y) {
  CallBuf dy;
  int rc = dy.alloc((size_t)N * 8);
  if (rc) return rc;
  hipLaunchKernelGGL(ppc_obs_kernel<Src>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, m->stream, src, N,
                     dy.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(y, dy.p, (size_t)N * 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return EXMC_OK;
}

// the four statistics of one data set v [N] about the observed mean m0 (include/exmc_hip_ppc.h): the
// expressions ppc_kernel applies to every replicated data set, here for the observed one
void ppc_tstat(const double* v, int N, double m0, double* T) {
  const double Nd = (double)N;
  double A = 0.0, Bq = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < N; i++) {
    const double e = v[i] - m0;
    A = A + e;
    Bq = Bq + e * e;
    mn = (v[i] < mn) ? v[i] : mn;
    mx = (v[i] > mx) ? v[i] : mx;
  }
  T[0] = m0 + A / Nd;
  T[1] = (Bq - (A * A) / Nd) / (Nd - 1.0);
  T[2] = mn;
  T[3] = mx;
}

// posterior predictive checks: the observed values and their statistics first, then the launch
template <class Src>
int ppc_launch(exmc_hip_model* m, const Src& src, PpcParams& P, double* y) {
  int rc = ppc_observed(m, src, P.N, y);
  if (rc) return rc;
  double sum = 0.0;
  for (int i = 0; i < P.N; i++) sum = sum + y[i];
  P.m0 = sum / (double)P.N;
  ppc_tstat(y, P.N, P.m0, P.t_obs);
  return pp_launch(m, ppc_kernel<Src>, ppc_lds_bytes(m->d), src, P);
}

// ---- LOO-PIT (exmc_loo_pit.hpp) ----
// what a call keeps beside the scratch_bytes budget (include/exmc_hip_loo_pit.h "Memory"): the tail tables
// of all N datums, which the second pass reads, and the block states [B][N][4]
struct LooPitScratch {
  CallBuf keys, idx, xs, meta, state;
  int M = 0, P = 0, B = 0;
  int alloc(int S, int C, int N) {
    M = psis_tail_len((long long)S * C);
    P = psis_pow2(M);
    B = (C + kPpBlock - 1) / kPpBlock;
    int rc = keys.alloc((size_t)N * P * 8);
    if (!rc) rc = idx.alloc((size_t)N * P * 4);
    if (!rc) rc = xs.alloc((size_t)N * P * 8);
    if (!rc) rc = meta.alloc((size_t)N * kPsisMeta * 8);
    if (!rc) rc = state.alloc((size_t)B * N * kLooPitFields * 8);
    if (rc) return rc;
    if (P <= kPsisLdsPairs && psis_tail_lds_bytes(P) > 40 * 1024)   // as PsisScratch::alloc
      EXMC_KMAXLDS(psis_tail_kernel<true>, psis_tail_lds_bytes(P));
    return EXMC_OK;
  }
  // the tables from datum i0 on: where a tail launch over the datums i0 .. writes
  PsisTables at(int i0) const {
    return {keys.as<uint64_t>() + (size_t)i0 * P, idx.as<uint32_t>() + (size_t)i0 * P, xs.as<double>() + (size_t)i0 * P,
            meta.as<double>() + (size_t)i0 * kPsisMeta, M, P};
  }
  LooPitTables tables() const { return {keys.as<uint64_t>(), idx.as<uint32_t>(), xs.as<double>(), meta.as<double>(), P}; }
};

int loo_pit_finish(hipStream_t stream, const LooPitScratch& sc, int N, double* out) {
  hipLaunchKernelGGL(loo_pit_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream,
                     sc.state.as<double>(), sc.B, N, sc.meta.as<double>(), out);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

// first pass: the tails of the model's datums, in psis_kind's blocks; second pass: the fused walk; the merge
template <class Src>
int loo_pit_kind(exmc_hip_model* m, const Src& src, LooPitParams& P, size_t scratch_bytes, double* out) {
  const int S = P.S, C = P.C, N = P.N;
  const size_t per = (size_t)S * C * 8;
  const size_t fit = scratch_bytes / per;
  const int Nb = (int)(fit < 1 ? 1 : (fit > (size_t)N ? (size_t)N : fit));
  LooPitScratch sc;
  CallBuf ll;
  int rc = sc.alloc(S, C, N);
  if (!rc) rc = ll.alloc(per * Nb);
  if (rc) return rc;
  P.tab = sc.tables();
  P.state = sc.state.as<double>();
  const size_t lds_ll = ic_lds_bytes(m->d), lds = loo_pit_lds_bytes(m->d);
  if (lds_ll > 64 * 1024) EXMC_KMAXLDS(pointwise_ll_range_kernel<Src>, lds_ll);
  if (lds > 64 * 1024) EXMC_KMAXLDS(loo_pit_kernel<Src>, lds);
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  for (int i0 = 0; i0 < N; i0 += Nb) {
    const int nb = (N - i0 < Nb) ? N - i0 : Nb;
    const IcGrid g = ic_grid(S, C, nb);
    hipLaunchKernelGGL(pointwise_ll_range_kernel<Src>, dim3((unsigned)g.n_chunks, (unsigned)g.yblocks),
                       dim3(g.block), lds_ll, m->stream, src, P.draws, S, m->d, C, i0, nb, g.chunk, ll.as<double>());
    HIP_TRY(hipGetLastError());
    rc = psis_tails(m->stream, sc.at(i0), ll.as<double>(), S, nb, C);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(loo_pit_kernel<Src>, dim3((unsigned)sc.B), dim3(kPpBlock), lds, m->stream, src, P);
  HIP_TRY(hipGetLastError());
  rc = loo_pit_finish(m->stream, sc, N, out);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);   // waits for the kernels: before the scratch is freed
}

#endif

#ifdef EXMC_GEN_POINTWISE
// a generated model's per-datum terms (exmc_gen_pointwise.hpp): one lane per sample, the constants from
// the handle's image
int gen_pointwise(exmc_hip_model* m, const double* draws, int S, int C, IcRange r, double* out) {
  GenPwParams P{m->pw, draws, out, S, C, r.i0, r.nb};
  const long long n = (long long)S * C;
  const long long blocks = (n + kGenPwBlock - 1) / kGenPwBlock;
  if (blocks > 0x7FFFFFFFLL) return fail(EXMC_ERR_BADARG, "model comparison: too many samples for one launch");
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  EXMC_KLAUNCH(m->device, (gen_pointwise_kernel<EXMC_GEN_PW_N>), dim3((unsigned)blocks), dim3(kGenPwBlock), 0,
               m->stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);
}
#endif

// the kind's source of ll over a device trace
int ic_run(exmc_hip_model* m, IcMode mode, const double* draws, int S, int d, int C, double* out,
           size_t scratch_bytes = 0, IcRange r = IcRange{0, 0}) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  const int N = ic_n_data(m);
  if (N < 0) return fail(EXMC_ERR_UNSUPPORTED, "model comparison: this model kind has no per-datum terms");
  if (!draws || !out || d != m->d || S < 1 || C < 1 || (long long)S * C < 2)
    return fail(EXMC_ERR_BADARG, "model comparison: bad arguments");
  if (mode == kIcRange && (r.i0 < 0 || r.nb < 1 || r.i0 >= N || r.nb > N - r.i0))
    return fail(EXMC_ERR_BADARG, "model comparison: the datum range is not inside [0, N)");
  HIP_TRY(hipSetDevice(m->device));
#ifdef EXMC_ONLY_CUSTOM
  (void)scratch_bytes;
#ifdef EXMC_GEN_POINTWISE
  // the terms themselves; the reductions are libexmc_hip.so's (a plug-in carries no reduction kernels)
  if (mode == kIcMatrix) return gen_pointwise(m, draws, S, C, IcRange{0, N}, out);
  if (mode == kIcRange) return gen_pointwise(m, draws, S, C, r, out);
  return fail(EXMC_ERR_UNSUPPORTED, "model comparison: a generated model reduces through "
              "exmc_hip_pointwise_loglik_range and libexmc_hip.so's exmc_hip_ic_stats_from_ll / "
              "exmc_hip_psis_stats_from_ll");
#else
  (void)mode; (void)out; (void)r;
  return fail(EXMC_ERR_UNSUPPORTED, "model comparison: this model kind has no per-datum terms");
#endif
#else
  if (mode == kIcPsis && (long long)S * C > kPsisMaxSamples)
    return fail(EXMC_ERR_BADARG, "psis: more than 2^31 - 1 pooled samples");
  return ic_with_src(m, [&](const auto& src) {
    return ic_dispatch(m, src, mode, scratch_bytes, draws, S, C, N, out, r);
  });
#endif
}

// the _host forms: the caller's [C][S][d] trace staged in the device layout [S][d][C], `run(draws_dev,
// out_dev)`, and its rows x N doubles back
template <class Run>
int ic_from_host(exmc_hip_model* m, const double* draws_host, int n_draws, int d, int n_chains, int rows,
                 double* out_host, Run&& run) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  const int N = ic_n_data(m);
  if (N < 0) return fail(EXMC_ERR_UNSUPPORTED, "model comparison: this model kind has no per-datum terms");
  if (!draws_host || !out_host || d != m->d || n_draws < 1 || n_chains < 1 || (long long)n_draws * n_chains < 2)
    return fail(EXMC_ERR_BADARG, "model comparison: bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  Scratch sc;
  const auto s_out = sc.take<double>((size_t)rows * N);
  int rc = sc.alloc_with_trace(draws_host, n_draws, d, n_chains);
  if (!rc) rc = run(sc.trace(), sc.dev(s_out));
  if (!rc) rc = sc.download();
  if (rc) return rc;
  std::copy(sc.host(s_out), sc.host(s_out) + (size_t)rows * N, out_host);
  return EXMC_OK;
}

}  // namespace

extern "C" {

int exmc_hip_model_n_data(const exmc_hip_model* m) {
  if (!m) return -1;
  return ic_n_data(m);
}

int exmc_hip_pointwise_loglik(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                              double* ll_dev) {
  return ic_run(m, kIcMatrix, draws_dev, n_draws, d, n_chains, ll_dev);
}

int exmc_hip_pointwise_loglik_range(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                                    int i0, int nb, double* ll_dev) {
  return ic_run(m, kIcRange, draws_dev, n_draws, d, n_chains, ll_dev, 0, IcRange{i0, nb});
}

int exmc_hip_ic_stats(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                      double* stats_dev) {
  return ic_run(m, kIcStats, draws_dev, n_draws, d, n_chains, stats_dev);
}

int exmc_hip_ic_stats_host(exmc_hip_model* m, const double* draws_host, int n_draws, int d, int n_chains,
                           double* stats_host) {
  return ic_from_host(m, draws_host, n_draws, d, n_chains, 4, stats_host, [&](const double* draws, double* stats) {
    return ic_run(m, kIcStats, draws, n_draws, d, n_chains, stats);
  });
}

int exmc_hip_ic_stats_from_ll(int device, const double* ll_dev, int n_draws, int n_data, int n_chains,
                              double* stats_dev) {
  if (!ll_dev || !stats_dev || n_draws < 1 || n_data < 1 || n_chains < 1 || (long long)n_draws * n_chains < 2)
    return fail(EXMC_ERR_BADARG, "model comparison: bad arguments");
  int rc = select_device(device);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  // a generated model's plug-in carries no model-comparison kernels: libexmc_hip.so serves this call
  return fail(EXMC_ERR_UNSUPPORTED, "model comparison: use libexmc_hip.so for the model-free reduction");
#else
  const int S = n_draws, C = n_chains, N = n_data;
  const IcGrid g = ic_grid(S, C, N);
  CallBuf part;
  rc = part.alloc((size_t)g.n_chunks * kIcFields * N * 8);
  if (rc) return rc;
  const size_t lds = ic_lds_bytes(0);
  hipLaunchKernelGGL(ic_partials_kernel<IcMatrixSrc>, dim3((unsigned)g.n_chunks, (unsigned)g.yblocks), dim3(g.block),
                     lds, (hipStream_t)0, IcMatrixSrc{ll_dev}, (const double*)nullptr, S, 0, C, N, g.chunk,
                     part.as<double>());
  HIP_TRY(hipGetLastError());
  rc = ic_merge((hipStream_t)0, part.as<double>(), g, (long long)S * C, N, stats_dev);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)0));
  return EXMC_OK;
#endif
}

int exmc_hip_psis_stats(exmc_hip_model* m, const double* draws_dev, int n_draws, int d, int n_chains,
                        size_t scratch_bytes, double* out_dev) {
  return ic_run(m, kIcPsis, draws_dev, n_draws, d, n_chains, out_dev,
                scratch_bytes ? scratch_bytes : (size_t)EXMC_PSIS_DEFAULT_SCRATCH);
}

int exmc_hip_psis_stats_host(exmc_hip_model* m, const double* draws_host, int n_draws, int d, int n_chains,
                             size_t scratch_bytes, double* out_host) {
  return ic_from_host(m, draws_host, n_draws, d, n_chains, 3, out_host, [&](const double* draws, double* out) {
    return exmc_hip_psis_stats(m, draws, n_draws, d, n_chains, scratch_bytes, out);
  });
}

int exmc_hip_psis_stats_from_ll(int device, const double* ll_dev, int n_draws, int n_data, int n_chains,
                                double* out_dev) {
  if (!ll_dev || !out_dev || n_draws < 1 || n_data < 1 || n_chains < 1 || (long long)n_draws * n_chains < 2)
    return fail(EXMC_ERR_BADARG, "model comparison: bad arguments");
  int rc = select_device(device);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  return fail(EXMC_ERR_UNSUPPORTED, "model comparison: use libexmc_hip.so for the model-free reduction");
#else
  if ((long long)n_draws * n_chains > kPsisMaxSamples)
    return fail(EXMC_ERR_BADARG, "psis: more than 2^31 - 1 pooled samples");
  PsisScratch sc;
  rc = sc.alloc(n_draws, n_chains, n_data);
  if (rc) return rc;
  rc = psis_launch((hipStream_t)0, psis_tables(sc), sc.part.as<double>(), ll_dev, n_draws, n_data, n_chains, n_data, 0,
                   out_dev);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)0));
  return EXMC_OK;
#endif
}

}  // extern "C"

namespace {

// ---- what Pathfinder and ADVI share: one fit per lane group, one launch -----------------------------
// KERNEL<M, G> of the handle's layout over n lane groups, one wavefront per workgroup (the launch shape of
// init_chains_kernel), between the handle's events
#define EXMC_FIT_LAUNCH(m, lanes, KERNEL, n, P)                                                        \
  dispatch(m, lanes, [&](auto tag, const auto& mc) {                                                   \
    using T = decltype(tag);                                                                           \
    const size_t xlds = aux_lds_bytes<typename T::M>();                                                \
    HIP_TRY(hipEventRecord(m->ev0, m->stream));                                                        \
    EXMC_KLAUNCH(m->device, (KERNEL<typename T::M, T::G>), grid_for(n, T::G, kBlock), dim3(kBlock),    \
                 xlds, m->stream, P, mc);                                                              \
    HIP_TRY(hipGetLastError());                                                                        \
    HIP_TRY(hipEventRecord(m->ev1, m->stream));                                                        \
    return (int)EXMC_OK;                                                                               \
  })

int pf_check(exmc_hip_model* m, const exmc_hip_pf_opts& o, int n_paths, int chain_lo) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  static_assert(EXMC_PF_MAX_HISTORY == kPfHistory, "the header states the kernel's bound");
  if (o.max_iters < 1 || o.num_draws < 1 || o.history_size < 1 || o.history_size > kPfHistory)
    return fail(EXMC_ERR_BADARG, "pathfinder: max_iters >= 1, num_draws >= 1 and 1 <= history_size <= 6");
  if (n_paths < 1 || chain_lo < 0) return fail(EXMC_ERR_BADARG, "pathfinder: bad arguments");
  return EXMC_OK;
}

int advi_check(exmc_hip_model* m, const exmc_hip_advi_opts& o, int n_fits, int chain_lo) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (o.max_iters < 1 || o.num_draws < 1 || o.num_mc_samples < 1 || o.window_size < 2)
    return fail(EXMC_ERR_BADARG, "advi: max_iters >= 1, num_draws >= 1, num_mc_samples >= 1 and window_size >= 2");
  if (n_fits < 1 || chain_lo < 0) return fail(EXMC_ERR_BADARG, "advi: bad arguments");
  return EXMC_OK;
}

// what exmc_hip_posterior_predictive and exmc_hip_ppc (and their _host forms) ask of their arguments;
// `what` opens the messages, `own_bad` is the entry point's own clause of the argument check
int pp_check(exmc_hip_model* m, const char* what, const exmc_hip_predictive_opts& o, const void* draws, int n_draws,
             int d, int n_chains, bool own_bad) {
  if (check_model(m)) return EXMC_ERR_BADARG;
#ifdef EXMC_ONLY_CUSTOM
  (void)o; (void)draws; (void)n_draws; (void)d; (void)n_chains; (void)own_bad;
  return fail(EXMC_ERR_UNSUPPORTED, std::string(what) + ": generated models are not supported");
#else
  if (m->kind == EXMC_MODEL_CUSTOM || ic_n_data(m) < 0)
    return fail(EXMC_ERR_UNSUPPORTED, std::string(what) + ": this model kind has no built-in datums");
  if (!draws || d != m->d || n_draws < 1 || n_chains < 1 || o.chain_lo < 0 || own_bad)
    return fail(EXMC_ERR_BADARG, std::string(what) + ": bad arguments");
  return EXMC_OK;
#endif
}

// the fields PredictiveParams, PpcParams and LooPitParams share
template <class Params>
void pp_fill(Params& P, exmc_hip_model* m, const exmc_hip_predictive_opts& o, const double* draws_dev, int n_draws,
             int d, int n_chains) {
  P.draws = draws_dev;
  P.S = n_draws;
  P.d = d;
  P.C = n_chains;
  P.N = ic_n_data(m);
  P.chain_lo = o.chain_lo;
  P.base_seed = o.seed;
  P.rng = rng_args(m);
}

#ifndef EXMC_ONLY_CUSTOM
// ---- the prior walk (include/exmc_hip_prior.h; prior_kernel, exmc_prior.hpp) --------------------------
// The free variables of the kind, indexed by kernel dimension, as the IR the kind stands for has them
// after Rewrite.apply: the family, the transform and the two parameters, a literal (ref < 0) or the
// kernel dimension of the parent. The literals are those of the kind's log-density (exmc_models.hpp).
std::vector<PriorEntry> prior_vars(const exmc_hip_model* m) {
  std::vector<PriorEntry> v((size_t)m->d);
  auto set = [&](int j, int family, int log, double a, double b, int ra = -1, int rb = -1) {
    v[j] = PriorEntry{j, family, log, {ra, rb}, 0, {a, b}};
  };
  switch (m->kind) {
    case EXMC_MODEL_SIMPLE:
      set(0, kPriorNormal, 0, 0.0, 5.0);
      set(1, kPriorExponential, 1, 1.0, 0.0);
      break;
    case EXMC_MODEL_EIGHT_SCHOOLS:
      set(0, kPriorNormal, 0, 0.0, 5.0);
      set(1, kPriorHalfCauchy, 1, 5.0, 0.0);
      for (int j = 2; j < 10; j++) set(j, kPriorNormal, 0, 0.0, 1.0);
      break;
    case EXMC_MODEL_SV:
    case EXMC_MODEL_SV_NCP:
      // s_1 ~ N(0.0, sigma); s_t ~ N(s_{t-1}, sigma), which the non-centring pass rewrites to z_t ~ N(0, 1)
      set(0, kPriorNormal, 0, 0.0, 0.0, -1, 100);
      for (int t = 1; t < 100; t++) {
        if (m->kind == EXMC_MODEL_SV_NCP) set(t, kPriorNormal, 0, 0.0, 1.0);
        else set(t, kPriorNormal, 0, 0.0, 0.0, t - 1, 100);
      }
      set(100, kPriorExponential, 1, m->sv.lam_s, 0.0);
      set(101, kPriorExponential, 1, m->sv.lam_n, 0.0);
      break;
    case EXMC_MODEL_LOGISTIC:
      for (int j = 0; j < m->d; j++) set(j, kPriorNormal, 0, 0.0, 10.0);
      break;
    case EXMC_MODEL_RADON:
      for (int j = 0; j < 85; j++) set(j, kPriorNormal, 0, 0.0, 1.0);
      set(85, kPriorNormal, 0, 0.0, 10.0);        // mu_alpha
      set(86, kPriorNormal, 0, 0.0, 5.0);         // gamma_u
      set(87, kPriorHalfCauchy, 1, 2.5, 0.0);     // sigma_alpha
      set(88, kPriorHalfCauchy, 1, 2.5, 0.0);     // sigma_y
      set(89, kPriorNormal, 0, 0.0, 5.0);         // beta
      break;
    default: v.clear();
  }
  return v;
}

// kahn_sort (predictive.ex:159-196): always the smallest ready id by string comparison, the string
// order being the handle's flat order
std::vector<PriorEntry> prior_program(const exmc_hip_model* m) {
  const std::vector<PriorEntry> v = prior_vars(m);
  const int d = (int)v.size();
  std::vector<int> deg((size_t)d, 0);
  std::vector<char> done((size_t)d, 0);
  for (int j = 0; j < d; j++) deg[j] = (v[j].ref[0] >= 0) + (v[j].ref[1] >= 0);
  auto rank = [&](int j) { return m->h_rank.empty() ? j : (int)m->h_rank[j]; };
  std::vector<PriorEntry> prog;
  for (int n = 0; n < d; n++) {
    int pick = -1;
    for (int j = 0; j < d; j++)
      if (!done[j] && deg[j] == 0 && (pick < 0 || rank(j) < rank(pick))) pick = j;
    if (pick < 0) break;   // (no built-in kind has a cycle)
    done[pick] = 1;
    prog.push_back(v[pick]);
    for (int j = 0; j < d; j++)
      if (!done[j] && (v[j].ref[0] == pick || v[j].ref[1] == pick)) deg[j]--;
  }
  return prog;
}

#endif

// what exmc_hip_prior_samples and its _host form ask of their arguments (pp_check; x stands where the
// trace stands there)
int prior_check(exmc_hip_model* m, const exmc_hip_predictive_opts& o, int n_draws, int n_chains, const void* x,
                const void* q, const void* rng_state) {
  return pp_check(m, "prior samples", o, x, n_draws, m ? m->d : 0, n_chains, !q || (o.resume && !rng_state));
}

}  // namespace

extern "C" {

// ---- Pathfinder (include/exmc_hip_pathfinder.h; pathfinder_kernel, exmc_pathfinder.hpp) --------------
int exmc_hip_pathfinder(exmc_hip_model* m, exmc_hip_pf_opts o, int n_paths, int chain_lo, double* draws_dev,
                        double* mu_dev, double* sigma_dev, double* elbo_dev, int32_t* num_iters_dev,
                        int32_t* best_index_dev, int32_t* status_dev) {
  int rc = pf_check(m, o, n_paths, chain_lo);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(m->device));
  const int lanes = resolve_lanes(m, o.lanes_per_chain);
  PathfinderParams P;
  P.n_chains = n_paths;
  P.chain_lo = chain_lo;
  P.base_seed = o.seed;
  P.max_iters = o.max_iters;
  P.history_size = o.history_size;
  P.num_draws = o.num_draws;
  P.entropy_const = 0.5 * m->d * (1.0 + std::log(2.0 * M_PI));   // pathfinder.ex:165, :math.log
  P.draws = draws_dev;
  P.mu = mu_dev;
  P.sigma = sigma_dev;
  P.elbo = elbo_dev;
  P.num_iters = num_iters_dev;
  P.best_index = best_index_dev;
  P.status = status_dev;
  P.rng = rng_args(m);
  P.flat = flat_order(m);
  rc = EXMC_FIT_LAUNCH(m, lanes, pathfinder_kernel, n_paths, P);
  if (rc) return rc;
  return finish_timing(m);   // waits for the launch
}

int exmc_hip_pathfinder_host(exmc_hip_model* m, exmc_hip_pf_opts o, int n_paths, int chain_lo, double* draws,
                             double* mu, double* sigma, double* elbo, int32_t* num_iters, int32_t* best_index,
                             int32_t* status) {
  int rc = pf_check(m, o, n_paths, chain_lo);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(m->device));
  const size_t C = (size_t)n_paths, d = (size_t)m->d, S = (size_t)o.num_draws;
  Scratch sc;
  const auto s_draws = sc.take<double>(draws ? S * d * C : 0);   // [S][d][C]
  const auto s_mu = sc.take<double>(d * C), s_sigma = sc.take<double>(d * C), s_elbo = sc.take<double>(C);
  const auto s_iters = sc.take<int32_t>(C), s_best = sc.take<int32_t>(C), s_status = sc.take<int32_t>(C);
  rc = sc.alloc();
  if (rc) return rc;
  rc = exmc_hip_pathfinder(m, o, n_paths, chain_lo, draws ? sc.dev(s_draws) : nullptr, sc.dev(s_mu), sc.dev(s_sigma),
                           sc.dev(s_elbo), sc.dev(s_iters), sc.dev(s_best), sc.dev(s_status));
  if (!rc) rc = sc.download();
  if (rc) return rc;
  if (draws) transpose_trace_vec(sc.host(s_draws), draws, o.num_draws, m->d, n_paths);
  fits_first(sc.host(s_mu), mu, d, C);
  fits_first(sc.host(s_sigma), sigma, d, C);
  fits_first(sc.host(s_elbo), elbo, 1, C);
  fits_first(sc.host(s_iters), num_iters, 1, C);
  fits_first(sc.host(s_best), best_index, 1, C);
  fits_first(sc.host(s_status), status, 1, C);
  return EXMC_OK;
}

// ---- ADVI (include/exmc_hip_advi.h; advi_kernel, exmc_advi.hpp) --------------------------------------
int exmc_hip_advi(exmc_hip_model* m, exmc_hip_advi_opts o, int n_fits, int chain_lo, double* draws_dev,
                  double* mu_dev, double* log_sigma_dev, double* elbo_history_dev, int32_t* num_iters_dev,
                  int32_t* converged_dev) {
  int rc = advi_check(m, o, n_fits, chain_lo);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(m->device));
  const int lanes = resolve_lanes(m, o.lanes_per_chain);
  // the ELBO window is read back from the history: scratch of the call where the caller wants none
  CallBuf window;
  if (!elbo_history_dev) {
    rc = window.alloc((size_t)o.max_iters * (size_t)n_fits * 8);
    if (rc) return rc;
  }
  AdviParams P;
  P.n_chains = n_fits;
  P.chain_lo = chain_lo;
  P.base_seed = o.seed;
  P.max_iters = o.max_iters;
  P.num_draws = o.num_draws;
  P.num_mc_samples = o.num_mc_samples;
  P.window_size = o.window_size;
  P.learning_rate = o.learning_rate;
  P.convergence_tol = o.convergence_tol;
  P.entropy_const = 0.5 * m->d * (1.0 + std::log(2.0 * M_PI));   // advi.ex:126, :math.log
  P.history = elbo_history_dev ? elbo_history_dev : window.as<double>();
  P.fill_history = elbo_history_dev ? 1 : 0;
  P.draws = draws_dev;
  P.mu = mu_dev;
  P.log_sigma = log_sigma_dev;
  P.num_iters = num_iters_dev;
  P.converged = converged_dev;
  P.rng = rng_args(m);
  P.flat = flat_order(m);
  rc = EXMC_FIT_LAUNCH(m, lanes, advi_kernel, n_fits, P);
  if (rc) return rc;
  return finish_timing(m);   // waits for the launch: before the window is freed
}

int exmc_hip_advi_host(exmc_hip_model* m, exmc_hip_advi_opts o, int n_fits, int chain_lo, double* draws,
                       double* mu, double* log_sigma, double* elbo_history, int32_t* num_iters,
                       int32_t* converged) {
  int rc = advi_check(m, o, n_fits, chain_lo);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(m->device));
  const size_t C = (size_t)n_fits, d = (size_t)m->d, S = (size_t)o.num_draws, I = (size_t)o.max_iters;
  Scratch sc;
  const auto s_draws = sc.take<double>(draws ? S * d * C : 0);     // [S][d][C]
  const auto s_hist = sc.take<double>(elbo_history ? I * C : 0);   // [I][C]
  const auto s_mu = sc.take<double>(d * C), s_ls = sc.take<double>(d * C);
  const auto s_iters = sc.take<int32_t>(C), s_conv = sc.take<int32_t>(C);
  rc = sc.alloc();
  if (rc) return rc;
  rc = exmc_hip_advi(m, o, n_fits, chain_lo, draws ? sc.dev(s_draws) : nullptr, sc.dev(s_mu), sc.dev(s_ls),
                     elbo_history ? sc.dev(s_hist) : nullptr, sc.dev(s_iters), sc.dev(s_conv));
  if (!rc) rc = sc.download();
  if (rc) return rc;
  if (draws) transpose_trace_vec(sc.host(s_draws), draws, o.num_draws, m->d, n_fits);
  fits_first(sc.host(s_hist), elbo_history, I, C);
  fits_first(sc.host(s_mu), mu, d, C);
  fits_first(sc.host(s_ls), log_sigma, d, C);
  fits_first(sc.host(s_iters), num_iters, 1, C);
  fits_first(sc.host(s_conv), converged, 1, C);
  return EXMC_OK;
}

}  // extern "C"

// ---- SMC and its bridged mode (include/exmc_hip_smc.h, exmc_hip_smc_bridge.h; exmc_smc.hpp) ------------------
namespace {

int smc_max_stages(const exmc_hip_smc_opts& o) { return o.max_stages > 0 ? o.max_stages : EXMC_SMC_DEFAULT_MAX_STAGES; }

int smc_opts_check(const exmc_hip_smc_opts& o, int n_runs, int run_lo) {
  if (o.num_particles < 1 || o.num_mh_steps < 1 || !std::isfinite(o.threshold_ratio) || o.max_stages < 0)
    return fail(EXMC_ERR_BADARG, "smc: num_particles >= 1, num_mh_steps >= 1, threshold_ratio finite and max_stages >= 0");
  if (n_runs < 1 || run_lo < 0 || (long long)n_runs * o.num_particles > 0x7FFFFFFFLL)
    return fail(EXMC_ERR_BADARG, "smc: bad arguments");
  return EXMC_OK;
}

int smc_state_check(const exmc_hip_smc_state& s, const void* q, const void* logp) {
  if (!q || !logp || !s.beta || !s.run_rng || !s.active || !s.scale || !s.accept || !s.betas || !s.ess_history ||
      !s.acceptance_rates || !s.num_stages || !s.status || !s.active_count)
    return fail(EXMC_ERR_BADARG, "smc: the arrays of the state are all required");
  return EXMC_OK;
}

SmcRuns smc_runs(const exmc_hip_smc_state& s) {
  return SmcRuns{s.beta, s.run_rng, s.active, s.scale, s.accept, s.betas, s.ess_history, s.acceptance_rates,
                 s.num_stages, s.status, s.active_count};
}

SmcParams smc_params(exmc_hip_model* m, const exmc_hip_smc_opts& o, int n_runs, int run_lo, double* q, double* logp,
                     uint64_t* words, const exmc_hip_smc_state& st) {
  SmcParams P;
  P.n_chains = n_runs * o.num_particles;
  P.n_particles = o.num_particles;
  P.n_runs = n_runs;
  P.run_lo = run_lo;
  P.base_seed = o.seed;
  P.num_mh_steps = o.num_mh_steps;
  P.max_stages = smc_max_stages(o);
  P.q = q;
  P.logp = logp;
  P.words = words;
  P.runs = smc_runs(st);
  P.rng = rng_args(m);
  P.flat = flat_order(m);
  return P;
}

// smc_init_kernel or smc_mutate_kernel of the handle's layout on its stream, with `B` their bridged siblings;
// the caller records the events
template <bool kInit>
int smc_model_launch(exmc_hip_model* m, int lanes, const SmcParams& P, const SmcBridge* B = nullptr) {
  return dispatch(m, lanes, [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    const size_t xlds = aux_lds_bytes<typename T::M>();
    if (B) {
      if constexpr (kInit) {
        EXMC_KLAUNCH(m->device, (smc_bridge_init_kernel<typename T::M, T::G>), grid_for(P.n_chains, T::G, kBlock),
                     dim3(kBlock), xlds, m->stream, P, *B, mc);
      } else {
        EXMC_KLAUNCH(m->device, (smc_bridge_mutate_kernel<typename T::M, T::G>), grid_for(P.n_chains, T::G, kBlock),
                     dim3(kBlock), xlds, m->stream, P, *B, mc);
      }
    } else if constexpr (kInit) {
      EXMC_KLAUNCH(m->device, (smc_init_kernel<typename T::M, T::G>), grid_for(P.n_chains, T::G, kBlock), dim3(kBlock),
                   xlds, m->stream, P, mc);
    } else {
      EXMC_KLAUNCH(m->device, (smc_mutate_kernel<typename T::M, T::G>), grid_for(P.n_chains, T::G, kBlock), dim3(kBlock),
                   xlds, m->stream, P, mc);
    }
    HIP_TRY(hipGetLastError());
    return (int)EXMC_OK;
  });
}

#ifndef EXMC_ONLY_CUSTOM
// the scratch of the model-free front of a stage, one allocation
struct SmcScratch {
  CallBuf buf;
  int n_blocks = 0;
  double *nw = nullptr, *rcum = nullptr, *tot = nullptr, *base = nullptr, *q2 = nullptr, *lp2 = nullptr, *lb2 = nullptr;
  int32_t *resample = nullptr, *idx = nullptr;
  int alloc(int N, int R, int d, bool bridge = false) {
    const size_t C = (size_t)N * R;
    n_blocks = (N + kRatioScan - 1) / kRatioScan;
    const size_t n_tot = (size_t)n_blocks * R, n_base = ((size_t)n_blocks + 1) * R;
    const size_t doubles = C + C + n_tot + n_base + (size_t)d * C + C + (bridge ? C : 0);
    int rc = buf.alloc(doubles * 8 + ((size_t)R + C) * 4);
    if (rc) return rc;
    nw = buf.as<double>();
    rcum = nw + C;
    tot = rcum + C;
    base = tot + n_tot;
    q2 = base + n_base;
    lp2 = q2 + (size_t)d * C;
    lb2 = lp2 + C;
    resample = (int32_t*)(lb2 + (bridge ? C : 0));
    idx = resample + R;
    return EXMC_OK;
  }
};

// exmc_hip_smc_reweight's launches for one stage; with `B` exmc_hip_smc_bridge_reweight's
int smc_stage_launch(hipStream_t stream, const SmcScratch& sc, const exmc_hip_smc_opts& o, int n_runs, int d, int stage,
                     double* q, double* logp, const SmcRuns& runs, const SmcBridge* B = nullptr) {
  const int N = o.num_particles, R = n_runs, max_stages = smc_max_stages(o);
  const long long C = (long long)N * R;
  const SmcStage S{N, R, stage, max_stages, o.num_mh_steps, o.threshold_ratio * (double)N, d, std::sqrt((double)d), runs};
  hipLaunchKernelGGL(smc_close_kernel, dim3(1), dim3(kSmcBlock), 0, stream, S);
  HIP_TRY(hipGetLastError());
  if (stage >= max_stages) return EXMC_OK;
  if (B && N <= kSmcLdsParticles)
    hipLaunchKernelGGL(smc_bridge_weights_kernel<true>, dim3((unsigned)R), dim3(kSmcBlock), (size_t)N * 8, stream, S, logp,
                       *B, sc.nw, sc.resample);
  else if (B)
    hipLaunchKernelGGL(smc_bridge_weights_kernel<false>, dim3((unsigned)R), dim3(kSmcBlock), 0, stream, S, logp, *B, sc.nw,
                       sc.resample);
  else if (N <= kSmcLdsParticles)
    hipLaunchKernelGGL(smc_weights_kernel<true>, dim3((unsigned)R), dim3(kSmcBlock), (size_t)N * 8, stream, S, logp, sc.nw,
                       sc.resample);
  else
    hipLaunchKernelGGL(smc_weights_kernel<false>, dim3((unsigned)R), dim3(kSmcBlock), 0, stream, S, logp, sc.nw,
                       sc.resample);
  HIP_TRY(hipGetLastError());
  const long long lanes = (long long)R * sc.n_blocks;
  hipLaunchKernelGGL(ratio_scan_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, sc.nw, 1, R, N,
                     sc.n_blocks, 1, sc.rcum, sc.tot);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(smc_resample_kernel, dim3((unsigned)R), dim3(kSmcBlock), 0, stream, S, sc.rcum, sc.tot, sc.base,
                     sc.n_blocks, sc.resample, sc.idx);
  HIP_TRY(hipGetLastError());
  const long long total = ((long long)d + (B ? 2 : 1)) * C;
  hipLaunchKernelGGL(smc_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, q, logp,
                     B ? B->logb : nullptr, sc.idx, d, N, C, sc.q2, sc.lp2, B ? sc.lb2 : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(q, sc.q2, (size_t)d * C * 8, hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipMemcpyAsync(logp, sc.lp2, (size_t)C * 8, hipMemcpyDeviceToDevice, stream));
  if (B) HIP_TRY(hipMemcpyAsync(B->logb, sc.lb2, (size_t)C * 8, hipMemcpyDeviceToDevice, stream));
  hipLaunchKernelGGL(smc_scale_kernel, dim3((unsigned)R, (unsigned)d), dim3(kSmcBlock), 0, stream, S, q, C);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}
#endif


// ---- the bridged mode's arguments (include/exmc_hip_smc_bridge.h) ----
// the base read back and checked: finite mu, finite sigma > 0
int smc_base_check(const double* mu_dev, const double* sigma_dev, int d) {
  std::vector<double> h((size_t)d);
  for (const double* a : {mu_dev, sigma_dev}) {
    if (!a) continue;
    HIP_TRY(hipMemcpy(h.data(), a, (size_t)d * 8, hipMemcpyDeviceToHost));
    for (double v : h)
      if (!std::isfinite(v) || (a == sigma_dev && !(v > 0.0)))
        return fail(EXMC_ERR_BADARG, "smc bridge: the base needs finite mu and finite sigma > 0");
  }
  return EXMC_OK;
}

SmcBridge smc_bridge(int d, const double* mu, const double* sigma, double* logb, double* log_evidence, double* steps) {
  return SmcBridge{mu, sigma, 0.5 * d * std::log(2.0 * M_PI), logb, log_evidence, steps};
}

int smc_bridge_check(const double* logb, const double* log_evidence, const double* steps) {
  if (!logb || !log_evidence || !steps)
    return fail(EXMC_ERR_BADARG, "smc bridge: logb, log_evidence and log_evidence_steps are required");
  return EXMC_OK;
}

// exmc_hip_smc_init / _mutate and their bridged forms (B)
template <bool kInit>
int smc_model_step(exmc_hip_model* m, const exmc_hip_smc_opts& o, int n_runs, int run_lo, double* q_dev, double* logp_dev,
                   uint64_t* rng_words_dev, const exmc_hip_smc_state& st, const SmcBridge* B) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  int rc = smc_opts_check(o, n_runs, run_lo);
  if (!rc) rc = smc_state_check(st, q_dev, logp_dev);
  if (!rc && !rng_words_dev) rc = fail(EXMC_ERR_BADARG, "smc: the arrays of the state are all required");
  if (!rc && B && kInit) rc = smc_bridge_check(B->logb, B->log_evidence, B->log_evidence_steps);
  if (!rc && B && !B->logb) rc = fail(EXMC_ERR_BADARG, "smc bridge: logb is required");   // the mutation writes no evidence
  if (rc) return rc;
  HIP_TRY(hipSetDevice(m->device));
  if (B && kInit) {
    rc = smc_base_check(B->mu, B->sigma, m->d);
    if (rc) return rc;
  }
  const SmcParams P = smc_params(m, o, n_runs, run_lo, q_dev, logp_dev, rng_words_dev, st);
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  rc = smc_model_launch<kInit>(m, resolve_lanes(m, o.lanes_per_chain), P, B);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);   // waits for the launch
}

int smc_reweight(int device, const exmc_hip_smc_opts& o, int n_runs, int d, int stage, double* q_dev, double* logp_dev,
                 const exmc_hip_smc_state& st, const SmcBridge* B) {
  int rc = smc_opts_check(o, n_runs, 0);
  if (!rc) rc = smc_state_check(st, q_dev, logp_dev);
  if (!rc && B) rc = smc_bridge_check(B->logb, B->log_evidence, B->log_evidence_steps);
  if (!rc && (d < 1 || stage < 0 || stage > smc_max_stages(o))) rc = fail(EXMC_ERR_BADARG, "smc: bad arguments");
  if (rc) return rc;
  rc = select_device(device);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  return fail(EXMC_ERR_UNSUPPORTED, "smc: use libexmc_hip.so for the model-free front of a stage");
#else
  SmcScratch sc;
  rc = sc.alloc(o.num_particles, n_runs, d, B != nullptr);
  if (!rc) rc = smc_stage_launch((hipStream_t)0, sc, o, n_runs, d, stage, q_dev, logp_dev, smc_runs(st), B);
  if (rc) {
    (void)hipStreamSynchronize((hipStream_t)0);   // the scratch is freed on return
    return rc;
  }
  HIP_TRY(hipStreamSynchronize((hipStream_t)0));
  return EXMC_OK;
#endif
}

// the outputs of a whole run, device or host; the last three are the bridged mode's
struct SmcOuts {
  double *particles, *logp, *betas, *ess_history, *acceptance_rates;
  int32_t *num_stages, *status;
  double *logb, *log_evidence, *log_evidence_steps;
};

#ifdef EXMC_ONLY_CUSTOM
const char* const kSmcPluginWhole = "smc: a generated model goes through exmc_hip_smc_init, exmc_hip_smc_mutate and "
                                    "libexmc_hip.so's exmc_hip_smc_reweight, or their bridged forms";
#endif

// exmc_hip_smc, and exmc_hip_smc_bridge with `base` (its mu, sigma and log_norm; the arrays come from `out`)
int smc_whole(exmc_hip_model* m, const exmc_hip_smc_opts& o, int n_runs, int run_lo, const SmcOuts& out,
              const SmcBridge* base) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  int rc = smc_opts_check(o, n_runs, run_lo);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)out; (void)base;
  return fail(EXMC_ERR_UNSUPPORTED, kSmcPluginWhole);
#else
  HIP_TRY(hipSetDevice(m->device));
  if (base) {
    rc = smc_base_check(base->mu, base->sigma, m->d);
    if (rc) return rc;
  }
  const int lanes = resolve_lanes(m, o.lanes_per_chain);
  const int N = o.num_particles, R = n_runs, d = m->d, max_stages = smc_max_stages(o);
  const size_t C = (size_t)N * R, H = (size_t)max_stages * R;
  // the state of the runs, and whatever the caller wants none of: scratch of the call
  CallBuf own;
  const size_t n_q = out.particles ? 0 : (size_t)d * C, n_lp = out.logp ? 0 : C;
  const size_t n_b = out.betas ? 0 : H, n_e = out.ess_history ? 0 : H, n_a = out.acceptance_rates ? 0 : H;
  const size_t n_lb = (base && !out.logb) ? C : 0, n_le = (base && !out.log_evidence) ? (size_t)R : 0;
  const size_t n_les = (base && !out.log_evidence_steps) ? H : 0;
  const size_t words8 = n_q + n_lp + n_b + n_e + n_a + n_lb + n_le + n_les + 2 * C + (size_t)R + 2 * (size_t)R + (size_t)d * R;
  rc = own.alloc(words8 * 8 + ((size_t)R + C + R + R + 1) * 4);
  if (rc) return rc;
  double* p = own.as<double>();
  auto take8 = [&](size_t n) { double* r = p; p += n; return r; };
  double* q = out.particles ? out.particles : take8(n_q);
  double* lp = out.logp ? out.logp : take8(n_lp);
  exmc_hip_smc_state st;
  st.betas = out.betas ? out.betas : take8(n_b);
  st.ess_history = out.ess_history ? out.ess_history : take8(n_e);
  st.acceptance_rates = out.acceptance_rates ? out.acceptance_rates : take8(n_a);
  SmcBridge bridge{};
  if (base) {
    bridge = *base;
    bridge.logb = out.logb ? out.logb : take8(n_lb);
    bridge.log_evidence = out.log_evidence ? out.log_evidence : take8(n_le);
    bridge.log_evidence_steps = out.log_evidence_steps ? out.log_evidence_steps : take8(n_les);
  }
  const SmcBridge* B = base ? &bridge : nullptr;
  uint64_t* words = (uint64_t*)take8(2 * C);
  st.beta = take8(R);
  st.run_rng = (uint64_t*)take8(2 * (size_t)R);
  st.scale = take8((size_t)d * R);
  int32_t* ip = (int32_t*)p;
  st.active = ip;
  st.accept = ip + R;
  int32_t* own_ns = st.accept + C;
  int32_t* own_status = own_ns + R;
  st.active_count = own_status + R;
  st.num_stages = out.num_stages ? out.num_stages : own_ns;
  st.status = out.status ? out.status : own_status;
  SmcScratch sc;
  rc = sc.alloc(N, R, d, base != nullptr);
  if (rc) return rc;
  const SmcParams P = smc_params(m, o, n_runs, run_lo, q, lp, words, st);
  const SmcRuns runs = smc_runs(st);
  float total_ms = 0.f;
  auto run = [&]() -> int {
    HIP_TRY(hipEventRecord(m->ev0, m->stream));
    int rc2 = smc_model_launch<true>(m, lanes, P, B);
    if (rc2) return rc2;
    for (int stage = 0;; stage++) {   // the front at stage == max_stages only closes: its count is 0
      rc2 = smc_stage_launch(m->stream, sc, o, n_runs, d, stage, q, lp, runs, B);
      if (rc2) return rc2;
      int32_t count = 0;
      HIP_TRY(hipMemcpyAsync(&count, st.active_count, 4, hipMemcpyDeviceToHost, m->stream));
      HIP_TRY(hipEventRecord(m->ev1, m->stream));
      HIP_TRY(hipEventSynchronize(m->ev1));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, m->ev0, m->ev1));
      total_ms += ms;
      if (count == 0 || stage >= max_stages) return EXMC_OK;
      HIP_TRY(hipEventRecord(m->ev0, m->stream));
      rc2 = smc_model_launch<false>(m, lanes, P, B);
      if (rc2) return rc2;
    }
  };
  rc = run();
  (void)hipStreamSynchronize(m->stream);   // before the scratch is freed
  if (rc) return rc;
  m->last_ms = total_ms;
  return EXMC_OK;
#endif
}

// exmc_hip_smc_host, and exmc_hip_smc_bridge_host with `bridge`: mu and sigma are host arrays [d] or null
int smc_whole_host(exmc_hip_model* m, const exmc_hip_smc_opts& o, int n_runs, int run_lo, const SmcOuts& out,
                   bool bridge, const double* mu, const double* sigma) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  int rc = smc_opts_check(o, n_runs, run_lo);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)out; (void)bridge; (void)mu; (void)sigma;
  return fail(EXMC_ERR_UNSUPPORTED, kSmcPluginWhole);
#else
  HIP_TRY(hipSetDevice(m->device));
  const size_t R = (size_t)n_runs, C = R * (size_t)o.num_particles, d = (size_t)m->d;
  const size_t H = (size_t)smc_max_stages(o);
  Scratch sc;
  const auto s_q = sc.take<double>(out.particles ? d * C : 0);   // [d][C]
  const auto s_lp = sc.take<double>(out.logp ? C : 0);
  const auto s_b = sc.take<double>(out.betas ? H * R : 0), s_e = sc.take<double>(out.ess_history ? H * R : 0);
  const auto s_a = sc.take<double>(out.acceptance_rates ? H * R : 0);
  const auto s_lb = sc.take<double>(out.logb ? C : 0), s_le = sc.take<double>(out.log_evidence ? R : 0);
  const auto s_les = sc.take<double>(out.log_evidence_steps ? H * R : 0);
  const auto s_ns = sc.take<int32_t>(R), s_st = sc.take<int32_t>(R);
  rc = sc.alloc();
  if (rc) return rc;
  CallBuf base_buf;
  SmcBridge base = smc_bridge(m->d, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (bridge && (mu || sigma)) {
    rc = base_buf.alloc(2 * d * 8);
    if (rc) return rc;
    if (mu) {
      HIP_TRY(hipMemcpy(base_buf.as<double>(), mu, d * 8, hipMemcpyHostToDevice));
      base.mu = base_buf.as<double>();
    }
    if (sigma) {
      HIP_TRY(hipMemcpy(base_buf.as<double>() + d, sigma, d * 8, hipMemcpyHostToDevice));
      base.sigma = base_buf.as<double>() + d;
    }
  }
  const SmcOuts dev{out.particles ? sc.dev(s_q) : nullptr, out.logp ? sc.dev(s_lp) : nullptr,
                    out.betas ? sc.dev(s_b) : nullptr, out.ess_history ? sc.dev(s_e) : nullptr,
                    out.acceptance_rates ? sc.dev(s_a) : nullptr, sc.dev(s_ns), sc.dev(s_st),
                    out.logb ? sc.dev(s_lb) : nullptr, out.log_evidence ? sc.dev(s_le) : nullptr,
                    out.log_evidence_steps ? sc.dev(s_les) : nullptr};
  rc = smc_whole(m, o, n_runs, run_lo, dev, bridge ? &base : nullptr);
  if (!rc) rc = sc.download();
  if (rc) return rc;
  fits_first(sc.host(s_q), out.particles, d, C);   // [d][C] -> [R][N][d]
  if (out.logp) std::copy(sc.host(s_lp), sc.host(s_lp) + C, out.logp);
  fits_first(sc.host(s_b), out.betas, H, R);
  fits_first(sc.host(s_e), out.ess_history, H, R);
  fits_first(sc.host(s_a), out.acceptance_rates, H, R);
  fits_first(sc.host(s_ns), out.num_stages, 1, R);
  fits_first(sc.host(s_st), out.status, 1, R);
  if (out.logb) std::copy(sc.host(s_lb), sc.host(s_lb) + C, out.logb);
  if (out.log_evidence) std::copy(sc.host(s_le), sc.host(s_le) + R, out.log_evidence);
  fits_first(sc.host(s_les), out.log_evidence_steps, H, R);
  return EXMC_OK;
#endif
}

}  // namespace

extern "C" {

int exmc_hip_smc_init(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, double* q_dev,
                      double* logp_dev, uint64_t* rng_words_dev, exmc_hip_smc_state st) {
  return smc_model_step<true>(m, o, n_runs, run_lo, q_dev, logp_dev, rng_words_dev, st, nullptr);
}

int exmc_hip_smc_mutate(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, double* q_dev, double* logp_dev,
                        uint64_t* rng_words_dev, exmc_hip_smc_state st) {
  return smc_model_step<false>(m, o, n_runs, 0, q_dev, logp_dev, rng_words_dev, st, nullptr);
}

int exmc_hip_smc_reweight(int device, exmc_hip_smc_opts o, int n_runs, int d, int stage, double* q_dev,
                          double* logp_dev, exmc_hip_smc_state st) {
  return smc_reweight(device, o, n_runs, d, stage, q_dev, logp_dev, st, nullptr);
}

int exmc_hip_smc(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, double* particles_dev,
                 double* logp_dev, double* betas_dev, double* ess_history_dev, double* acceptance_rates_dev,
                 int32_t* num_stages_dev, int32_t* status_dev) {
  return smc_whole(m, o, n_runs, run_lo,
                   SmcOuts{particles_dev, logp_dev, betas_dev, ess_history_dev, acceptance_rates_dev, num_stages_dev,
                           status_dev, nullptr, nullptr, nullptr},
                   nullptr);
}

int exmc_hip_smc_host(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, double* particles,
                      double* logp, double* betas, double* ess_history, double* acceptance_rates,
                      int32_t* num_stages, int32_t* status) {
  return smc_whole_host(m, o, n_runs, run_lo,
                        SmcOuts{particles, logp, betas, ess_history, acceptance_rates, num_stages, status, nullptr,
                                nullptr, nullptr},
                        false, nullptr, nullptr);
}

int exmc_hip_smc_bridge_init(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, const double* mu_dev,
                             const double* sigma_dev, double* q_dev, double* logp_dev, double* logb_dev,
                             uint64_t* rng_words_dev, exmc_hip_smc_state st, double* log_evidence_dev,
                             double* log_evidence_steps_dev) {
  const SmcBridge B = smc_bridge(m ? m->d : 0, mu_dev, sigma_dev, logb_dev, log_evidence_dev, log_evidence_steps_dev);
  return smc_model_step<true>(m, o, n_runs, run_lo, q_dev, logp_dev, rng_words_dev, st, &B);
}

int exmc_hip_smc_bridge_mutate(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, const double* mu_dev,
                               const double* sigma_dev, double* q_dev, double* logp_dev, double* logb_dev,
                               uint64_t* rng_words_dev, exmc_hip_smc_state st) {
  const SmcBridge B = smc_bridge(m ? m->d : 0, mu_dev, sigma_dev, logb_dev, nullptr, nullptr);
  return smc_model_step<false>(m, o, n_runs, 0, q_dev, logp_dev, rng_words_dev, st, &B);
}

int exmc_hip_smc_bridge_reweight(int device, exmc_hip_smc_opts o, int n_runs, int d, int stage, double* q_dev,
                                 double* logp_dev, double* logb_dev, exmc_hip_smc_state st, double* log_evidence_dev,
                                 double* log_evidence_steps_dev) {
  const SmcBridge B = smc_bridge(d, nullptr, nullptr, logb_dev, log_evidence_dev, log_evidence_steps_dev);
  return smc_reweight(device, o, n_runs, d, stage, q_dev, logp_dev, st, &B);
}

int exmc_hip_smc_bridge(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, const double* mu_dev,
                        const double* sigma_dev, double* particles_dev, double* logp_dev, double* logb_dev,
                        double* betas_dev, double* ess_history_dev, double* acceptance_rates_dev,
                        int32_t* num_stages_dev, int32_t* status_dev, double* log_evidence_dev,
                        double* log_evidence_steps_dev) {
  const SmcBridge base = smc_bridge(m ? m->d : 0, mu_dev, sigma_dev, nullptr, nullptr, nullptr);
  return smc_whole(m, o, n_runs, run_lo,
                   SmcOuts{particles_dev, logp_dev, betas_dev, ess_history_dev, acceptance_rates_dev, num_stages_dev,
                           status_dev, logb_dev, log_evidence_dev, log_evidence_steps_dev},
                   &base);
}

int exmc_hip_smc_bridge_host(exmc_hip_model* m, exmc_hip_smc_opts o, int n_runs, int run_lo, const double* mu,
                             const double* sigma, double* particles, double* logp, double* logb, double* betas,
                             double* ess_history, double* acceptance_rates, int32_t* num_stages, int32_t* status,
                             double* log_evidence, double* log_evidence_steps) {
  return smc_whole_host(m, o, n_runs, run_lo,
                        SmcOuts{particles, logp, betas, ess_history, acceptance_rates, num_stages, status, logb,
                                log_evidence, log_evidence_steps},
                        true, mu, sigma);
}

}  // extern "C"

// ---- importance diagnostics of the fits (include/exmc_hip_fit_psis.h; exmc_fit_psis.hpp, exmc_psis_ratio.hpp) ----
namespace {

int fit_lr_check(exmc_hip_model* m, const void* draws, const void* mu, const void* scale, int scale_kind, int n_draws,
                 int d, int n_fits) {
  if (check_model(m)) return EXMC_ERR_BADARG;
  if (!draws || !mu || !scale || (scale_kind != EXMC_FIT_SIGMA && scale_kind != EXMC_FIT_LOG_SIGMA) || n_draws < 1 ||
      n_fits < 1 || d != m->d)
    return fail(EXMC_ERR_BADARG, "fit psis: bad arguments");
  return EXMC_OK;
}

// fit_log_ratio_kernel of the handle's layout on its stream; the caller records the events
int fit_lr_launch(exmc_hip_model* m, const double* draws, const double* mu, const double* scale, int scale_kind,
                  int n_draws, int n_fits, int lanes_per_chain, double* lr, double* logp) {
  static_assert(EXMC_FIT_SIGMA == kFitSigma && EXMC_FIT_LOG_SIGMA == kFitLogSigma, "the header states the kernel's kinds");
  FitLogRatioParams P;
  P.draws = draws;
  P.mu = mu;
  P.scale = scale;
  P.scale_kind = scale_kind;
  P.n_draws = n_draws;
  P.n_fits = n_fits;
  P.log_norm = 0.5 * m->d * std::log(2.0 * M_PI);
  P.lr = lr;
  P.logp = logp;
  return dispatch(m, resolve_lanes(m, lanes_per_chain), [&](auto tag, const auto& mc) {
    using T = decltype(tag);
    const size_t xlds = aux_lds_bytes<typename T::M>();
    EXMC_KLAUNCH(m->device, (fit_log_ratio_kernel<typename T::M, T::G>), grid_for(n_fits, T::G, kBlock), dim3(kBlock),
                 xlds, m->stream, P, mc);
    HIP_TRY(hipGetLastError());
    return (int)EXMC_OK;
  });
}

int ratio_check(const void* lr, int n_draws, int n_fits, int pooled, int n_resample, const void* out,
                const void* idx) {
  if (!lr || !out || n_draws < 1 || n_fits < 1 || n_resample < 0 || (n_resample > 0 && !idx))
    return fail(EXMC_ERR_BADARG, "fit psis: bad arguments");
  if (pooled && (long long)n_draws * n_fits > 0x7FFFFFFFLL)
    return fail(EXMC_ERR_BADARG, "fit psis: more than 2^31 - 1 pooled samples");
  return EXMC_OK;
}

#ifndef EXMC_ONLY_CUSTOM
// the scratch of the smoothing and the resampling of lr[S][F] in one view, and their launches
struct RatioScratch {
  PsisScratch ps;
  CallBuf l1, xs, r, tot, base;
  int S = 0, Nb = 0, C = 0, n_blocks = 0;
  // the view; `need_xs`: no caller's lw to hold the smoothed values, and the resampling reads them
  int alloc(int n_draws, int n_fits, int pooled, int n_resample, bool need_xs) {
    S = n_draws;
    Nb = pooled ? 1 : n_fits;
    C = pooled ? n_fits : 1;
    const long long n = (long long)S * C;
    n_blocks = (int)((n + kRatioScan - 1) / kRatioScan);
    static_assert(kRatioFields <= kPsisFields, "the chunk states fit PsisScratch::part");
    int rc = ps.alloc(S, C, Nb);
    if (!rc) rc = l1.alloc((size_t)Nb * 8);
    if (!rc && need_xs) rc = xs.alloc((size_t)S * n_fits * 8);
    if (!rc && n_resample > 0) rc = r.alloc((size_t)S * n_fits * 8);
    if (!rc && n_resample > 0) rc = tot.alloc((size_t)n_blocks * Nb * 8);
    if (!rc && n_resample > 0) rc = base.alloc(((size_t)n_blocks + 1) * Nb * 8);
    if (rc) return rc;
    if (ps.P <= kPsisLdsPairs && psis_tail_lds_bytes(ps.P) > 40 * 1024)   // as PsisScratch::alloc, for this instantiation
      EXMC_KMAXLDS((psis_tail_kernel<true, true>), psis_tail_lds_bytes(ps.P));
    return EXMC_OK;
  }
};

int ratio_launch(hipStream_t stream, const RatioScratch& sc, const double* lr, int n_resample, uint64_t seed,
                 double* out, double* lw, int32_t* idx) {
  const int S = sc.S, Nb = sc.Nb, C = sc.C;
  const long long n = (long long)S * C, total = n * Nb;
  const PsisTables t = psis_tables(sc.ps);
  const IcGrid g = sc.ps.g;
  double* part = sc.ps.part.as<double>();
  double* x = lw ? lw : sc.xs.as<double>();   // null: nobody reads the weights
  int rc = psis_tails<true>(stream, t, lr, S, Nb, C);
  if (rc) return rc;
  hipLaunchKernelGGL(ratio_weights_kernel, dim3((unsigned)g.n_chunks, (unsigned)g.yblocks), dim3(g.block), 0, stream,
                     lr, S, Nb, C, g.chunk, t.P, t.keys, t.idx, t.xs, t.meta, part, x);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ratio_merge_kernel, dim3((unsigned)((Nb + 255) / 256)), dim3(256), 0, stream, part, g.n_chunks, n,
                     Nb, t.meta, out, sc.l1.as<double>());
  HIP_TRY(hipGetLastError());
  if (!x) return EXMC_OK;
  hipLaunchKernelGGL(ratio_normalise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, total, Nb,
                     C, sc.l1.as<double>());
  HIP_TRY(hipGetLastError());
  if (n_resample < 1) return EXMC_OK;
  const long long lanes = (long long)Nb * sc.n_blocks;
  hipLaunchKernelGGL(ratio_scan_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, x, S, Nb, C,
                     sc.n_blocks, 0, sc.r.as<double>(), sc.tot.as<double>());
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ratio_resample_kernel, dim3((unsigned)Nb), dim3(kRatioBlock), 0, stream, sc.r.as<double>(),
                     sc.tot.as<double>(), sc.base.as<double>(), S, Nb, C, sc.n_blocks, n_resample, seed,
                     sc.l1.as<double>(), idx);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}

int gather_launch(hipStream_t stream, const double* draws, const int32_t* idx, int n_draws, int d, int n_fits,
                  int pooled, int n_resample, double* out) {
  const long long total = (long long)n_resample * d * (pooled ? 1 : n_fits);
  hipLaunchKernelGGL(ratio_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, draws, idx,
                     n_draws, d, n_fits, pooled ? 1 : 0, n_resample, out);
  HIP_TRY(hipGetLastError());
  return EXMC_OK;
}
#endif

}  // namespace

extern "C" {

int exmc_hip_fit_log_ratio(exmc_hip_model* m, const double* draws_dev, const double* mu_dev, const double* scale_dev,
                           int scale_kind, int n_draws, int d, int n_fits, int lanes_per_chain, double* lr_dev,
                           double* logp_dev) {
  int rc = fit_lr_check(m, draws_dev, mu_dev, scale_dev, scale_kind, n_draws, d, n_fits);
  if (rc) return rc;
  if (!lr_dev) return fail(EXMC_ERR_BADARG, "fit psis: bad arguments");
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  rc = fit_lr_launch(m, draws_dev, mu_dev, scale_dev, scale_kind, n_draws, n_fits, lanes_per_chain, lr_dev, logp_dev);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);   // waits for the launch
}

int exmc_hip_ratio_psis_from_lr(int device, const double* lr_dev, int n_draws, int n_fits, int pooled, int n_resample,
                                uint64_t seed, double* out_dev, double* lw_dev, int32_t* idx_dev) {
  int rc = ratio_check(lr_dev, n_draws, n_fits, pooled, n_resample, out_dev, idx_dev);
  if (rc) return rc;
  rc = select_device(device);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)seed; (void)lw_dev;
  return fail(EXMC_ERR_UNSUPPORTED, "fit psis: use libexmc_hip.so for the model-free smoothing and resampling");
#else
  RatioScratch sc;
  rc = sc.alloc(n_draws, n_fits, pooled, n_resample, !lw_dev && n_resample > 0);
  if (!rc) rc = ratio_launch((hipStream_t)0, sc, lr_dev, n_resample, seed, out_dev, lw_dev, idx_dev);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)0));
  return EXMC_OK;
#endif
}

int exmc_hip_ratio_gather(int device, const double* draws_dev, const int32_t* idx_dev, int n_draws, int d, int n_fits,
                          int pooled, int n_resample, double* out_dev) {
  if (!draws_dev || !idx_dev || !out_dev || n_draws < 1 || d < 1 || n_fits < 1 || n_resample < 1)
    return fail(EXMC_ERR_BADARG, "fit psis: bad arguments");
  if (pooled && (long long)n_draws * n_fits > 0x7FFFFFFFLL)
    return fail(EXMC_ERR_BADARG, "fit psis: more than 2^31 - 1 pooled samples");
  int rc = select_device(device);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  return fail(EXMC_ERR_UNSUPPORTED, "fit psis: use libexmc_hip.so for the model-free smoothing and resampling");
#else
  rc = gather_launch((hipStream_t)0, draws_dev, idx_dev, n_draws, d, n_fits, pooled, n_resample, out_dev);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)0));
  return EXMC_OK;
#endif
}

int exmc_hip_fit_psis(exmc_hip_model* m, const double* draws_dev, const double* mu_dev, const double* scale_dev,
                      int scale_kind, int n_draws, int d, int n_fits, int lanes_per_chain, int pooled, int n_resample,
                      uint64_t seed, double* out_dev, double* lw_dev, int32_t* idx_dev, double* resampled_dev,
                      double* lr_dev, double* logp_dev) {
  int rc = fit_lr_check(m, draws_dev, mu_dev, scale_dev, scale_kind, n_draws, d, n_fits);
  if (rc) return rc;
  if (!out_dev || n_resample < 0) return fail(EXMC_ERR_BADARG, "fit psis: bad arguments");
  if (pooled && (long long)n_draws * n_fits > 0x7FFFFFFFLL)
    return fail(EXMC_ERR_BADARG, "fit psis: more than 2^31 - 1 pooled samples");
#ifdef EXMC_ONLY_CUSTOM
  (void)lanes_per_chain; (void)seed; (void)lw_dev; (void)idx_dev; (void)resampled_dev; (void)lr_dev; (void)logp_dev;
  return fail(EXMC_ERR_UNSUPPORTED, "fit psis: a generated model goes through exmc_hip_fit_log_ratio and "
              "libexmc_hip.so's exmc_hip_ratio_psis_from_lr");
#else
  HIP_TRY(hipSetDevice(m->device));
  const size_t G = pooled ? 1 : (size_t)n_fits;
  RatioScratch sc;
  CallBuf lr_own, idx_own;
  if (!lr_dev) {
    rc = lr_own.alloc((size_t)n_draws * n_fits * 8);
    if (rc) return rc;
    lr_dev = lr_own.as<double>();
  }
  if (n_resample > 0 && !idx_dev) {
    rc = idx_own.alloc((size_t)n_resample * G * 4);
    if (rc) return rc;
    idx_dev = idx_own.as<int32_t>();
  }
  rc = sc.alloc(n_draws, n_fits, pooled, n_resample, !lw_dev && n_resample > 0);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(m->ev0, m->stream));
  rc = fit_lr_launch(m, draws_dev, mu_dev, scale_dev, scale_kind, n_draws, n_fits, lanes_per_chain, lr_dev, logp_dev);
  if (!rc) rc = ratio_launch(m->stream, sc, lr_dev, n_resample, seed, out_dev, lw_dev, idx_dev);
  if (!rc && n_resample > 0 && resampled_dev)
    rc = gather_launch(m->stream, draws_dev, idx_dev, n_draws, d, n_fits, pooled, n_resample, resampled_dev);
  if (rc) {
    (void)hipStreamSynchronize(m->stream);   // the scratch is freed on return
    return rc;
  }
  HIP_TRY(hipEventRecord(m->ev1, m->stream));
  return finish_timing(m);   // waits for the launches: before the scratch is freed
#endif
}

int exmc_hip_fit_psis_host(exmc_hip_model* m, const double* draws, const double* mu, const double* scale,
                           int scale_kind, int n_draws, int d, int n_fits, int lanes_per_chain, int pooled,
                           int n_resample, uint64_t seed, double* out, double* lw, int32_t* idx, double* resampled,
                           double* lr, double* logp) {
  int rc = fit_lr_check(m, draws, mu, scale, scale_kind, n_draws, d, n_fits);
  if (rc) return rc;
  if (!out || n_resample < 0) return fail(EXMC_ERR_BADARG, "fit psis: bad arguments");
  if (pooled && (long long)n_draws * n_fits > 0x7FFFFFFFLL)
    return fail(EXMC_ERR_BADARG, "fit psis: more than 2^31 - 1 pooled samples");
#ifdef EXMC_ONLY_CUSTOM
  (void)lanes_per_chain; (void)seed; (void)lw; (void)idx; (void)resampled; (void)lr; (void)logp;
  return fail(EXMC_ERR_UNSUPPORTED, "fit psis: a generated model goes through exmc_hip_fit_log_ratio and "
              "libexmc_hip.so's exmc_hip_ratio_psis_from_lr");
#else
  HIP_TRY(hipSetDevice(m->device));
  const size_t C = (size_t)n_fits, D = (size_t)d, S = (size_t)n_draws, R = (size_t)n_resample;
  const size_t G = pooled ? 1 : C;
  Scratch sc;
  const auto s_mu = sc.take<double>(D * C), s_scale = sc.take<double>(D * C);
  const auto s_out = sc.take<double>((size_t)EXMC_FIT_PSIS_NOUT * G);
  const auto s_lw = sc.take<double>(S * C), s_lr = sc.take<double>(S * C), s_logp = sc.take<double>(S * C);
  const auto s_res = sc.take<double>(R * D * G);
  const auto s_idx = sc.take<int32_t>(R * G);
  rc = sc.alloc_with_trace(draws, n_draws, d, n_fits);
  if (rc) return rc;
  {
    std::vector<double> h(2 * D * C);   // [C][d] -> [d][C]
    for (size_t c = 0; c < C; c++)
      for (size_t i = 0; i < D; i++) {
        h[i * C + c] = mu[c * D + i];
        h[D * C + i * C + c] = scale[c * D + i];
      }
    HIP_TRY(hipMemcpy(sc.dev(s_mu), h.data(), h.size() * 8, hipMemcpyHostToDevice));
  }
  rc = exmc_hip_fit_psis(m, sc.trace(), sc.dev(s_mu), sc.dev(s_scale), scale_kind, n_draws, d, n_fits, lanes_per_chain,
                         pooled, n_resample, seed, sc.dev(s_out), sc.dev(s_lw), R ? sc.dev(s_idx) : nullptr,
                         R ? sc.dev(s_res) : nullptr, sc.dev(s_lr), sc.dev(s_logp));
  if (!rc) rc = sc.download();
  if (rc) return rc;
  std::copy(sc.host(s_out), sc.host(s_out) + (size_t)EXMC_FIT_PSIS_NOUT * G, out);
  fits_first(sc.host(s_lw), lw, S, C);
  fits_first(sc.host(s_lr), lr, S, C);
  fits_first(sc.host(s_logp), logp, S, C);
  if (R) {
    fits_first(sc.host(s_idx), idx, R, G);                                                 // [R][G] -> [G][R]
    if (resampled) transpose_trace_vec(sc.host(s_res), resampled, n_resample, d, (int)G);   // [R][d][G] -> [G][R][d]
  }
  return EXMC_OK;
#endif
}

// ---- posterior predictive (include/exmc_hip_predictive.h; predictive_kernel, exmc_predictive.hpp) ------
int exmc_hip_posterior_predictive(exmc_hip_model* m, exmc_hip_predictive_opts o, const double* draws_dev,
                                  int n_draws, int d, int n_chains, uint64_t* rng_state_dev, double* yrep_dev) {
  int rc = pp_check(m, "posterior predictive", o, draws_dev, n_draws, d, n_chains,
                    !yrep_dev || (o.resume && !rng_state_dev));
  if (rc) return rc;
#ifndef EXMC_ONLY_CUSTOM
  HIP_TRY(hipSetDevice(m->device));
  PredictiveParams P;
  pp_fill(P, m, o, draws_dev, n_draws, d, n_chains);
  P.yrep = yrep_dev;
  P.rng_state = rng_state_dev;
  P.resume = o.resume ? 1 : 0;
  rc = ic_with_src(m, [&](const auto& src) { return predictive_launch(m, src, P); });
#endif
  return rc;
}

int exmc_hip_posterior_predictive_host(exmc_hip_model* m, exmc_hip_predictive_opts o, const double* draws,
                                       int n_draws, int d, int n_chains, uint64_t* rng_state, double* yrep) {
  int rc = pp_check(m, "posterior predictive", o, draws, n_draws, d, n_chains, !yrep || (o.resume && !rng_state));
  if (rc) return rc;
#ifndef EXMC_ONLY_CUSTOM
  HIP_TRY(hipSetDevice(m->device));
  const size_t S = (size_t)n_draws, C = (size_t)n_chains, N = (size_t)ic_n_data(m);
  Scratch sc;
  const auto s_yrep = sc.take<double>(S * N * C);                // [S][N][C]
  const auto s_rng = sc.take<uint64_t>(rng_state ? 2 * C : 0);   // the generators [2][C]
  rc = sc.alloc_with_trace(draws, n_draws, d, n_chains);
  if (rc) return rc;
  if (rng_state && o.resume) HIP_TRY(hipMemcpy(sc.dev(s_rng), rng_state, 2 * C * 8, hipMemcpyHostToDevice));
  rc = exmc_hip_posterior_predictive(m, o, sc.trace(), n_draws, d, n_chains, rng_state ? sc.dev(s_rng) : nullptr,
                                     sc.dev(s_yrep));
  if (!rc) rc = sc.download();
  if (rc) return rc;
  transpose_trace_vec(sc.host(s_yrep), yrep, n_draws, (int)N, n_chains);
  if (rng_state) std::copy(sc.host(s_rng), sc.host(s_rng) + 2 * C, rng_state);
#endif
  return rc;
}

// ---- prior and prior predictive samples (include/exmc_hip_prior.h; prior_kernel, exmc_prior.hpp) -------
int exmc_hip_prior_samples(exmc_hip_model* m, exmc_hip_predictive_opts o, int n_draws, int n_chains,
                           uint64_t* rng_state_dev, double* x_dev, double* q_dev, double* yrep_dev) {
  int rc = prior_check(m, o, n_draws, n_chains, x_dev, q_dev, rng_state_dev);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)yrep_dev;
#else
  HIP_TRY(hipSetDevice(m->device));
  const std::vector<PriorEntry> prog = prior_program(m);
  if ((int)prog.size() != m->d) return fail(EXMC_ERR_UNSUPPORTED, "prior samples: this model kind has no prior walk");
  CallBuf dprog;
  rc = dprog.alloc(prog.size() * sizeof(PriorEntry));
  if (rc) return rc;
  HIP_TRY(hipMemcpy(dprog.p, prog.data(), prog.size() * sizeof(PriorEntry), hipMemcpyHostToDevice));
  PriorParams P;
  P.prog = dprog.as<PriorEntry>();
  P.x = x_dev;
  P.q = q_dev;
  P.yrep = yrep_dev;
  P.rng_state = rng_state_dev;
  P.S = n_draws;
  P.d = m->d;
  P.C = n_chains;
  P.N = ic_n_data(m);
  P.chain_lo = o.chain_lo;
  P.resume = o.resume ? 1 : 0;
  P.xwalk = (m->kind == EXMC_MODEL_SV_NCP) ? 100 : 0;
  P.base_seed = o.seed;
  P.rng = rng_args(m);
  rc = ic_with_src(m, [&](const auto& src) {
    using Src = std::decay_t<decltype(src)>;
    return pp_launch(m, prior_kernel<Src>, pp_lds_bytes(m->d), src, P);   // waits: before the program is freed
  });
#endif
  return rc;
}

int exmc_hip_prior_samples_host(exmc_hip_model* m, exmc_hip_predictive_opts o, int n_draws, int n_chains,
                                uint64_t* rng_state, double* x, double* q, double* yrep) {
  int rc = prior_check(m, o, n_draws, n_chains, x, q, rng_state);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)yrep;
#else
  HIP_TRY(hipSetDevice(m->device));
  const size_t S = (size_t)n_draws, C = (size_t)n_chains, d = (size_t)m->d, N = (size_t)ic_n_data(m);
  Scratch sc;
  const auto s_x = sc.take<double>(S * d * C), s_q = sc.take<double>(S * d * C);   // [S][d][C]
  const auto s_yrep = sc.take<double>(yrep ? S * N * C : 0);                       // [S][N][C]
  const auto s_rng = sc.take<uint64_t>(rng_state ? 2 * C : 0);                     // the generators [2][C]
  rc = sc.alloc();
  if (rc) return rc;
  if (rng_state && o.resume) HIP_TRY(hipMemcpy(sc.dev(s_rng), rng_state, 2 * C * 8, hipMemcpyHostToDevice));
  rc = exmc_hip_prior_samples(m, o, n_draws, n_chains, rng_state ? sc.dev(s_rng) : nullptr, sc.dev(s_x), sc.dev(s_q),
                              yrep ? sc.dev(s_yrep) : nullptr);
  if (!rc) rc = sc.download();
  if (rc) return rc;
  transpose_trace_vec(sc.host(s_x), x, n_draws, (int)d, n_chains);
  transpose_trace_vec(sc.host(s_q), q, n_draws, (int)d, n_chains);
  if (yrep) transpose_trace_vec(sc.host(s_yrep), yrep, n_draws, (int)N, n_chains);
  if (rng_state) std::copy(sc.host(s_rng), sc.host(s_rng) + 2 * C, rng_state);
#endif
  return rc;
}

// ---- posterior predictive checks (include/exmc_hip_ppc.h; ppc_kernel, exmc_ppc.hpp) -------------------
int exmc_hip_ppc(exmc_hip_model* m, exmc_hip_predictive_opts o, const double* draws_dev, int n_draws, int d,
                 int n_chains, double* datum_sums_dev, int64_t* datum_counts_dev, int32_t* chain_counts_dev,
                 double* tstat_dev, double* t_obs, double* m0, double* y_obs) {
  int rc = pp_check(m, "posterior predictive checks", o, draws_dev, n_draws, d, n_chains,
                    !(datum_sums_dev && datum_counts_dev && chain_counts_dev && t_obs && m0) || o.resume);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)tstat_dev; (void)y_obs;
#else
  HIP_TRY(hipSetDevice(m->device));
  PpcParams P;
  pp_fill(P, m, o, draws_dev, n_draws, d, n_chains);
  P.datum_sums = datum_sums_dev;
  P.datum_counts = (long long*)datum_counts_dev;
  P.chain_counts = (int*)chain_counts_dev;
  P.tstat = tstat_dev;
  std::vector<double> y((size_t)P.N);
  rc = ic_with_src(m, [&](const auto& src) { return ppc_launch(m, src, P, y.data()); });
  if (rc) return rc;
  for (int k = 0; k < kPpcStats; k++) t_obs[k] = P.t_obs[k];
  *m0 = P.m0;
  if (y_obs) std::copy(y.begin(), y.end(), y_obs);
#endif
  return rc;
}

int exmc_hip_ppc_host(exmc_hip_model* m, exmc_hip_predictive_opts o, const double* draws, int n_draws, int d,
                      int n_chains, double* datum, double* t_obs, double* p_value, double* tstat) {
  int rc = pp_check(m, "posterior predictive checks", o, draws, n_draws, d, n_chains,
                    !(datum && t_obs && p_value) || o.resume);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)tstat;
#else
  HIP_TRY(hipSetDevice(m->device));
  const size_t S = (size_t)n_draws, C = (size_t)n_chains, N = (size_t)ic_n_data(m);
  const size_t B = (C + kPpBlock - 1) / kPpBlock;
  Scratch sc;
  const auto s_sums = sc.take<double>(2 * B * N);                       // [B][N][2]
  const auto s_counts = sc.take<int64_t>(2 * B * N);                    // [B][N][2]
  const auto s_ts = sc.take<double>(tstat ? S * kPpcStats * C : 0);     // [S][4][C] where it is asked for
  const auto s_cc = sc.take<int32_t>(kPpcStats * C);                    // [4][C]
  rc = sc.alloc_with_trace(draws, n_draws, d, n_chains);
  if (rc) return rc;
  std::vector<double> y(N);
  double m0 = 0.0;
  rc = exmc_hip_ppc(m, o, sc.trace(), n_draws, d, n_chains, sc.dev(s_sums), sc.dev(s_counts), sc.dev(s_cc),
                    tstat ? sc.dev(s_ts) : nullptr, t_obs, &m0, y.data());
  if (!rc) rc = sc.download();
  if (rc) return rc;
  const double* sums = sc.host(s_sums);
  const int64_t* counts = sc.host(s_counts);
  const int32_t* cc = sc.host(s_cc);
  // the blocks left to right, then the finished numbers (include/exmc_hip_ppc.h)
  const double n = (double)(S * C);
  for (size_t i = 0; i < N; i++) {
    double E = 0.0, E2 = 0.0;
    int64_t n_lt = 0, n_eq = 0;
    for (size_t b = 0; b < B; b++) {
      E = E + sums[(b * N + i) * 2];
      E2 = E2 + sums[(b * N + i) * 2 + 1];
      n_lt += counts[(b * N + i) * 2];
      n_eq += counts[(b * N + i) * 2 + 1];
    }
    datum[i * 4] = y[i] + E / n;
    datum[i * 4 + 1] = (E2 - (E * E) / n) / (n - 1.0);
    datum[i * 4 + 2] = (double)n_lt / n;
    datum[i * 4 + 3] = (double)n_eq / n;
  }
  for (size_t k = 0; k < (size_t)kPpcStats; k++) {
    int64_t above = 0;
    for (size_t c = 0; c < C; c++) above += cc[k * C + c];
    p_value[k] = (double)above / n;
  }
  if (tstat) transpose_trace_vec(sc.host(s_ts), tstat, n_draws, kPpcStats, n_chains);
#endif
  return rc;
}

// ---- LOO-PIT (include/exmc_hip_loo_pit.h; loo_pit_kernel, exmc_loo_pit.hpp) ----------------------------
int exmc_hip_loo_pit(exmc_hip_model* m, exmc_hip_predictive_opts o, const double* draws_dev, int n_draws, int d,
                     int n_chains, size_t scratch_bytes, double* out_dev) {
  const long long n = (long long)n_draws * n_chains;
  int rc = pp_check(m, "loo-pit", o, draws_dev, n_draws, d, n_chains,
                    !out_dev || o.resume || n < 2 || n > 0x7FFFFFFFLL);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)scratch_bytes;
#else
  HIP_TRY(hipSetDevice(m->device));
  LooPitParams P;
  pp_fill(P, m, o, draws_dev, n_draws, d, n_chains);
  const size_t scratch = scratch_bytes ? scratch_bytes : (size_t)EXMC_LOO_PIT_DEFAULT_SCRATCH;
  rc = ic_with_src(m, [&](const auto& src) { return loo_pit_kind(m, src, P, scratch, out_dev); });
#endif
  return rc;
}

int exmc_hip_loo_pit_host(exmc_hip_model* m, exmc_hip_predictive_opts o, const double* draws, int n_draws, int d,
                          int n_chains, size_t scratch_bytes, double* out) {
  const long long n = (long long)n_draws * n_chains;
  int rc = pp_check(m, "loo-pit", o, draws, n_draws, d, n_chains, !out || o.resume || n < 2 || n > 0x7FFFFFFFLL);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  (void)scratch_bytes;
#else
  HIP_TRY(hipSetDevice(m->device));
  const size_t n_out = (size_t)kLooPitRows * (size_t)ic_n_data(m);
  Scratch sc;
  const auto s_out = sc.take<double>(n_out);   // [4][N]
  rc = sc.alloc_with_trace(draws, n_draws, d, n_chains);
  if (!rc) rc = exmc_hip_loo_pit(m, o, sc.trace(), n_draws, d, n_chains, scratch_bytes, sc.dev(s_out));
  if (!rc) rc = sc.download();
  if (rc) return rc;
  std::copy(sc.host(s_out), sc.host(s_out) + n_out, out);
#endif
  return rc;
}

int exmc_hip_loo_pit_from_ll(int device, const double* ll_dev, const double* yrep_dev, const double* y_dev,
                             int n_draws, int n_data, int n_chains, double* out_dev) {
  if (!ll_dev || !yrep_dev || !y_dev || !out_dev || n_draws < 1 || n_data < 1 || n_chains < 1 ||
      (long long)n_draws * n_chains < 2)
    return fail(EXMC_ERR_BADARG, "loo-pit: bad arguments");
  int rc = select_device(device);
  if (rc) return rc;
#ifdef EXMC_ONLY_CUSTOM
  return fail(EXMC_ERR_UNSUPPORTED, "loo-pit: use libexmc_hip.so for the model-free reduction");
#else
  if ((long long)n_draws * n_chains > kPsisMaxSamples)
    return fail(EXMC_ERR_BADARG, "loo-pit: more than 2^31 - 1 pooled samples");
  const int S = n_draws, N = n_data, C = n_chains;
  const hipStream_t stream = (hipStream_t)0;
  LooPitScratch sc;
  rc = sc.alloc(S, C, N);
  if (!rc) rc = psis_tails(stream, sc.at(0), ll_dev, S, N, C);
  if (rc) return rc;
  hipLaunchKernelGGL(loo_pit_ll_kernel, dim3((unsigned)sc.B, (unsigned)((N + kPpBlock - 1) / kPpBlock)), dim3(kPpBlock),
                     0, stream, ll_dev, yrep_dev, y_dev, S, N, C, sc.tables(), sc.state.as<double>());
  HIP_TRY(hipGetLastError());
  rc = loo_pit_finish(stream, sc, N, out_dev);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(stream));
  return EXMC_OK;
#endif
}

}  // extern "C"
