// The model-dependent kernel instantiations of a plug-in, once per layout the generated header carries
// (the EXMC_MODEL_CUSTOM rows of exmc_layouts.inc: a plug-in build has no other).
// Included by exmc_plugin_part.hip (EXMC_PLUGIN_PART = which part: explicit instantiation) and by
// exmc_hip.hip under EXMC_PLUGIN_SPLIT (EXMC_PLUGIN_PART undefined: extern declarations of all).
#ifdef EXMC_PLUGIN_PART
#define EXMC_PK_DECL template
#else
#define EXMC_PK_DECL extern template
#endif
#define EXMC_PK_NUTS(M, G, LDSL, STREAM) \
  EXMC_PK_DECL __global__ void nuts_kernel<M, G, LDSL, false, STREAM>(NutsParams, typename M::Consts);
#define EXMC_PK_WARM(M, G, LDSL, PIPE) \
  EXMC_PK_DECL __global__ void warmup_kernel<M, G, LDSL, PIPE>(WarmupParams, typename M::Consts);

// part 5: the auxiliary kernels of a layout (vag_fn batches, chain init, the step-size search, Pathfinder, ADVI,
// the fits' log ratios, the start and the mutation of SMC and of its bridged mode)
#define EXMC_PK_AUX(M, G) \
  EXMC_PK_DECL __global__ void multi_step_kernel<M, G>(MultiStepParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void logp_grad_kernel<M, G>(const double*, int, double*, double*, typename M::Consts); \
  EXMC_PK_DECL __global__ void init_chains_kernel<M, G>(InitParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void find_eps_kernel<M, G>(FindEpsParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void pathfinder_kernel<M, G>(PathfinderParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void advi_kernel<M, G>(AdviParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void fit_log_ratio_kernel<M, G>(FitLogRatioParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void smc_init_kernel<M, G>(SmcParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void smc_mutate_kernel<M, G>(SmcParams, typename M::Consts); \
  EXMC_PK_DECL __global__ void smc_bridge_init_kernel<M, G>(SmcParams, SmcBridge, typename M::Consts); \
  EXMC_PK_DECL __global__ void smc_bridge_mutate_kernel<M, G>(SmcParams, SmcBridge, typename M::Consts);

// and the chain init of a one-chain form (EXMC_ONE_CHAIN rows)
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 5
#define EXMC_LAYOUT(K, L, M, LDSL, ...) EXMC_PK_AUX(M, L)
#define EXMC_ONE_CHAIN(K, L, M, G, LDSL, ...) \
  EXMC_PK_DECL __global__ void init_chains_kernel<M, G>(InitParams, typename M::Consts);
#include "exmc_layouts.inc"
#endif
// part 6: the warmup kernel of a one-chain form (a lane layout of fewer than 64 lanes per chain,
// exmc_models.hpp CustomSplit) -- with the chain init, the kernels of the shared warmup only
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 6
#define EXMC_LAYOUT(...)
#define EXMC_ONE_CHAIN(K, L, M, G, LDSL, ...) EXMC_PK_WARM(M, G, LDSL, false)
#include "exmc_layouts.inc"
#endif
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 1
#define EXMC_LAYOUT(K, L, M, LDSL, ...) EXMC_PK_NUTS(M, L, LDSL, false)
#include "exmc_layouts.inc"
#endif
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 2
#define EXMC_LAYOUT(K, L, M, LDSL, ...) EXMC_PK_NUTS(M, L, LDSL, true)
#include "exmc_layouts.inc"
#endif
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 3
#define EXMC_LAYOUT(K, L, M, LDSL, ...) EXMC_PK_WARM(M, L, LDSL, true)
#include "exmc_layouts.inc"
#endif
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 4
#define EXMC_LAYOUT(K, L, M, LDSL, ...) EXMC_PK_WARM(M, L, LDSL, false)
#include "exmc_layouts.inc"
#endif
// part 7: the independent-adaptation kernel (sample_chains vectorized: false), one per layout
#define EXMC_PK_INDEP(M, G, LDSL) \
  EXMC_PK_DECL __global__ void indep_kernel<M, G, LDSL>(IndepParams, typename M::Consts);
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 7
#define EXMC_LAYOUT(K, L, M, LDSL, ...) EXMC_PK_INDEP(M, L, LDSL)
#include "exmc_layouts.inc"
#endif
// part 8: the workgroup form of the sampling kernel for a lane layout that asks for it (EXMC_GEN_WG, codegen_lanes.py)
#if defined(EXMC_GEN_LANES) && EXMC_GEN_WG && (!defined(EXMC_PLUGIN_LAYOUT) || EXMC_PLUGIN_LAYOUT == 3)
#if !defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 8
EXMC_PK_DECL __global__ void nuts_kernel_wg<Custom<EXMC_GEN_LANES>, EXMC_GEN_LANES, 1, 8>(
    NutsParams, typename Custom<EXMC_GEN_LANES>::Consts);
#endif
#endif
// part 9: the per-datum terms over a trace, when the header carries them (codegen.py generate(pointwise=True));
// the kernel is no template on a layout
#if defined(EXMC_GEN_POINTWISE) && (!defined(EXMC_PLUGIN_PART) || EXMC_PLUGIN_PART == 9)
EXMC_PK_DECL __global__ void gen_pointwise_kernel<EXMC_GEN_PW_N>(GenPwParams);
#endif
#undef EXMC_PK_INDEP
#undef EXMC_PK_NUTS
#undef EXMC_PK_WARM
#undef EXMC_PK_AUX
#undef EXMC_PK_DECL
