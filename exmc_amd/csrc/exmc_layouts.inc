// exmc_layouts.inc — every compiled lane layout of every model kind, one row each. Read by
// exmc_hip.hip (dispatch, the dense variants, the default lanes, the stream / independent kernels)
// and by exmc_plugin_kernels.inc (a plug-in's kernel instantiations). The includer defines
// EXMC_LAYOUT and, if it reads them, EXMC_ONE_CHAIN; the table undefines both.
//
// EXMC_LAYOUT(kind, lanes, model, LDSL, member, roles, dense LDSL, dense model)
//   lanes: lanes_per_chain, the model's G; LDSL: tree-stack levels nuts_kernel keeps in LDS
//   member: the constants on the handle (exmc_hip_model::es, sp, sv, lg, rd, cu)
//   roles: kRoleSample / kRoleWarmup / kRoleDense: the kind's default lanes for sampling, for the
//     one-chain warmup, for a dense mass (the first row of the kind with the role; none: 1);
//     kRoleStream: the layout carries the push-style stream and the independent-adaptation kernels
//   dense model: the model under a dense mass in this layout (void: none; one lane takes any model)
// EXMC_ONE_CHAIN(kind, lanes, model, G, LDSL, member, roles): the form the launches of the shared
//   one-chain warmup (chain init, warmup kernel) take at `lanes` for the sampling layout of G lanes
#ifndef EXMC_ONE_CHAIN
#define EXMC_ONE_CHAIN(...)
#endif

#ifdef EXMC_CUSTOM_HEADER
// a generated model (exmc_amd/codegen.py). EXMC_PLUGIN_LAYOUT (1 one lane, 2 plates over 16 lanes,
// 3 several dimensions per lane) narrows a plug-in part to one of them, so that a model with two
// layouts builds its kernels side by side
#if defined(EXMC_GEN_LANES) && (!defined(EXMC_PLUGIN_LAYOUT) || EXMC_PLUGIN_LAYOUT == 3)
#if EXMC_GEN_LANES < 64   // the chain's model terms over the whole wavefront (exmc_models.hpp CustomSplit)
EXMC_ONE_CHAIN(EXMC_MODEL_CUSTOM, 64, CustomSplit, EXMC_GEN_LANES, EXMC_GEN_LDSL, cu, kRoleWarmup)
#endif
EXMC_LAYOUT(EXMC_MODEL_CUSTOM, EXMC_GEN_LANES, Custom<EXMC_GEN_LANES>, EXMC_GEN_LDSL, cu,
            kRoleSample | kRoleWarmup | kRoleStream, 0, void)
#endif
#if defined(EXMC_GEN_VEC) && (!defined(EXMC_PLUGIN_LAYOUT) || EXMC_PLUGIN_LAYOUT == 2)
EXMC_LAYOUT(EXMC_MODEL_CUSTOM, 16, Custom<16>, 6, cu, kRoleSample | kRoleWarmup | kRoleStream, 0, void)
#endif
#if defined(EXMC_GEN_ONE_LANE) && (!defined(EXMC_PLUGIN_LAYOUT) || EXMC_PLUGIN_LAYOUT == 1)
EXMC_LAYOUT(EXMC_MODEL_CUSTOM, 1, Custom<1>, EXMC_GEN_LDS_LEVELS, cu,
            kRoleSample | kRoleWarmup | kRoleDense | kRoleStream, 0, void)
#endif
#endif

#ifndef EXMC_ONLY_CUSTOM   // plug-in builds carry the generated model only
// development builds for kernel work carry one model in one layout: -DEXMC_DEV_ES16_ONLY,
// -DEXMC_DEV_ONLY=EXMC_DEV_SV64 (or _RADON64, _LOGISTIC16)
#define EXMC_DEV_SV64 1
#define EXMC_DEV_RADON64 2
#define EXMC_DEV_LOGISTIC16 3
#if defined(EXMC_DEV_ES16_ONLY)
#define EXMC_ROWS(dev) ((dev) == 4)
#elif defined(EXMC_DEV_ONLY)
#define EXMC_ROWS(dev) ((dev) == EXMC_DEV_ONLY)
#else
#define EXMC_ROWS(dev) 1
#endif
#if EXMC_ROWS(4)
EXMC_LAYOUT(EXMC_MODEL_EIGHT_SCHOOLS, 16, EightSchools<16>, 6, es, kRoleSample | kRoleWarmup | kRoleStream,
            6, RowDenseModel<EightSchools<16>>)
#endif
#if EXMC_ROWS(0)
EXMC_LAYOUT(EXMC_MODEL_EIGHT_SCHOOLS, 1, EightSchools<1>, 2, es, kRoleDense, 0, void)
EXMC_LAYOUT(EXMC_MODEL_EIGHT_SCHOOLS, 2, EightSchools<2>, 3, es, 0, 0, void)
EXMC_LAYOUT(EXMC_MODEL_EIGHT_SCHOOLS, 4, EightSchools<4>, 4, es, 0, 0, void)
EXMC_LAYOUT(EXMC_MODEL_EIGHT_SCHOOLS, 8, EightSchools<8>, 5, es, 0, 0, void)
EXMC_LAYOUT(EXMC_MODEL_SIMPLE, 1, Simple<1>, 6, sp, kRoleSample | kRoleWarmup | kRoleDense | kRoleStream, 0, void)
EXMC_LAYOUT(EXMC_MODEL_SV, 32, SV<32>, 2, sv, 0, 0, void)
EXMC_LAYOUT(EXMC_MODEL_SV_NCP, 64, SVNcp<64>, 3, sv, kRoleSample | kRoleWarmup | kRoleDense | kRoleStream,
            2, LaneDenseModel<SVNcp<64>, 64>)
EXMC_LAYOUT(EXMC_MODEL_LOGISTIC, 4, Logistic<4>, 2, lg, 0, 0, void)   // matrix-core path
EXMC_LAYOUT(EXMC_MODEL_LOGISTIC, 8, Logistic<8>, 2, lg, 0, 0, void)
EXMC_LAYOUT(EXMC_MODEL_RADON, 32, Radon<32>, 2, rd, 0, 0, void)
#endif
#if EXMC_ROWS(EXMC_DEV_SV64)
EXMC_LAYOUT(EXMC_MODEL_SV, 64, SV<64>, 3, sv, kRoleSample | kRoleWarmup | kRoleDense | kRoleStream,
            2, LaneDenseModel<SV<64>, 64>)
#endif
#if EXMC_ROWS(EXMC_DEV_RADON64)
EXMC_LAYOUT(EXMC_MODEL_RADON, 64, Radon<64>, 3, rd, kRoleSample | kRoleWarmup | kRoleDense | kRoleStream,
            2, LaneDenseModel<Radon<64>, 64>)
#endif
#if EXMC_ROWS(EXMC_DEV_LOGISTIC16)
EXMC_LAYOUT(EXMC_MODEL_LOGISTIC, 16, Logistic<16>, 2, lg, kRoleSample | kRoleDense | kRoleStream,
            2, LaneDenseModel<Logistic<16>, 16>)
// logistic's shared warmup is ONE chain, so its 500 observations are best spread over a whole
// wavefront (8 per lane instead of 32: 158 -> 62 ms); sampling keeps 16 lanes per chain
EXMC_LAYOUT(EXMC_MODEL_LOGISTIC, 64, Logistic<64>, 2, lg, kRoleWarmup, 0, void)
#endif
#undef EXMC_ROWS
#undef EXMC_DEV_SV64
#undef EXMC_DEV_RADON64
#undef EXMC_DEV_LOGISTIC16
#endif

#undef EXMC_LAYOUT
#undef EXMC_ONE_CHAIN
