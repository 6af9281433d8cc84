/* exmc_hip_ppc_nif.c -- NIF module `Elixir.Exmc.NUTS.HipPpcNative`: posterior predictive checks of a built
 * model kind on the device (include/exmc_hip_ppc.h; DESIGN.md "Posterior predictive checks").
 *
 *   ppc/6   model = {kind, data_bin} as HipNative.model_create/2 takes them, draws_bin [chain][draw][dim]
 *           (kernel order, unconstrained, as HipNative's sampling functions return it), n_chains, n_draws,
 *           seed, chain_lo
 *           -> {datum_bin [datum][4] (mean, var, p_lt, p_eq; datums in the kind's data order),
 *               t_obs_bin [4], p_value_bin [4]} (f64; the statistics mean, var, min, max)
 *           (exmc_hip_ppc_host; the replicates are exmc_hip_posterior_predictive's at the same arguments)
 *
 * A per-call module on the frame of exmc_nif_util.h: the call makes a handle of its own from the model's
 * kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian f64 binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without datums: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"
#include "../include/exmc_hip_ppc.h"

static ERL_NIF_TERM ppc(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  nif_model model;
  int c, s, d, N;
  const double* draws;
  size_t n;
  ErlNifUInt64 seed;
  exmc_hip_predictive_opts o;
  (void)argc;
  if (!get_model(env, argv[0], &model) || !get_f64_bin(env, argv[1], &draws, &n) ||
      !enif_get_int(env, argv[2], &c) || !enif_get_int(env, argv[3], &s) || !enif_get_uint64(env, argv[4], &seed) ||
      !enif_get_int(env, argv[5], &o.chain_lo) || c < 1 || s < 1 || o.chain_lo < 0)
    return enif_make_badarg(env);
  o.seed = (uint64_t)seed;
  o.resume = 0;
  exmc_hip_model* m = NULL;
  int rc = model_open(&model, g_device, &m, &d, &N);
  if (rc != EXMC_OK) return raise_hip(env, rc);
  ERL_NIF_TERM out[3] = {0, 0, 0};
  if (n != (size_t)c * (size_t)s * (size_t)d) {
    rc = EXMC_ERR_BADARG;
  } else if (N < 0) {
    double none[EXMC_PPC_NSTAT];   /* EXMC_ERR_UNSUPPORTED and its message */
    rc = exmc_hip_ppc_host(m, o, draws, s, d, c, none, none, none, NULL);
  } else {
    double* datum = new_f64_bin(env, (size_t)N * 4, &out[0]);
    double* t_obs = new_f64_bin(env, EXMC_PPC_NSTAT, &out[1]);
    double* p_value = new_f64_bin(env, EXMC_PPC_NSTAT, &out[2]);
    rc = exmc_hip_ppc_host(m, o, draws, s, d, c, datum, t_obs, p_value, NULL);
  }
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? enif_make_tuple_from_array(env, out, 3) : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"ppc", 6, ppc, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipPpcNative, nif_funcs, load_device, NULL, NULL, NULL)
