/* exmc_hip_predictive_nif.c -- NIF module `Elixir.Exmc.NUTS.HipPredictiveNative`: posterior predictive
 * replicates of a built model kind on the device (include/exmc_hip_predictive.h; DESIGN.md "Posterior
 * predictive"; Exmc.Predictive.posterior_predictive, lib/exmc/predictive.ex).
 *
 *   posterior_predictive/6  model = {kind, data_bin} as HipNative.model_create/2 takes them, draws_bin
 *           [chain][draw][dim] (kernel order, unconstrained, as HipNative's sampling functions return
 *           it), n_chains, n_draws, seed, chain_lo
 *           -> yrep_bin [chain][draw][datum] (f64; datums in the kind's data order)
 *           (exmc_hip_posterior_predictive_host; chain c draws with seed + 7919 (chain_lo + c))
 *
 * A per-call module on the frame of exmc_nif_util.h: the call makes a handle of its own from the model's
 * kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian f64 binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without datums: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"
#include "../include/exmc_hip_predictive.h"

static ERL_NIF_TERM posterior_predictive(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
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
  ERL_NIF_TERM out = 0;
  if (n != (size_t)c * (size_t)s * (size_t)d) {
    rc = EXMC_ERR_BADARG;
  } else if (N < 0) {
    double none = 0.0;   /* EXMC_ERR_UNSUPPORTED and its message */
    rc = exmc_hip_posterior_predictive_host(m, o, draws, s, d, c, NULL, &none);
  } else {
    double* yrep = new_f64_bin(env, (size_t)c * (size_t)s * (size_t)N, &out);
    rc = exmc_hip_posterior_predictive_host(m, o, draws, s, d, c, NULL, yrep);
  }
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? out : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"posterior_predictive", 6, posterior_predictive, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipPredictiveNative, nif_funcs, load_device, NULL, NULL, NULL)
