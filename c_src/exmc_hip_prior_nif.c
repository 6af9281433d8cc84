/* exmc_hip_prior_nif.c -- NIF module `Elixir.Exmc.NUTS.HipPriorNative`: prior and prior predictive samples
 * of a built model kind on the device (include/exmc_hip_prior.h; DESIGN.md "Prior predictive";
 * Exmc.Predictive.prior_samples, lib/exmc/predictive.ex).
 *
 *   prior_samples/6  model = {kind, data_bin} as HipNative.model_create/2 takes them, n_chains, n_draws,
 *           seed, chain_lo, replicates (0 | 1)
 *           -> {x_bin, q_bin, yrep_bin}: x [chain][draw][dim] the constrained values, q [chain][draw][dim]
 *           the unconstrained position (both f64, kernel order; q is a trace HipPredictive takes), yrep
 *           [chain][draw][datum] the datums' replicates in the kind's data order, an empty binary with
 *           replicates = 0 (then no datum is drawn and the generators do not advance for them)
 *           (exmc_hip_prior_samples_host; chain c draws with seed + 7919 (chain_lo + c))
 *
 * A per-call module on the frame of exmc_nif_util.h: the call makes a handle of its own from the model's
 * kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian f64 binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without a prior walk: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"
#include "../include/exmc_hip_prior.h"

static ERL_NIF_TERM prior_samples(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  nif_model model;
  int c, s, rep, d, N;
  ErlNifUInt64 seed;
  exmc_hip_predictive_opts o;
  (void)argc;
  if (!get_model(env, argv[0], &model) || !enif_get_int(env, argv[1], &c) || !enif_get_int(env, argv[2], &s) ||
      !enif_get_uint64(env, argv[3], &seed) || !enif_get_int(env, argv[4], &o.chain_lo) ||
      !enif_get_int(env, argv[5], &rep) || c < 1 || s < 1 || o.chain_lo < 0 || (rep != 0 && rep != 1))
    return enif_make_badarg(env);
  o.seed = (uint64_t)seed;
  o.resume = 0;
  exmc_hip_model* m = NULL;
  int rc = model_open(&model, g_device, &m, &d, &N);
  if (rc != EXMC_OK) return raise_hip(env, rc);
  ERL_NIF_TERM out[3] = {0, 0, 0};
  if (N < 0) {
    double none = 0.0;   /* EXMC_ERR_UNSUPPORTED and its message */
    rc = exmc_hip_prior_samples_host(m, o, s, c, NULL, &none, &none, NULL);
  } else {
    const size_t rows = (size_t)c * (size_t)s;
    double* x = new_f64_bin(env, rows * (size_t)d, &out[0]);
    double* q = new_f64_bin(env, rows * (size_t)d, &out[1]);
    double* yrep = new_f64_bin(env, rep ? rows * (size_t)N : 0, &out[2]);
    rc = exmc_hip_prior_samples_host(m, o, s, c, NULL, x, q, rep ? yrep : NULL);
  }
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? enif_make_tuple_from_array(env, out, 3) : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"prior_samples", 6, prior_samples, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipPriorNative, nif_funcs, load_device, NULL, NULL, NULL)
