/* exmc_hip_psis_nif.c -- NIF module `Elixir.Exmc.NUTS.HipPsisNative`: PSIS-LOO with the Pareto k
 * diagnostic of a built model kind (include/exmc_hip_psis.h; DESIGN.md "PSIS-LOO").
 *
 *   psis_stats/4 model = {kind, data_bin} as HipNative.model_create/2 takes them, draws_bin
 *                [chain][draw][dim] (kernel order, as HipNative's sampling functions return it),
 *                n_chains, n_draws -> out_bin [3][N]: per datum elpd_loo, p_loo, Pareto k
 *                (exmc_hip_psis_stats_host with the default scratch budget)
 *
 * A per-call module on the frame of exmc_nif_util.h: the call makes a handle of its own from the model's
 * kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian f64 binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without per-datum terms: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"

static ERL_NIF_TERM psis_stats(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  nif_model model;
  int c, s, d, N;
  const double* draws;
  size_t n;
  (void)argc;
  if (!get_model(env, argv[0], &model) || !get_f64_bin(env, argv[1], &draws, &n) ||
      !enif_get_int(env, argv[2], &c) || !enif_get_int(env, argv[3], &s) || c < 1 || s < 1)
    return enif_make_badarg(env);
  exmc_hip_model* m = NULL;
  int rc = model_open(&model, g_device, &m, &d, &N);
  if (rc != EXMC_OK) return raise_hip(env, rc);
  ERL_NIF_TERM out = 0;
  if (n != (size_t)c * (size_t)s * (size_t)d) {
    rc = EXMC_ERR_BADARG;
  } else if (N < 0) {
    rc = exmc_hip_psis_stats_host(m, draws, s, d, c, 0, NULL);   /* EXMC_ERR_UNSUPPORTED and its message */
  } else {
    double* st = new_f64_bin(env, (size_t)3 * (size_t)N, &out);
    rc = exmc_hip_psis_stats_host(m, draws, s, d, c, 0, st);
  }
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? out : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"psis_stats", 4, psis_stats, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipPsisNative, nif_funcs, load_device, NULL, NULL, NULL)
