/* exmc_hip_compare_nif.c -- NIF module `Elixir.Exmc.NUTS.HipCompareNative`: model comparison of a
 * built model kind (include/exmc_hip_compare.h; Exmc.ModelComparison, lib/exmc/model_comparison.ex).
 *
 *   ic_stats/4   model = {kind, data_bin} as HipNative.model_create/2 takes them, draws_bin
 *                [chain][draw][dim] (kernel order, as HipNative's sampling functions return it),
 *                n_chains, n_draws -> stats_bin [4][N]: per datum lppd, p_waic, elpd_loo, p_loo
 *
 * A module of its own, as each later feature's is: HipNative's function table is fixed. A per-call
 * module on the frame of exmc_nif_util.h: the call makes a handle of its own from the model's kind and
 * data and destroys it before it returns. Conventions as exmc_hip_nif.c: native-endian f64
 * binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without per-datum terms: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"

static ERL_NIF_TERM ic_stats(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
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
    rc = exmc_hip_ic_stats_host(m, draws, s, d, c, NULL);   /* EXMC_ERR_UNSUPPORTED and its message */
  } else {
    double* st = new_f64_bin(env, (size_t)4 * (size_t)N, &out);
    rc = exmc_hip_ic_stats_host(m, draws, s, d, c, st);
  }
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? out : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"ic_stats", 4, ic_stats, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipCompareNative, nif_funcs, load_device, NULL, NULL, NULL)
