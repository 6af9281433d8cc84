/* exmc_hip_psis_nif.c -- NIF module `Elixir.Exmc.NUTS.HipPsisNative`: PSIS-LOO with the Pareto k
 * diagnostic of a built model kind (include/exmc_hip_psis.h; DESIGN.md "PSIS-LOO").
 *
 *   psis_stats/4 model = {kind, data_bin} as HipNative.model_create/2 takes them, draws_bin
 *                [chain][draw][dim] (kernel order, as HipNative's sampling functions return it),
 *                n_chains, n_draws -> out_bin [3][N]: per datum elpd_loo, p_loo, Pareto k
 *                (exmc_hip_psis_stats_host with the default scratch budget)
 *
 * Written the way exmc_hip_compare_nif.c's ic_stats/4 is, and a module beside it: the function
 * table of HipCompareNative is fixed, as HipNative's is. The call makes a handle of its own from
 * the model's kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian f64 binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without per-datum terms: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"

static int g_device = 0;

static ERL_NIF_TERM raise_rc(ErlNifEnv* env, int rc) {
  if (rc == EXMC_ERR_BADARG) return enif_make_badarg(env);
  return enif_raise_exception(env, tuple3(env, enif_make_atom(env, "exmc_hip_error"), enif_make_int(env, rc),
                                          enif_make_string(env, exmc_hip_last_error(), ERL_NIF_LATIN1)));
}

static ERL_NIF_TERM psis_stats(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  const ERL_NIF_TERM* model;
  int arity, kind, c, s;
  const double *data, *draws;
  size_t nd, n;
  (void)argc;
  if (!enif_get_tuple(env, argv[0], &arity, &model) || arity != 2 || !enif_get_int(env, model[0], &kind) ||
      !get_f64_bin(env, model[1], &data, &nd) || !get_f64_bin(env, argv[1], &draws, &n) ||
      !enif_get_int(env, argv[2], &c) || !enif_get_int(env, argv[3], &s) || c < 1 || s < 1)
    return enif_make_badarg(env);
  exmc_hip_model* m = NULL;
  int rc = exmc_hip_model_create(kind, 0, data, (int)nd, g_device, &m);
  if (rc != EXMC_OK) return raise_rc(env, rc);
  const int d = exmc_hip_model_dim(m);
  const int N = exmc_hip_model_n_data(m);
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
  return rc == EXMC_OK ? out : raise_rc(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"psis_stats", 4, psis_stats, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

static int on_load(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)env;
  (void)priv;
  (void)info;
  const char* dev = getenv("EXMC_HIP_DEVICE");
  g_device = dev ? atoi(dev) : 0;
  return 0;
}

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipPsisNative, nif_funcs, on_load, NULL, NULL, NULL)
