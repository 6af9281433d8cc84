/* exmc_hip_loo_pit_nif.c -- NIF module `Elixir.Exmc.NUTS.HipLooPitNative`: PSIS-LOO-PIT of a built model
 * kind on the device (include/exmc_hip_loo_pit.h; DESIGN.md "LOO-PIT").
 *
 *   loo_pit/6   model = {kind, data_bin} as HipNative.model_create/2 takes them, draws_bin
 *               [chain][draw][dim] (kernel order, unconstrained, as HipNative's sampling functions return
 *               it), n_chains, n_draws, seed, chain_lo
 *               -> out_bin [4][datum] (rows p_lt, p_eq, pit, Pareto k; f64; datums in the kind's data order)
 *               (exmc_hip_loo_pit_host with the default scratch; the replicates are
 *               exmc_hip_posterior_predictive's at the same arguments, the weights PSIS-LOO's)
 *
 * Written the way exmc_hip_ppc_nif.c is, and a module beside it: the call makes a handle of its own from
 * the model's kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian f64 binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without datums: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"
#include "../include/exmc_hip_loo_pit.h"

static int g_device = 0;

static ERL_NIF_TERM loo_pit(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  const ERL_NIF_TERM* model;
  int arity, kind, c, s;
  const double *data, *draws;
  size_t nd, n;
  ErlNifUInt64 seed;
  exmc_hip_predictive_opts o;
  (void)argc;
  if (!enif_get_tuple(env, argv[0], &arity, &model) || arity != 2 || !enif_get_int(env, model[0], &kind) ||
      !get_f64_bin(env, model[1], &data, &nd) || !get_f64_bin(env, argv[1], &draws, &n) ||
      !enif_get_int(env, argv[2], &c) || !enif_get_int(env, argv[3], &s) || !enif_get_uint64(env, argv[4], &seed) ||
      !enif_get_int(env, argv[5], &o.chain_lo) || c < 1 || s < 1 || o.chain_lo < 0)
    return enif_make_badarg(env);
  o.seed = (uint64_t)seed;
  o.resume = 0;
  exmc_hip_model* m = NULL;
  int rc = exmc_hip_model_create(kind, 0, data, (int)nd, g_device, &m);
  if (rc != EXMC_OK) return raise_hip(env, rc);
  const int d = exmc_hip_model_dim(m);
  const int N = exmc_hip_model_n_data(m);
  ERL_NIF_TERM out = 0;
  if (n != (size_t)c * (size_t)s * (size_t)d) {
    rc = EXMC_ERR_BADARG;
  } else if (N < 0) {
    double none[EXMC_LOO_PIT_ROWS];   /* EXMC_ERR_UNSUPPORTED and its message */
    rc = exmc_hip_loo_pit_host(m, o, draws, s, d, c, 0, none);
  } else {
    double* rows = new_f64_bin(env, (size_t)EXMC_LOO_PIT_ROWS * (size_t)N, &out);
    rc = exmc_hip_loo_pit_host(m, o, draws, s, d, c, 0, rows);
  }
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? out : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"loo_pit", 6, loo_pit, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

static int on_load(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)env;
  (void)priv;
  (void)info;
  const char* dev = getenv("EXMC_HIP_DEVICE");
  g_device = dev ? atoi(dev) : 0;
  return 0;
}

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipLooPitNative, nif_funcs, on_load, NULL, NULL, NULL)
