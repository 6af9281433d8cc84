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
 * Written the way exmc_hip_predictive_nif.c is, and a module beside it: the call makes a handle of its own
 * from the model's kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian f64 binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind without datums: code 4), a dirty IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_compare.h"
#include "../include/exmc_hip_ppc.h"

static int g_device = 0;

static ERL_NIF_TERM ppc(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
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

static int on_load(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)env;
  (void)priv;
  (void)info;
  const char* dev = getenv("EXMC_HIP_DEVICE");
  g_device = dev ? atoi(dev) : 0;
  return 0;
}

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipPpcNative, nif_funcs, on_load, NULL, NULL, NULL)
