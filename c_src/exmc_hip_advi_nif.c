/* exmc_hip_advi_nif.c -- NIF module `Elixir.Exmc.NUTS.HipAdviNative`: Exmc.ADVI of a built model kind
 * on the device (include/exmc_hip_advi.h; DESIGN.md "ADVI").
 *
 *   fit/12  model = {kind, data_bin} as HipNative.model_create/2 takes them, perm (the list
 *           model_set_flat_order/2 takes; []: the kernel order is the flat order), n_fits, chain_lo,
 *           num_draws, max_iters, num_mc_samples, window_size, learning_rate, convergence_tol, seed,
 *           lanes_per_chain (0: the kind's default)
 *           -> {draws_bin [fit][draw][dim], mu_bin [fit][dim], log_sigma_bin [fit][dim],
 *               elbo_history_bin [fit][max_iters] (f64, kernel order, unconstrained; NaN at and after
 *               num_iters), num_iters_bin, converged_bin [fit] (i32)}
 *           (exmc_hip_advi_host; fit c has seed + 7919 (chain_lo + c))
 *
 * Written the way exmc_hip_pathfinder_nif.c is, and a module beside it: the call makes a handle of its
 * own from the model's kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind or lane count without a compiled layout: code 4), a dirty
 * IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_advi.h"

static int g_device = 0;

static ERL_NIF_TERM fit(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  const ERL_NIF_TERM* model;
  int arity, kind, n_fits, chain_lo, lanes;
  exmc_hip_advi_opts o;
  const double* data;
  size_t nd;
  unsigned plen;
  ErlNifUInt64 seed;
  (void)argc;
  if (!enif_get_tuple(env, argv[0], &arity, &model) || arity != 2 || !enif_get_int(env, model[0], &kind) ||
      !get_f64_bin(env, model[1], &data, &nd) || !enif_get_list_length(env, argv[1], &plen) ||
      !enif_get_int(env, argv[2], &n_fits) || !enif_get_int(env, argv[3], &chain_lo) ||
      !enif_get_int(env, argv[4], &o.num_draws) || !enif_get_int(env, argv[5], &o.max_iters) ||
      !enif_get_int(env, argv[6], &o.num_mc_samples) || !enif_get_int(env, argv[7], &o.window_size) ||
      !get_f64(env, argv[8], &o.learning_rate) || !get_f64(env, argv[9], &o.convergence_tol) ||
      !enif_get_uint64(env, argv[10], &seed) || !enif_get_int(env, argv[11], &lanes) || n_fits < 1 ||
      o.num_draws < 1 || o.max_iters < 1 || chain_lo < 0 || lanes < 0)
    return enif_make_badarg(env);
  o.seed = (uint64_t)seed;
  o.lanes_per_chain = lanes;
  exmc_hip_model* m = NULL;
  int rc = exmc_hip_model_create(kind, 0, data, (int)nd, g_device, &m);
  if (rc != EXMC_OK) return raise_hip(env, rc);
  const int d = exmc_hip_model_dim(m);
  if (plen != 0) {
    int32_t* perm = (int32_t*)enif_alloc(plen * sizeof(int32_t));
    ERL_NIF_TERM head, tail = argv[1];
    int ok = (int)plen == d;
    for (unsigned i = 0; i < plen && ok; i++) {
      int v;
      ok = enif_get_list_cell(env, tail, &head, &tail) && enif_get_int(env, head, &v);
      perm[i] = ok ? v : 0;
    }
    rc = ok ? exmc_hip_model_set_flat_order(m, perm, d) : EXMC_ERR_BADARG;
    enif_free(perm);
    if (rc != EXMC_OK) {
      exmc_hip_model_destroy(m);
      return raise_hip(env, rc);
    }
  }
  const size_t C = (size_t)n_fits, S = (size_t)o.num_draws, D = (size_t)d, I = (size_t)o.max_iters;
  ERL_NIF_TERM t[6];
  double* draws = new_f64_bin(env, C * S * D, &t[0]);
  double* mu = new_f64_bin(env, C * D, &t[1]);
  double* ls = new_f64_bin(env, C * D, &t[2]);
  double* hist = new_f64_bin(env, C * I, &t[3]);
  int32_t* ni = (int32_t*)enif_make_new_binary(env, C * 4, &t[4]);
  int32_t* cv = (int32_t*)enif_make_new_binary(env, C * 4, &t[5]);
  rc = exmc_hip_advi_host(m, o, n_fits, chain_lo, draws, mu, ls, hist, ni, cv);
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? enif_make_tuple_from_array(env, t, 6) : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"fit", 12, fit, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

static int on_load(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)env;
  (void)priv;
  (void)info;
  const char* dev = getenv("EXMC_HIP_DEVICE");
  g_device = dev ? atoi(dev) : 0;
  return 0;
}

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipAdviNative, nif_funcs, on_load, NULL, NULL, NULL)
