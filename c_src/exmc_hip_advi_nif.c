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
 * A per-call module on the frame of exmc_nif_util.h: the call makes a handle of its own from the model's
 * kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind or lane count without a compiled layout: code 4), a dirty
 * IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_advi.h"

static ERL_NIF_TERM fit(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  nif_model model;
  int n_fits, chain_lo, lanes, d;
  exmc_hip_advi_opts o;
  unsigned plen;
  ErlNifUInt64 seed;
  (void)argc;
  if (!get_model(env, argv[0], &model) || !enif_get_list_length(env, argv[1], &plen) ||
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
  int rc = model_open(&model, g_device, &m, &d, NULL);
  if (rc != EXMC_OK) return raise_hip(env, rc);
  if (plen != 0) {   /* []: the kernel order is the flat order, no call */
    int32_t* perm;
    rc = EXMC_ERR_BADARG;
    if (get_i32_list(env, argv[1], (unsigned)d, &perm)) {
      rc = exmc_hip_model_set_flat_order(m, perm, d);
      enif_free(perm);
    }
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

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipAdviNative, nif_funcs, load_device, NULL, NULL, NULL)
