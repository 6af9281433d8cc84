/* exmc_hip_pathfinder_nif.c -- NIF module `Elixir.Exmc.NUTS.HipPathfinderNative`: Exmc.Pathfinder of a
 * built model kind on the device (include/exmc_hip_pathfinder.h; DESIGN.md "Pathfinder").
 *
 *   fit/9  model = {kind, data_bin} as HipNative.model_create/2 takes them, perm (the list
 *          model_set_flat_order/2 takes; []: the kernel order is the flat order), n_paths, chain_lo,
 *          num_draws, max_iters, history_size, seed, lanes_per_chain (0: the kind's default)
 *          -> {draws_bin [path][draw][dim], mu_bin [path][dim], sigma_bin [path][dim], elbo_bin [path]
 *              (f64, kernel order, unconstrained), num_iters_bin, best_index_bin, status_bin [path] (i32)}
 *          (exmc_hip_pathfinder_host; path c has seed + 7919 (chain_lo + c))
 *
 * A per-call module on the frame of exmc_nif_util.h: the call makes a handle of its own from the model's
 * kind and data and destroys it before it returns. Conventions as exmc_hip_nif.c:
 * native-endian binaries, a decode failure is a badarg, a failed library call raises
 * {:exmc_hip_error, code, message} (a kind or lane count without a compiled layout: code 4), a dirty
 * IO-bound job. */
#include "exmc_nif_util.h"

#include "../include/exmc_hip_pathfinder.h"

static ERL_NIF_TERM fit(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  nif_model model;
  int n_paths, chain_lo, num_draws, max_iters, history, lanes, d;
  unsigned plen;
  ErlNifUInt64 seed;
  (void)argc;
  if (!get_model(env, argv[0], &model) || !enif_get_list_length(env, argv[1], &plen) ||
      !enif_get_int(env, argv[2], &n_paths) || !enif_get_int(env, argv[3], &chain_lo) ||
      !enif_get_int(env, argv[4], &num_draws) || !enif_get_int(env, argv[5], &max_iters) ||
      !enif_get_int(env, argv[6], &history) || !enif_get_uint64(env, argv[7], &seed) ||
      !enif_get_int(env, argv[8], &lanes) || n_paths < 1 || num_draws < 1 || chain_lo < 0 || lanes < 0)
    return enif_make_badarg(env);
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
  const size_t C = (size_t)n_paths, S = (size_t)num_draws, D = (size_t)d;
  ERL_NIF_TERM t[7];
  double* draws = new_f64_bin(env, C * S * D, &t[0]);
  double* mu = new_f64_bin(env, C * D, &t[1]);
  double* sigma = new_f64_bin(env, C * D, &t[2]);
  double* elbo = new_f64_bin(env, C, &t[3]);
  int32_t* ni = (int32_t*)enif_make_new_binary(env, C * 4, &t[4]);
  int32_t* bi = (int32_t*)enif_make_new_binary(env, C * 4, &t[5]);
  int32_t* st = (int32_t*)enif_make_new_binary(env, C * 4, &t[6]);
  exmc_hip_pf_opts o;
  o.num_draws = num_draws;
  o.max_iters = max_iters;
  o.history_size = history;
  o.seed = (uint64_t)seed;
  o.lanes_per_chain = lanes;
  rc = exmc_hip_pathfinder_host(m, o, n_paths, chain_lo, draws, mu, sigma, elbo, ni, bi, st);
  exmc_hip_model_destroy(m);
  return rc == EXMC_OK ? enif_make_tuple_from_array(env, t, 7) : raise_hip(env, rc);
}

static ErlNifFunc nif_funcs[] = {
    {"fit", 9, fit, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.Exmc.NUTS.HipPathfinderNative, nif_funcs, load_device, NULL, NULL, NULL)
