/* exmc_nif_util.h -- what the ten NIF shims of c_src/ share, stated once.
 *
 *   terms      get_* / make_* / tupleN: argument decoding with Rustler's conventions (a decode failure is a
 *              badarg; native/exmc_tree/src/lib.rs:19-32) and result building. Every shim.
 *   raising    raise_msg: {:exmc_hip_error, code, message}; raise_hip takes the message of the library the
 *              shim is linked against, exmc_hip_nif.c's raise_api that of the handle's library. Every shim.
 *   device     env_device: EXMC_HIP_DEVICE, default 0; g_device holds it from load on. load_device is the
 *              whole on_load of a module that needs nothing else (the eight per-call modules name it in
 *              ERL_NIF_INIT); exmc_hip_nif.c and exmc_native_tree_nif.c open a resource type as well and
 *              keep an on_load of their own.
 *   the frame of a per-call module (exmc_hip_{compare,psis,pathfinder,advi,predictive,ppc,loo_pit,prior}_nif.c):
 *              a NIF library cannot read another library's resources, so such a module takes
 *              model = {kind, data_bin} as HipNative.model_create/2 takes them, makes a handle of its own
 *              (one small upload) and destroys it before it returns:
 *                1. get_model and the module's own arguments: any failure is a badarg, and no library call
 *                   has been made yet;
 *                2. model_open(&model, g_device, &m, &d, &N), a failure raised with raise_hip;
 *                3. the module's one library call;
 *                4. exmc_hip_model_destroy(m) on every way out, then the result or raise_hip.
 *   get_i32_list  the flat order as a list (HipNative.model_set_flat_order/2, and the perm argument of
 *              the Pathfinder and ADVI modules).
 *
 * What is NOT here, on purpose: each module's `static ErlNifFunc nif_funcs[]` table and its ERL_NIF_INIT
 * line stand literally in its file (INTEGRATION.md and tests/test_beam_boundary_sources.py read them). */
#ifndef EXMC_NIF_UTIL_H
#define EXMC_NIF_UTIL_H

#ifdef EXMC_USE_SYSTEM_ERL_NIF
#include <erl_nif.h>
#else
#include "erl_nif_decl.h"
#endif

#include <stdlib.h>
#include <string.h>

#include "../include/exmc_hip_compare.h"   /* exmc_hip.h, and exmc_hip_model_n_data */

/* f64: floats, and integers as Elixir callers sometimes pass `0` for `0.0` */
static __attribute__((unused)) int get_f64(ErlNifEnv* env, ERL_NIF_TERM t, double* out) {
  ErlNifSInt64 i;
  if (enif_get_double(env, t, out)) return 1;
  if (enif_get_int64(env, t, &i)) { *out = (double)i; return 1; }
  return 0;
}
static __attribute__((unused)) int get_usize(ErlNifEnv* env, ERL_NIF_TERM t, int* out) {
  ErlNifUInt64 u;
  if (!enif_get_uint64(env, t, &u) || u > 0x7fffffffULL) return 0;
  *out = (int)u;
  return 1;
}
static __attribute__((unused)) int get_bool(ErlNifEnv* env, ERL_NIF_TERM t, int32_t* out) {
  char buf[8];
  if (!enif_get_atom(env, t, buf, sizeof buf, ERL_NIF_LATIN1)) return 0;
  if (strcmp(buf, "true") == 0) { *out = 1; return 1; }
  if (strcmp(buf, "false") == 0) { *out = 0; return 1; }
  return 0;
}
/* a native-endian f64 binary (Nx.to_binary of an f64 tensor) */
static __attribute__((unused)) int get_f64_bin(ErlNifEnv* env, ERL_NIF_TERM t, const double** p, size_t* n) {
  ErlNifBinary b;
  if (!enif_inspect_binary(env, t, &b) || (b.size & 7) != 0) return 0;
  *p = (const double*)b.data;
  *n = b.size / 8;
  return 1;
}
/* a list of numbers -> enif_alloc'd doubles (the legacy list API, lib.rs:345-434) */
static __attribute__((unused)) int get_f64_list(ErlNifEnv* env, ERL_NIF_TERM t, double** p, size_t* n) {
  unsigned len;
  ERL_NIF_TERM head, tail = t;
  if (!enif_get_list_length(env, t, &len)) return 0;
  double* v = (double*)enif_alloc((len ? len : 1) * sizeof(double));
  if (!v) return 0;
  for (unsigned i = 0; i < len; i++) {
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_f64(env, head, &v[i])) {
      enif_free(v);
      return 0;
    }
  }
  *p = v;
  *n = len;
  return 1;
}
/* a list of exactly `want` integers -> enif_alloc'd int32_t (the caller frees it); 0 and nothing to
 * free on another length, an improper list or an element that is no int */
static __attribute__((unused)) int get_i32_list(ErlNifEnv* env, ERL_NIF_TERM t, unsigned want, int32_t** p) {
  unsigned len;
  ERL_NIF_TERM head, tail = t;
  if (!enif_get_list_length(env, t, &len) || len != want) return 0;
  int32_t* v = (int32_t*)enif_alloc((len ? len : 1) * sizeof(int32_t));
  if (!v) return 0;
  for (unsigned i = 0; i < len; i++) {
    int x;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_int(env, head, &x)) {
      enif_free(v);
      return 0;
    }
    v[i] = x;
  }
  *p = v;
  return 1;
}
static __attribute__((unused)) ERL_NIF_TERM make_f64_bin(ErlNifEnv* env, const double* src, size_t n) {
  ERL_NIF_TERM t;
  unsigned char* dst = enif_make_new_binary(env, n * 8, &t);
  if (n) memcpy(dst, src, n * 8);
  return t;
}
static __attribute__((unused)) double* new_f64_bin(ErlNifEnv* env, size_t n, ERL_NIF_TERM* t) {
  return (double*)enif_make_new_binary(env, n * 8, t);
}
static __attribute__((unused)) ERL_NIF_TERM make_f64_list(ErlNifEnv* env, const double* src, size_t n) {
  ERL_NIF_TERM* terms = (ERL_NIF_TERM*)enif_alloc((n ? n : 1) * sizeof(ERL_NIF_TERM));
  for (size_t i = 0; i < n; i++) terms[i] = enif_make_double(env, src[i]);
  ERL_NIF_TERM l = enif_make_list_from_array(env, terms, (unsigned)n);
  enif_free(terms);
  return l;
}
static __attribute__((unused)) ERL_NIF_TERM make_bool(ErlNifEnv* env, int v) { return enif_make_atom(env, v ? "true" : "false"); }
static __attribute__((unused)) ERL_NIF_TERM map_put(ErlNifEnv* env, ERL_NIF_TERM map, const char* key, ERL_NIF_TERM val) {
  ERL_NIF_TERM out = map;
  enif_make_map_put(env, map, enif_make_atom(env, key), val, &out);
  return out;
}
static __attribute__((unused)) ERL_NIF_TERM tuple2(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b) {
  ERL_NIF_TERM v[2] = {a, b};
  return enif_make_tuple_from_array(env, v, 2);
}
static __attribute__((unused)) ERL_NIF_TERM tuple3(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b, ERL_NIF_TERM c) {
  ERL_NIF_TERM v[3] = {a, b, c};
  return enif_make_tuple_from_array(env, v, 3);
}
static __attribute__((unused)) ERL_NIF_TERM tuple4(ErlNifEnv* env, ERL_NIF_TERM a, ERL_NIF_TERM b, ERL_NIF_TERM c,
                                                   ERL_NIF_TERM d) {
  ERL_NIF_TERM v[4] = {a, b, c, d};
  return enif_make_tuple_from_array(env, v, 4);
}
/* a failed library call: raise {:exmc_hip_error, code, message} (Rustler turns a NifResult::Err
 * into a raised term the same way); the library's EXMC_ERR_BADARG is a badarg */
static __attribute__((unused)) ERL_NIF_TERM raise_msg(ErlNifEnv* env, int rc, const char* msg) {
  if (rc == EXMC_ERR_BADARG) return enif_make_badarg(env);
  return enif_raise_exception(env, tuple3(env, enif_make_atom(env, "exmc_hip_error"), enif_make_int(env, rc),
                                          enif_make_string(env, msg, ERL_NIF_LATIN1)));
}
static __attribute__((unused)) ERL_NIF_TERM raise_hip(ErlNifEnv* env, int rc) {
  return raise_msg(env, rc, exmc_hip_last_error());
}

/* the GPU every handle of this module is made on: EXMC_HIP_DEVICE when the module is loaded, default 0 */
static __attribute__((unused)) int env_device(void) {
  const char* dev = getenv("EXMC_HIP_DEVICE");
  return dev ? atoi(dev) : 0;
}
static __attribute__((unused)) int g_device = 0;
static __attribute__((unused)) int load_device(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)env;
  (void)priv;
  (void)info;
  g_device = env_device();
  return 0;
}

/* model = {kind, data_bin}: 0 for a list, a tuple of another arity, a kind that is no int, a binary that
 * is no whole number of f64. data points into the term. */
typedef struct { int kind; const double* data; size_t nd; } nif_model;
static __attribute__((unused)) int get_model(ErlNifEnv* env, ERL_NIF_TERM t, nif_model* out) {
  const ERL_NIF_TERM* item;
  int arity;
  return enif_get_tuple(env, t, &arity, &item) && arity == 2 && enif_get_int(env, item[0], &out->kind) &&
         get_f64_bin(env, item[1], &out->data, &out->nd);
}
/* the per-call handle of a decoded model on `device`, with its dimension and (N != NULL) its number of
 * datums, negative for a kind without datums; returns the library's code. After EXMC_OK the caller owes
 * one exmc_hip_model_destroy(*m). */
static __attribute__((unused)) int model_open(const nif_model* model, int device, exmc_hip_model** m, int* d, int* N) {
  const int rc = exmc_hip_model_create(model->kind, 0, model->data, (int)model->nd, device, m);
  if (rc != EXMC_OK) return rc;
  *d = exmc_hip_model_dim(*m);
  if (N) *N = exmc_hip_model_n_data(*m);
  return EXMC_OK;
}

#endif
