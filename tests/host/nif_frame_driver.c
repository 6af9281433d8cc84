/* nif_frame_driver.c -- TEST INFRASTRUCTURE ONLY: drives the frame the per-call NIF modules share
 * (c_src/exmc_nif_util.h) as a program of its own, compiled with tests/host/fake_erl_nif.c and
 * tests/host/stub_exmc_hip.c under -fsanitize=address,undefined (tests/test_nif_frame.py), no GPU:
 *   A  get_model: {kind, data_bin}, and every refused form
 *   B  model_open / exmc_hip_model_destroy against the stub library, and a kind it refuses
 *   C  get_i32_list: the right length, a wrong one, an element that is no int, [], no list
 *   D  raise_msg / raise_hip: a badarg for EXMC_ERR_BADARG, else {:exmc_hip_error, code, message}
 *   E  env_device / load_device
 * Exit code 0, the line "nif_frame_driver: ok" and no sanitizer report = pass. */
#include <stdio.h>

#include "../../c_src/exmc_nif_util.h"

/* the harness API of fake_erl_nif.c */
void fk_reset(void);
ERL_NIF_TERM fk_atom(const char* name);
ERL_NIF_TERM fk_double(double x);
ERL_NIF_TERM fk_int(long long v);
ERL_NIF_TERM fk_binary(const void* p, size_t n);
ERL_NIF_TERM fk_list(const ERL_NIF_TERM* items, unsigned n);
long long fk_get_int(ERL_NIF_TERM t);
const char* fk_get_str(ERL_NIF_TERM t);
unsigned fk_len(ERL_NIF_TERM t);
ERL_NIF_TERM fk_item(ERL_NIF_TERM t, unsigned i);
ERL_NIF_TERM fk_exception(void);
int fk_badarg(void);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static ErlNifEnv* const ENV = NULL;   /* the fake runtime has one environment and ignores the argument */

static ERL_NIF_TERM tuple_of(const ERL_NIF_TERM* items, unsigned n) { return enif_make_tuple_from_array(ENV, items, n); }
static ERL_NIF_TERM int_list(const long long* v, unsigned n) {
  ERL_NIF_TERM items[8];
  for (unsigned i = 0; i < n; i++) items[i] = fk_int(v[i]);
  return fk_list(items, n);
}

static void model_tuple(void) {
  const double data[4] = {1.5, -2.0, 3.25, 4.0};
  nif_model mt;
  ERL_NIF_TERM good[3] = {fk_int(2), fk_binary(data, sizeof data), fk_int(1)};
  CHECK(get_model(ENV, tuple_of(good, 2), &mt));
  CHECK(mt.kind == 2 && mt.nd == 4 && memcmp(mt.data, data, sizeof data) == 0);
  ERL_NIF_TERM empty[2] = {fk_int(0), fk_binary(data, 0)};
  CHECK(get_model(ENV, tuple_of(empty, 2), &mt) && mt.kind == 0 && mt.nd == 0);
  CHECK(!get_model(ENV, fk_list(good, 2), &mt));              /* a list */
  CHECK(!get_model(ENV, tuple_of(good, 3), &mt));             /* another arity */
  CHECK(!get_model(ENV, tuple_of(good, 1), &mt));
  CHECK(!get_model(ENV, fk_atom("model"), &mt));
  ERL_NIF_TERM atom_kind[2] = {fk_atom("eight_schools"), good[1]};
  CHECK(!get_model(ENV, tuple_of(atom_kind, 2), &mt));        /* a kind that is no int */
  ERL_NIF_TERM float_kind[2] = {fk_double(2.0), good[1]};
  CHECK(!get_model(ENV, tuple_of(float_kind, 2), &mt));
  ERL_NIF_TERM short_bin[2] = {good[0], fk_binary(data, 12)};
  CHECK(!get_model(ENV, tuple_of(short_bin, 2), &mt));        /* no whole number of f64 */
  ERL_NIF_TERM no_bin[2] = {good[0], fk_int(7)};
  CHECK(!get_model(ENV, tuple_of(no_bin, 2), &mt));
  fk_reset();
}

static void handle(void) {
  const double data[3] = {0.0, 1.0, 2.0};
  nif_model mt = {2, data, 3};
  exmc_hip_model* m = NULL;
  int d = -7, N = -7;
  CHECK(model_open(&mt, 0, &m, &d, &N) == EXMC_OK && m != NULL);
  CHECK(d == exmc_hip_model_dim(m) && d == 3 && N == exmc_hip_model_n_data(m));
  exmc_hip_model_destroy(m);
  m = NULL;
  d = -7;
  CHECK(model_open(&mt, 1, &m, &d, NULL) == EXMC_OK && m != NULL && d == 3);   /* a caller without datums */
  exmc_hip_model_destroy(m);
  m = NULL;
  d = N = -7;
  mt.kind = -1;                                                /* the stub refuses it: nothing to destroy */
  CHECK(model_open(&mt, 0, &m, &d, &N) == EXMC_ERR_BADARG && m == NULL && d == -7 && N == -7);
}

static void i32_list(void) {
  const long long v[4] = {3, 0, -2147483647LL - 1, 2147483647LL};
  int32_t* p = NULL;
  CHECK(get_i32_list(ENV, int_list(v, 4), 4, &p) && p != NULL);
  CHECK(p[0] == 3 && p[1] == 0 && p[2] == INT32_MIN && p[3] == INT32_MAX);
  enif_free(p);
  p = NULL;
  CHECK(get_i32_list(ENV, int_list(v, 0), 0, &p) && p != NULL);          /* []: a length like any other */
  enif_free(p);
  p = NULL;
  CHECK(!get_i32_list(ENV, int_list(v, 4), 3, &p) && p == NULL);         /* a wrong length, both ways */
  CHECK(!get_i32_list(ENV, int_list(v, 4), 5, &p) && p == NULL);
  CHECK(!get_i32_list(ENV, int_list(v, 0), 4, &p) && p == NULL);
  ERL_NIF_TERM mixed[3] = {fk_int(0), fk_int(1), fk_atom("two")};
  CHECK(!get_i32_list(ENV, fk_list(mixed, 3), 3, &p) && p == NULL);      /* an element that is no int: nothing leaks */
  mixed[0] = fk_double(0.0);
  CHECK(!get_i32_list(ENV, fk_list(mixed, 3), 3, &p) && p == NULL);
  mixed[0] = fk_int(1LL << 40);                                           /* no int32 */
  mixed[2] = fk_int(2);
  CHECK(!get_i32_list(ENV, fk_list(mixed, 3), 3, &p) && p == NULL);
  CHECK(!get_i32_list(ENV, fk_atom("none"), 0, &p) && p == NULL);        /* no list */
  CHECK(!get_i32_list(ENV, fk_binary(v, sizeof v), 4, &p) && p == NULL);
  CHECK(!get_i32_list(ENV, tuple_of(mixed, 3), 3, &p) && p == NULL);
  fk_reset();
}

static void raising(void) {
  (void)raise_msg(ENV, EXMC_ERR_BADARG, "not shown");
  CHECK(fk_badarg() == 1 && fk_exception() == 0);
  fk_reset();
  (void)raise_msg(ENV, EXMC_ERR_UNSUPPORTED, "this kind has no datums");
  ERL_NIF_TERM e = fk_exception();
  CHECK(fk_badarg() == 0 && e != 0 && fk_len(e) == 3);
  CHECK(strcmp(fk_get_str(fk_item(e, 0)), "exmc_hip_error") == 0 && fk_get_int(fk_item(e, 1)) == EXMC_ERR_UNSUPPORTED);
  CHECK(strcmp(fk_get_str(fk_item(e, 2)), "this kind has no datums") == 0);
  fk_reset();
  const nif_model refused = {-1, NULL, 0};                    /* leaves the stub's message behind */
  exmc_hip_model* m = NULL;
  int d;
  CHECK(model_open(&refused, 0, &m, &d, NULL) == EXMC_ERR_BADARG);
  (void)raise_hip(ENV, EXMC_ERR_HIP);
  e = fk_exception();
  CHECK(fk_badarg() == 0 && e != 0 && fk_len(e) == 3 && fk_get_int(fk_item(e, 1)) == EXMC_ERR_HIP);
  CHECK(strcmp(fk_get_str(fk_item(e, 2)), exmc_hip_last_error()) == 0 && strlen(exmc_hip_last_error()) > 0);
  fk_reset();
}

static void device(void) {
  CHECK(setenv("EXMC_HIP_DEVICE", "3", 1) == 0 && env_device() == 3);
  CHECK(g_device == 0 && load_device(ENV, NULL, 0) == 0 && g_device == 3);
  CHECK(unsetenv("EXMC_HIP_DEVICE") == 0 && env_device() == 0);
  CHECK(load_device(ENV, NULL, 0) == 0 && g_device == 0);
}

int main(void) {
  model_tuple();
  handle();
  i32_list();
  raising();
  device();
  puts("nif_frame_driver: ok");
  return 0;
}
