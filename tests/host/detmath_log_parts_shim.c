/* Host build of the separated logarithm of include/exmc_detmath.h -- the main path both exmc_log_ge1 and
 * exmc_log_unit evaluate, and the fix-up of each -- for tests/test_detmath_log_parts.py (compiled with
 * -ffp-contract=off). Test infrastructure only. */
#include "../../include/exmc_detmath.h"

double h_ge1_parts(double x) { return exmc_log_ge1_fix(x, exmc_log_main(x)); }
double h_unit_parts(double x) { return exmc_log_unit_fix(x, exmc_log_main(x)); }
double h_log_ge1(double x) { return exmc_log_ge1(x); }
double h_log_unit(double x) { return exmc_log_unit(x); }
/* the number of values for which main path + fix-up differs in its bits from the range function
 * (which = 0: exmc_log_ge1, 1: exmc_log_unit) or from the general exmc_log */
long h_parts_compare(int which, const double* x, long n) {
  long bad = 0;
  for (long i = 0; i < n; i++) {
    const double m = exmc_log_main(x[i]);
    const double a = which ? exmc_log_unit_fix(x[i], m) : exmc_log_ge1_fix(x[i], m);
    const double b = which ? exmc_log_unit(x[i]) : exmc_log_ge1(x[i]);
    const double c = exmc_log(x[i]);
    bad += __builtin_memcmp(&a, &b, 8) != 0;
    bad += __builtin_memcmp(&a, &c, 8) != 0;
  }
  return bad;
}
