/* Host build of exmc_tan_halfpi (include/exmc_detmath.h) for tests/prior_statement.py and
 * tests/test_detmath_tan.py (compiled with -ffp-contract=off). Test infrastructure only. */
#include "../../include/exmc_detmath.h"

double h_tan_halfpi(double u) { return exmc_tan_halfpi(u); }
void h_tan_halfpi_n(const double* u, long n, double* out) {
  for (long i = 0; i < n; i++) out[i] = exmc_tan_halfpi(u[i]);
}
