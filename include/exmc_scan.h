/* exmc_scan.h — the association order of the 64-lane prefix and suffix sums, in plain C.
 *
 * exmc_amd/csrc/exmc_device.hpp wave_scan_fwd / wave_scan_bwd sum a chain's values over the 64
 * lanes of a wavefront and N register slots (element 64 k + l in slot k of lane l). Their order of
 * additions is part of the numeric contract: the host statement of a
 * generated lane layout (exmc_amd/codegen_lanes.py, scan chains) runs these functions where the
 * device runs the wave-wide scans, and gets the same bits.
 *
 * Forward, slot by slot:
 *   1. inside each 16-lane row, Hillis-Steele: for d = 1, 2, 4, 8 a lane whose row position is
 *      >= d adds the value d lanes below;
 *   2. rows 1 and 3 add the total of the row below; rows 2 and 3 add (total 0 + total 1), the row
 *      totals taken after stage 1;
 *   3. slot k adds the last element of slot k - 1 (after that slot's own carry).
 * Backward is the mirror image: row_shl, row totals at row position 0, rows 0 and 2 add the row
 * above, rows 0 and 1 add (total 2 + total 3), slot k adds the first element of slot k + 1.
 * Every stage selects; nothing is multiplied by a 0 standing in for "no value".
 *
 * x holds 64 * nslots doubles in element order (x[64 k + l] = slot k of lane l). Compile with
 * -ffp-contract=off, like every user of exmc_detmath.h. */
#ifndef EXMC_SCAN_H
#define EXMC_SCAN_H

#include <string.h>

static inline void exmc_scan_fwd_slot64(double* v) {
  double n[64], t[64], t2[64];
  for (int d = 1; d < 16; d <<= 1) {
    for (int l = 0; l < 64; l++) n[l] = ((l & 15) >= d) ? v[l] + v[l - d] : v[l];
    memcpy(v, n, sizeof n);
  }
  for (int l = 0; l < 64; l++) t[l] = v[(l & ~15) + 15];
  for (int l = 0; l < 64; l++) {
    const double p = t[l ^ 16];
    if (l & 16) v[l] = v[l] + p;
    t2[l] = t[l] + p;
  }
  for (int l = 0; l < 64; l++)
    if (l & 32) v[l] = v[l] + t2[l ^ 32];
}

static inline void exmc_scan_bwd_slot64(double* v) {
  double n[64], t[64], t2[64];
  for (int d = 1; d < 16; d <<= 1) {
    for (int l = 0; l < 64; l++) n[l] = ((l & 15) + d < 16) ? v[l] + v[l + d] : v[l];
    memcpy(v, n, sizeof n);
  }
  for (int l = 0; l < 64; l++) t[l] = v[l & ~15];
  for (int l = 0; l < 64; l++) {
    const double p = t[l ^ 16];
    if (!(l & 16)) v[l] = v[l] + p;
    t2[l] = t[l] + p;
  }
  for (int l = 0; l < 64; l++)
    if (!(l & 32)) v[l] = v[l] + t2[l ^ 32];
}

/* x[i] <- x[0] + ... + x[i] */
static inline void exmc_scan_fwd64(double* x, int nslots) {
  for (int k = 0; k < nslots; k++) exmc_scan_fwd_slot64(x + 64 * k);
  for (int k = 1; k < nslots; k++) {
    const double carry = x[64 * k - 1];
    for (int l = 0; l < 64; l++) x[64 * k + l] = x[64 * k + l] + carry;
  }
}

/* x[i] <- x[i] + ... + x[64 nslots - 1] */
static inline void exmc_scan_bwd64(double* x, int nslots) {
  for (int k = 0; k < nslots; k++) exmc_scan_bwd_slot64(x + 64 * k);
  for (int k = nslots - 2; k >= 0; k--) {
    const double carry = x[64 * (k + 1)];
    for (int l = 0; l < 64; l++) x[64 * k + l] = x[64 * k + l] + carry;
  }
}

/* group_allsum_n over 64 lanes: part[l] is lane l's partial; the xor butterfly, every lane's total
 * the same bits; returns it */
static inline double exmc_allsum64(double* part) {
  double nxt[64];
  for (int m = 1; m < 64; m <<= 1) {
    for (int l = 0; l < 64; l++) nxt[l] = part[l] + part[l ^ m];
    memcpy(part, nxt, sizeof nxt);
  }
  return part[0];
}

#endif
