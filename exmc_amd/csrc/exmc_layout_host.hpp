// exmc_layout_host.hpp — the host-side layout changes between the caller's arrays (chain or fit first)
// and the device's (chain or fit last, the coalesced index). Plain loops over host memory: this header
// includes no HIP header, so tests/host/layout_host_shim.cpp compiles it for the CPU.
#pragma once

#include <cstddef>

namespace exmc {
namespace host __attribute__((visibility("hidden"))) {

// the caller's trace [C][n][d] into the device layout [n][d][C]
inline void chains_last(const double* src, double* dst, int n, int d, int C) {
  for (int c = 0; c < C; c++)
    for (int s = 0; s < n; s++)
      for (int i = 0; i < d; i++) dst[((size_t)s * d + i) * C + c] = src[((size_t)c * n + s) * d + i];
}

// [C][n][d] host <- [n][d][C] device-layout host copy
inline void transpose_trace_vec(const double* src, double* dst, int n, int d, int C) {
  for (int s = 0; s < n; s++)
    for (int i = 0; i < d; i++)
      for (int c = 0; c < C; c++) dst[((size_t)c * n + s) * d + i] = src[((size_t)s * d + i) * C + c];
}
template <class T>
void transpose_trace_scalar(const T* src, T* dst, int n, int C) {
  for (int s = 0; s < n; s++)
    for (int c = 0; c < C; c++) dst[(size_t)c * n + s] = src[(size_t)s * C + c];
}

// a device result [rows][C] (fit the fastest index) into the host's [C][rows]; dst may be null
template <class T>
void fits_first(const T* src, T* dst, size_t rows, size_t C) {
  if (!dst) return;
  for (size_t c = 0; c < C; c++)
    for (size_t i = 0; i < rows; i++) dst[c * rows + i] = src[i * C + c];
}

}  // namespace host
}  // namespace exmc
