// Host build of the library's layout loops (exmc_amd/csrc/exmc_layout_host.hpp) for
// tests/test_layout_host.py, and with -DLAYOUT_HOST_MAIN a stand-alone program that runs the same
// shapes against the index formulas (for a sanitizer build: g++ -fsanitize=address,undefined
// -DLAYOUT_HOST_MAIN ... && ./a.out). Test infrastructure only.
#include "../../exmc_amd/csrc/exmc_layout_host.hpp"

#include <cstdint>

using namespace exmc::host;

extern "C" {
void layout_chains_last(const double* src, double* dst, int n, int d, int C) { chains_last(src, dst, n, d, C); }
void layout_trace_vec(const double* src, double* dst, int n, int d, int C) { transpose_trace_vec(src, dst, n, d, C); }
void layout_trace_scalar_f64(const double* src, double* dst, int n, int C) { transpose_trace_scalar(src, dst, n, C); }
void layout_trace_scalar_i32(const int32_t* src, int32_t* dst, int n, int C) { transpose_trace_scalar(src, dst, n, C); }
void layout_fits_first_f64(const double* src, double* dst, long rows, long C) {
  fits_first(src, dst, (size_t)rows, (size_t)C);
}
void layout_fits_first_i32(const int32_t* src, int32_t* dst, long rows, long C) {
  fits_first(src, dst, (size_t)rows, (size_t)C);
}
}

#ifdef LAYOUT_HOST_MAIN
#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);             \
      bad++;                                                             \
    }                                                                    \
  } while (0)

static void trace_shape(int C, int S, int d) {
  const size_t n = (size_t)C * S * d;
  std::vector<double> host(n), dev(n, -1.0), back(n, -1.0);   // exactly n each: a stray index is out of bounds
  for (size_t i = 0; i < n; i++) host[i] = (double)i + 0.25;
  chains_last(host.data(), dev.data(), S, d, C);
  for (int c = 0; c < C; c++)
    for (int s = 0; s < S; s++)
      for (int j = 0; j < d; j++)
        CHECK(dev[((size_t)s * d + j) * C + c] == host[((size_t)c * S + s) * d + j]);
  transpose_trace_vec(dev.data(), back.data(), S, d, C);
  CHECK(back == host);
  // a scalar trace [S][C] -> [C][S], both element types
  std::vector<double> sd((size_t)S * C), sh((size_t)S * C, -1.0);
  std::vector<int32_t> id((size_t)S * C), ih((size_t)S * C, -1);
  for (size_t i = 0; i < sd.size(); i++) {
    sd[i] = (double)i - 0.5;
    id[i] = (int32_t)i;
  }
  transpose_trace_scalar(sd.data(), sh.data(), S, C);
  transpose_trace_scalar(id.data(), ih.data(), S, C);
  for (int c = 0; c < C; c++)
    for (int s = 0; s < S; s++) {
      CHECK(sh[(size_t)c * S + s] == sd[(size_t)s * C + c]);
      CHECK(ih[(size_t)c * S + s] == id[(size_t)s * C + c]);
    }
}

static void fits_shape(size_t rows, size_t C) {
  std::vector<double> src(rows * C), dst(rows * C, -1.0);
  std::vector<int32_t> isrc(rows * C), idst(rows * C, -1);
  for (size_t i = 0; i < src.size(); i++) {
    src[i] = (double)i + 0.5;
    isrc[i] = (int32_t)i;
  }
  fits_first(src.data(), dst.data(), rows, C);
  fits_first(isrc.data(), idst.data(), rows, C);
  for (size_t c = 0; c < C; c++)
    for (size_t i = 0; i < rows; i++) {
      CHECK(dst[c * rows + i] == src[i * C + c]);
      CHECK(idst[c * rows + i] == isrc[i * C + c]);
    }
  fits_first(src.data(), (double*)nullptr, rows, C);   // a null dst is accepted and nothing is written
  fits_first(isrc.data(), (int32_t*)nullptr, rows, C);
}

int main() {
  trace_shape(1, 1, 1);
  trace_shape(3, 2, 5);
  trace_shape(65, 2, 3);
  fits_shape(1, 1);
  fits_shape(5, 3);
  std::printf(bad ? "layout_host: %d checks FAILED\n" : "layout_host: all shapes ok\n", bad);
  return bad ? 1 : 0;
}
#endif
