// tan_probe.hip -- exmc_tan_halfpi (include/exmc_detmath.h) evaluated on the device for the doubles of a file:
//   tan_probe IN OUT     IN: n native-endian doubles; OUT: the n results
// tests/test_gpu_prior.py compares OUT with the host build of the same header, bit for bit.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I include -o tools/probe/tan_probe tools/probe/tan_probe.hip
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "exmc_detmath.h"

__global__ void tan_kernel(const double* __restrict__ u, double* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = exmc_tan_halfpi(u[i]);
}

#define TRY(x)                                                                   \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));               \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: tan_probe IN OUT\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f) / 8;
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> h((size_t)n), r((size_t)n);
  if (n < 1 || std::fread(h.data(), 8, (size_t)n, f) != (size_t)n) return 2;
  std::fclose(f);
  double *du, *dout;
  TRY(hipMalloc(&du, (size_t)n * 8));
  TRY(hipMalloc(&dout, (size_t)n * 8));
  TRY(hipMemcpy(du, h.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(tan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, du, dout, n);
  TRY(hipGetLastError());
  TRY(hipMemcpy(r.data(), dout, (size_t)n * 8, hipMemcpyDeviceToHost));
  TRY(hipFree(du));
  TRY(hipFree(dout));
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(r.data(), 8, (size_t)n, f) != (size_t)n) return 2;
  std::fclose(f);
  std::printf("tan_probe: %ld values\n", n);
  return 0;
}
