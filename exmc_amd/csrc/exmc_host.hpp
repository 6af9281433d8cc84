// exmc_host.hpp — what the two host units of a library share: exmc_common.hip (model-free, built
// once) and exmc_hip.hip (the handle and all that names a model type). Hidden visibility: two
// libraries in one process (libexmc_hip.so and a plug-in) never reach into each other.
#pragma once

#include "../../include/exmc_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

namespace exmc {
namespace host __attribute__((visibility("hidden"))) {

// keeps `msg` for exmc_hip_last_error (one string per library and thread, exmc_common.hip); returns `code`
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(EXMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

inline double f32r(double x) { return (double)(float)x; }
inline double log2pi32() { return f32r(std::log(f32r(2.0 * M_PI))); }

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return EXMC_OK;
    release();
    HIP_TRY(hipMalloc(&p, bytes));
    cap = bytes;
    return EXMC_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// one device allocation that lives for one call
struct CallBuf {
  void* p = nullptr;
  ~CallBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes) {
    HIP_TRY(hipMalloc(&p, bytes ? bytes : 8));
    return EXMC_OK;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// makes `device` current; EXMC_ERR_NO_DEVICE without one, EXMC_ERR_BADARG out of range
int select_device(int device);

// ---- the diagnostics launches (exmc_common.hip), over a [S][D][C] device array, asynchronous ----
// Diagnostics.ess of every series; `work` holds the worklist of the series that need the tail kernel
int launch_ess(hipStream_t stream, DevBuf& work, const double* src, int n_draws, int d, int n_chains,
               double* ess_dev);
// the normal scores of the ranks of `draws` into `scores`, same shape; rank_scores_lds (the LDS
// opt-in of a long series) goes first, outside the caller's timed region
int rank_scores_lds(int n_draws);
int launch_rank_scores(hipStream_t stream, const double* draws, int n_draws, int d, int n_chains,
                       double* scores);
// Diagnostics.rhat of every dimension; `stats`: scratch of d * 4 * n_chains doubles
int launch_rhat(hipStream_t stream, const double* draws, int n_draws, int d, int n_chains, double* stats,
                double* rhat_dev);
// exmc_hip_convergence over draws [S][D][C] into out_dev [6][D]; allocates its scratch (at most
// `scratch_bytes`, never less than one dimension's), records `start` in front of the first launch and
// returns when the stream has drained
int launch_convergence(hipStream_t stream, hipEvent_t start, const double* draws, int n_draws, int d,
                       int n_chains, size_t scratch_bytes, double* out_dev);

}  // namespace host
}  // namespace exmc
