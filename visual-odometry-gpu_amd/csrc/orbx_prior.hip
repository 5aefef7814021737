// orbx_prior.hip -- landmark priors of a carried window (rule P6): every landmark of the
// current landmarks block that was carried from the last generation gets its old coordinates as an anchor, so that the
// solve (k_ba_lm<true>, orbx_ba.hip) keeps the carried window on the map it came from.  The reference keeps no point
// across a solve, it re-detects (src/with_bundle_adjustment.cpp:586-593).
//   k_prior_gather  one lane per (window, landmark j): s = slot_of_point[j]; carried (the carry block's point[w][s] >= 0)
//                   -> the bits of xyz[w][s] and the weight, otherwise four zeros
//   k_prior_count   one wave per window: count[w] = the landmarks with a prior, by ballot and popcount
// Copies and integer logic only: no arithmetic that rounds.  No atomics.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_lm_math.h"  // LM_OK

namespace {

constexpr int PRIOR_THREADS = 256;

// grid: `blocks` workgroups of PRIOR_THREADS landmarks per window
__global__ __launch_bounds__(PRIOR_THREADS) void k_prior_gather(const int32_t* __restrict__ status,
                                                                 const int32_t* __restrict__ pt_off,
                                                                 const int32_t* __restrict__ slot_of_point,
                                                                 const double* __restrict__ carry_xyz,
                                                                 const int32_t* __restrict__ carry_point, int cap,
                                                                 int blocks, double weight,
                                                                 double* __restrict__ prior) {
  const int w = blockIdx.x / blocks;
  const int j = (blockIdx.x % blocks) * PRIOR_THREADS + threadIdx.x;
  const int p0 = pt_off[w], np = pt_off[w + 1] - p0;  // (a window that is not LM_OK owns no landmark: np = 0)
  if (j >= np) return;
  const int s = slot_of_point[p0 + j];
  double A[3] = {0.0, 0.0, 0.0}, lam = 0.0;
  if (status[w] == LM_OK && s >= 0 && s < cap) {  // (a landmark's slot always is: the test keeps a damaged block from reading outside)
    const size_t at = (size_t)w * cap + s;
    if (carry_point[at] >= 0) A[0] = carry_xyz[3 * at], A[1] = carry_xyz[3 * at + 1], A[2] = carry_xyz[3 * at + 2], lam = weight;
  }
  double* out = prior + 4 * ((size_t)p0 + j);
  out[0] = A[0], out[1] = A[1], out[2] = A[2], out[3] = lam;
}

__global__ __launch_bounds__(64) void k_prior_count(const int32_t* __restrict__ status,
                                                     const int32_t* __restrict__ pt_off,
                                                     const int32_t* __restrict__ slot_of_point,
                                                     const int32_t* __restrict__ carry_point, int cap,
                                                     int32_t* __restrict__ count) {
  const int w = blockIdx.x;
  const int p0 = pt_off[w], np = status[w] == LM_OK ? pt_off[w + 1] - p0 : 0;
  int c = 0;
  for (int base = 0; base < np; base += 64) {  // (uniform trip count: every lane reaches the ballot)
    const int j = base + (int)threadIdx.x;
    bool has = false;
    if (j < np) {
      const int s = slot_of_point[p0 + j];
      has = s >= 0 && s < cap && carry_point[(size_t)w * cap + s] >= 0;
    }
    c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(has));
  }
  if (threadIdx.x == 0) count[w] = c;
}

}  // namespace

hipError_t orbx_launch_prior_gather(hipStream_t s, const int32_t* d_status, const int32_t* d_pt_off,
                                    const int32_t* d_slot_of_point, const double* d_carry_xyz,
                                    const int32_t* d_carry_point, int n_windows, int cap, double weight,
                                    double* d_prior, int32_t* d_count) {
  if (n_windows < 1 || cap < 1 || cap > ORBX_BA_MAX_POINTS || !(weight >= 0.0)) return hipErrorInvalidValue;
  const int blocks = (cap + PRIOR_THREADS - 1) / PRIOR_THREADS;  // n_windows * blocks <= n_windows * cap < 2^31
  hipLaunchKernelGGL(k_prior_gather, dim3((unsigned)n_windows * blocks), dim3(PRIOR_THREADS), 0, s, d_status, d_pt_off,
                     d_slot_of_point, d_carry_xyz, d_carry_point, cap, blocks, weight, d_prior);
  hipLaunchKernelGGL(k_prior_count, dim3(n_windows), dim3(64), 0, s, d_status, d_pt_off, d_slot_of_point, d_carry_point,
                     cap, d_count);
  return hipGetLastError();
}
