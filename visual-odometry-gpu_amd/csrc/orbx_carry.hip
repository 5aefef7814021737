// orbx_carry.hip -- landmarks carried from one generation of windows into the next: what the
// top-up's `origin` joins to, and what the next window's frames are localised against.  The reference re-detects at
// every solve (src/with_bundle_adjustment.cpp:586-593) and chains its poses (src/with_bundle_adjustment.cpp:196-208).
//   k_carry_join    one lane per (window, new slot): rule A, a binary search of the old window's ascending slot_of_point
//   k_carry_count   one wave per window: count[w], an integer sum that no launch shape changes
//   k_carry_gather  one workgroup per problem (window, frame k >= 0): rule B, compacted in ascending slot order into the
//                   rows k_pnp_ransac (orbx_pnp.hip) reads, with the problem's count (-1: nothing carried, rule D)
//   k_carry_fill    one lane per window: rule E
// Integer logic, copies and one float -> double widening: no arithmetic that rounds.  No atomics.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_lm_math.h"   // LM_OK
#include "orbx_pnp_math.h"  // PNP_OK
#include "orbx_wave.h"

namespace {

constexpr int CARRY_THREADS = 256;

__device__ __forceinline__ bool finite_bits(double v) {
  return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
__device__ __forceinline__ bool finite_bits(float v) {
  return (__builtin_bit_cast(unsigned int, v) & 0x7f800000u) != 0x7f800000u;
}

__global__ __launch_bounds__(CARRY_THREADS) void k_carry_join(const OrbxCarryIn in, const int32_t* __restrict__ origin,
                                                               int n_windows, int cap, double* __restrict__ xyz,
                                                               int32_t* __restrict__ point) {
  const long long at = (long long)blockIdx.x * CARRY_THREADS + threadIdx.x;
  if (at >= (long long)n_windows * cap) return;
  const int w = (int)(at / cap);
  int found = -1;
  double X[3] = {0.0, 0.0, 0.0};
  const int o = origin[at];
  if (in.status[w] == LM_OK && o >= 0 && o < in.old_cap) {
    const int p0 = in.pt_off[w], np = in.pt_off[w + 1] - p0;
    const int32_t* slot = in.slot + p0;
    int lo = 0, hi = np;  // the first j with slot[j] >= o; np <= 65536: at most 17 steps
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (slot[mid] < o) lo = mid + 1;
      else hi = mid;
    }
    if (lo < np && slot[lo] == o) {
      const double* src = in.src + 3 * ((size_t)p0 + lo);
      const double x = src[0], y = src[1], z = src[2];
      if (finite_bits(x) && finite_bits(y) && finite_bits(z)) found = lo, X[0] = x, X[1] = y, X[2] = z;
    }
  }
  xyz[3 * at] = X[0], xyz[3 * at + 1] = X[1], xyz[3 * at + 2] = X[2];
  point[at] = found;
}

__global__ __launch_bounds__(64) void k_carry_count(const int32_t* __restrict__ point, int cap,
                                                     int32_t* __restrict__ count) {
  const int w = blockIdx.x;
  const int32_t* P = point + (size_t)w * cap;
  int c = 0;
  for (int s = threadIdx.x; s < cap; s += 64) c += P[s] >= 0 ? 1 : 0;
  c = wave_sum(c);
  if (threadIdx.x == 0) count[w] = c;
}

__global__ __launch_bounds__(CARRY_THREADS) void k_carry_gather(const double* __restrict__ xyz,
                                                                 const int32_t* __restrict__ point,
                                                                 const int32_t* __restrict__ count,
                                                                 const float* __restrict__ tracks,
                                                                 const int32_t* __restrict__ seen, int cap, int len,
                                                                 OrbxPnpCorr* __restrict__ corr,
                                                                 int32_t* __restrict__ cidx,
                                                                 int32_t* __restrict__ ncorr) {
  __shared__ int scan[CARRY_THREADS / 64];
  const int tid = threadIdx.x;
  const int prob_i = blockIdx.x, w = prob_i / len, k = prob_i % len;
  if (count[w] == 0) {
    if (tid == 0) ncorr[prob_i] = -1;
    return;
  }
  OrbxPnpCorr* C = corr + (size_t)prob_i * cap;
  int32_t* CI = cidx + (size_t)prob_i * cap;
  const size_t s0 = (size_t)w * cap;
  int n = 0;
  for (int base = 0; base < cap; base += CARRY_THREADS) {
    const int s = base + tid;
    int has = 0;
    float px = 0.f, py = 0.f;
    if (s < cap && point[s0 + s] >= 0) {
      int sn = seen[s0 + s];
      sn = sn < 0 ? 0 : (sn > len ? len : sn);
      if (sn > k) {
        const float* t = tracks + 2 * ((s0 + s) * len + k);
        px = t[0], py = t[1];
        has = finite_bits(px) && finite_bits(py) ? 1 : 0;
      }
    }
    int total;
    const int at = n + block_scan_excl<CARRY_THREADS>(has, scan, &total);
    if (has) {  // (at < cap: at most one correspondence per slot)
      OrbxPnpCorr q;
      const double* X = xyz + 3 * (s0 + s);
      q.X[0] = X[0], q.X[1] = X[1], q.X[2] = X[2];
      q.x = (double)px, q.y = (double)py;
      C[at] = q;
      CI[at] = s;
    }
    n += total;
  }
  if (tid == 0) ncorr[prob_i] = n;
}

__global__ __launch_bounds__(64) void k_carry_fill(const OrbxPnpRecord* __restrict__ rec, int n_windows, int len,
                                                    double* __restrict__ poses6, int32_t* __restrict__ wstatus) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= n_windows) return;
  const OrbxPnpRecord* R = rec + (size_t)w * len;
  double* P = poses6 + 6 * (size_t)w * len;
  const bool lost = R[0].status != PNP_OK || R[1].status != PNP_OK;
  double prev[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < len; k++) {
    if (!lost && R[k].status == PNP_OK) {
#pragma unroll
      for (int i = 0; i < 6; i++) prev[i] = R[k].pose6[i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) P[6 * k + i] = prev[i];  // (lost: zeros throughout)
  }
  wstatus[w] = lost ? CARRY_LOST : CARRY_OK;
}

}  // namespace

hipError_t orbx_launch_carry_join(hipStream_t s, const OrbxCarryIn& in, const int32_t* d_origin, int n_windows, int cap,
                                  double* d_xyz, int32_t* d_point, int32_t* d_count) {
  if (n_windows <= 0 || cap <= 0) return hipSuccess;
  const long long lanes = (long long)n_windows * cap;
  hipLaunchKernelGGL(k_carry_join, dim3((unsigned)((lanes + CARRY_THREADS - 1) / CARRY_THREADS)), dim3(CARRY_THREADS), 0,
                     s, in, d_origin, n_windows, cap, d_xyz, d_point);
  hipLaunchKernelGGL(k_carry_count, dim3(n_windows), dim3(64), 0, s, d_point, cap, d_count);
  return hipGetLastError();
}

hipError_t orbx_launch_carry_gather(hipStream_t s, const double* d_xyz, const int32_t* d_point, const int32_t* d_count,
                                    const float* d_tracks, const int32_t* d_seen, int n_windows, int cap, int window_len,
                                    OrbxPnpCorr* d_corr, int32_t* d_cidx, int32_t* d_ncorr) {
  if (n_windows <= 0 || cap <= 0 || window_len <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_carry_gather, dim3(n_windows * window_len), dim3(CARRY_THREADS), 0, s, d_xyz, d_point, d_count,
                     d_tracks, d_seen, cap, window_len, d_corr, d_cidx, d_ncorr);
  return hipGetLastError();
}

hipError_t orbx_launch_carry_fill(hipStream_t s, const OrbxPnpRecord* d_rec, int n_windows, int window_len,
                                  double* d_poses6, int32_t* d_wstatus) {
  if (n_windows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_carry_fill, dim3((n_windows + 63) / 64), dim3(64), 0, s, d_rec, n_windows, window_len, d_poses6,
                     d_wstatus);
  return hipGetLastError();
}
