// orbx_gftt.hip -- batched Shi-Tomasi corner detection for gfx950.
//
// Replaces cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance) as called by
// src/with_bundle_adjustment.cpp:586-593 and src/t.cpp:285 (no mask, blockSize 3, gradientSize 3, minimum
// eigenvalue).  The rules are OpenCV 4.x's published algorithm with every choice it leaves to its SIMD build
// fixed (rules 1-6); tests/gftt_ref.py restates them in numpy, results are bit-identical.
//
// Kernels, each ONE launch for all frames of a batch slice
//   k_gftt_response    rule 1.  One wave per 60-column x 16-row tile streams the rows through registers: three
//                      byte-granular buffer loads per row and lane, Sobel / products / 3x3 box sums as exact
//                      integers (horizontal neighbours by lane shuffles, vertical ones in a three-row ring), the
//                      eigenvalue in the documented float32 sequence.  Writes the float map and reduces the frame's
//                      largest value in-wave, then one atomicMax per wave on the bit pattern (non-negative floats
//                      order like their bits).
//   k_gftt_candidates  rules 2-3.  A second pass over the map: the local-maximum test needs the finished frame
//                      maximum only through `e > thr`, but the map is written anyway for the stage entry
//                      (orbx_corner_min_eigen_val), and a candidate pool filtered by thr is a fifth of an unfiltered
//                      one on a camera frame (kitti_000000: 4122 of 21554 local maxima with e > 0; every weak
//                      maximum of a textured road qualifies) -- a shorter sort.  Emits 64-bit keys, response bits
//                      high, row-major index low, compacted per frame with one atomicAdd per wave; the pool holds
//                      (w - 2)(h - 2) keys per frame, so no candidate is ever dropped.
//   k_gftt_select      rules 4-6.  One workgroup per frame: bitonic sort of the keys, descending (the key is the
//                      whole order, ties by index descending included), then the FIRST WAVE walks the sorted list in
//                      chunks of 64 -- every lane tests its candidate against the accepted corners of the 3x3 cells
//                      around it, conflicts inside the chunk are resolved by a serial walk over the ballot of
//                      survivors -- which is sequential greedy selection done exactly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_internal.h"
#include "orbx_wave.h"

namespace {

#define GF_STRIP 60  // output columns of a wave: lanes 2..61 (lanes 0, 1, 62, 63 carry the two halo columns)
#define GF_BAND 16   // output rows of a wave

// REFLECT_101 for an index at most one step outside [0, len), len >= 2
__device__ __forceinline__ int gf_reflect(int p, int len) { return p < 0 ? -p : (p >= len ? 2 * len - 2 - p : p); }

// Rule 1, the float32 sequence (every operation rounded once, no contraction).  K = (float)(1 / 3060^2) is
// s^2 of OpenCV's scale s = 1 / (4 * 3 * 255) for CV_8U, aperture 3, block 3; 0.5f * K is exact.
//   a = (0.5 K) * (float)Sxx    b = K * (float)Sxy    c = (0.5 K) * (float)Syy
//   d = a - c    t = d * d + b * b    e = (a + c) - sqrt(t)
__device__ __forceinline__ float gf_min_eig(int sxx, int sxy, int syy) {
  const float K = (float)(1.0 / 9363600.0), KH = 0.5f * K;
  const float a = __fmul_rn(KH, (float)sxx), b = __fmul_rn(K, (float)sxy), c = __fmul_rn(KH, (float)syy);
  const float d = __fsub_rn(a, c);
  const float t = __fadd_rn(__fmul_rn(d, d), __fmul_rn(b, b));
  return __fsub_rn(__fadd_rn(a, c), sqrtf(t));  // correctly rounded (the build keeps HIP's default for sqrt)
}

// value of the lane below / above; the wave's end lanes get their own value back (never used)
__device__ __forceinline__ int gf_left(int v) { return __shfl_up(v, 1, 64); }
__device__ __forceinline__ int gf_right(int v) { return __shfl_down(v, 1, 64); }

__global__ __launch_bounds__(256) void k_gftt_response(const uint8_t* __restrict__ frames, int w, int h, int row_stride,
                                                       size_t frame_stride, float* __restrict__ map,
                                                       uint32_t* __restrict__ fmax) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int f = blockIdx.z;
  const int y0 = (blockIdx.y * 4 + wave) * GF_BAND;
  if (y0 >= h) return;  // whole wave
  const int y1 = min(y0 + GF_BAND, h);
  const int x = blockIdx.x * GF_STRIP - 2 + lane;
  // the frame's bytes exactly; a lane outside the image reads a column inside it (its values are never used), so
  // every load is in range
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(frames) + (size_t)f * frame_stride, 0, row_stride * (h - 1) + w, 0x00020000);
  const uint32_t voff = (uint32_t)min(max(x, 0), w - 1);
  const bool first = x == 0, last = x == w - 1;
  const bool writes = lane >= 2 && lane <= 61 && x < w;
  float* out = map + (size_t)f * ((size_t)w * h);
  int h0xx = 0, h0xy = 0, h0yy = 0, h1xx = 0, h1xy = 0, h1yy = 0;
  float m = 0.f;
  // v: row of the product maps, one beyond the band on either side; outside the image it is the reflected row of
  // the PRODUCT maps (boxFilter's border), whose Sobel in turn reflects the image rows
  for (int v = y0 - 1; v <= y1; v++) {
    const int pr = gf_reflect(v, h);
    const int ra = gf_reflect(pr - 1, h), rc = gf_reflect(pr + 1, h);
    const int pa = __builtin_amdgcn_raw_buffer_load_b8(rsrc, voff, ra * row_stride, 0);
    const int pb = __builtin_amdgcn_raw_buffer_load_b8(rsrc, voff, pr * row_stride, 0);
    const int pc = __builtin_amdgcn_raw_buffer_load_b8(rsrc, voff, rc * row_stride, 0);
    const int s = pa + 2 * pb + pc, d = pc - pa;  // column smoothing and column difference of the 3x3 Sobel
    int sl = gf_left(s), sr = gf_right(s), dl = gf_left(d), dr = gf_right(d);
    if (first) sl = sr, dl = dr;  // image column -1 is column 1
    if (last) sr = sl, dr = dl;
    const int gx = sr - sl, gy = dl + 2 * d + dr;
    const int pxx = gx * gx, pxy = gx * gy, pyy = gy * gy;
    int lxx = gf_left(pxx), rxx = gf_right(pxx), lxy = gf_left(pxy), rxy = gf_right(pxy), lyy = gf_left(pyy),
        ryy = gf_right(pyy);
    if (first) lxx = rxx, lxy = rxy, lyy = ryy;  // product column -1 is product column 1
    if (last) rxx = lxx, rxy = lxy, ryy = lyy;
    const int hxx = pxx + lxx + rxx, hxy = pxy + lxy + rxy, hyy = pyy + lyy + ryy;
    if (v > y0) {
      const float e = gf_min_eig(h0xx + h1xx + hxx, h0xy + h1xy + hxy, h0yy + h1yy + hyy);
      if (writes) {
        out[(size_t)(v - 1) * w + x] = e;
        if (e > m) m = e;
      }
    }
    h0xx = h1xx, h0xy = h1xy, h0yy = h1yy;
    h1xx = hxx, h1xy = hxy, h1yy = hyy;
  }
  uint32_t mb = __float_as_uint(m);  // m >= 0
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) mb = max(mb, (uint32_t)__shfl_xor((int)mb, dlt, 64));
  if (lane == 0 && mb != 0u) atomicMax(&fmax[f], mb);
}

// Rule 2: thr = (float)((double)max * quality); a frame whose largest value is not positive has no corner.  A value
// that is not above thr -- every non-positive one among them, thr being positive -- is 0 in the thresholded map and
// never a corner.  Rule 3 on interior pixels: all eight neighbours are inside the image, and `value == maximum of the
// thresholded 3x3` is `e >= each neighbour's e` for a value above thr (a neighbour below thr counts as 0 < e).
__global__ __launch_bounds__(256) void k_gftt_candidates(const float* __restrict__ map, int w, int h,
                                                         const uint32_t* __restrict__ fmax, double quality,
                                                         unsigned long long* __restrict__ keys, size_t pool,
                                                         int32_t* __restrict__ ncand) {
  const int f = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const float mx = __uint_as_float(fmax[f]);
  bool cand = false;
  float e = 0.f;
  if (mx > 0.f && x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
    const float thr = (float)((double)mx * quality);
    const float* p = map + (size_t)f * ((size_t)w * h) + (size_t)y * w + x;
    e = p[0];
    if (e > thr) {
      const float* a = p - w;
      const float* c = p + w;
      cand = e >= a[-1] && e >= a[0] && e >= a[1] && e >= p[-1] && e >= p[1] && e >= c[-1] && e >= c[0] && e >= c[1];
    }
  }
  const unsigned long long bal = __ballot(cand);
  if (bal == 0ull) return;  // whole wave
  int base = 0;
  if (lane == 0) base = atomicAdd(&ncand[f], (int)__popcll(bal));
  base = __builtin_amdgcn_readfirstlane(base);
  if (cand) {
    const int rank = (int)__popcll(bal & ((1ull << lane) - 1ull));
    // base + rank < (w - 2)(h - 2) = pool: every interior pixel is counted at most once
    keys[(size_t)f * pool + (size_t)(base + rank)] =
        ((unsigned long long)__float_as_uint(e) << 32) | (unsigned long long)(uint32_t)(y * w + x);
  }
}

#define GF_SELECT_THREADS 1024
#define GF_LDS_KEYS 8192  // lists up to this length are sorted in LDS (64 KB)
#define GF_EMPTY 0xffffffffu

__device__ __forceinline__ void gf_cmpswap(unsigned long long* a, int lo, int hi) {
  const unsigned long long u = a[lo], v = a[hi];
  if (v > u) a[lo] = v, a[hi] = u;
}

// Bitonic sorting network in which EVERY compare-exchange puts the larger key at the lower index (a merge step
// starts with the mirrored pairing instead of alternating directions), over the next power of two P >= n: the
// positions n..P-1 stand for keys smaller than any real one, which such a network never moves, so pairs that reach
// them are skipped and the list needs no padding.
__device__ void gf_sort_desc(unsigned long long* a, int n) {
  int P = 1;
  while (P < n) P <<= 1;
  const int half = P >> 1;
  for (int k = 2; k <= P; k <<= 1) {
    const int kh = k >> 1;
    for (int i = threadIdx.x; i < half; i += GF_SELECT_THREADS) {
      const int blk = i / kh, off = i - blk * kh;
      const int lo = blk * k + off, hi = blk * k + k - 1 - off;
      if (hi < n) gf_cmpswap(a, lo, hi);
    }
    __syncthreads();
    for (int j = k >> 2; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < half; i += GF_SELECT_THREADS) {
        const int lo = 2 * j * (i / j) + (i % j), hi = lo + j;
        if (hi < n) gf_cmpswap(a, lo, hi);
      }
      __syncthreads();
    }
  }
}

// Rules 4-6.  grid: gw x gh cells of `slots` packed corners (x | y << 16, GF_EMPTY: free), filled with 0xff by the
// host before the launch (not read when min_dist < 1).
// Cell occupancy: cell = cvRound(d) with d >= 1, so cell - 0.5 <= d.  A cell spans cell x cell integer positions,
// side L = cell - 1.  cell == 1: one position, one corner.  cell >= 2: of any five points in a square of side L two
// share one of its four closed quadrants of side L / 2 and are at most L / sqrt(2) < L < d apart, so a cell never
// holds more than FOUR accepted corners.  Reach: a corner two cells away differs by at least cell + 1 > d in one
// coordinate (d <= cell + 0.5), so the 3x3 cells around a candidate hold every corner that can reject it.
__global__ __launch_bounds__(GF_SELECT_THREADS) void k_gftt_select(unsigned long long* __restrict__ keys, size_t pool,
                                                                   const int32_t* __restrict__ ncand, int w,
                                                                   float d2, int suppress, int cell, int gw, int gh,
                                                                   int slots, uint32_t* __restrict__ grid,
                                                                   size_t grid_stride, int cap,
                                                                   int32_t* __restrict__ counts,
                                                                   float2* __restrict__ corners) {
  __shared__ unsigned long long s_keys[GF_LDS_KEYS];
  const int f = blockIdx.x;
  const int n = ncand[f];
  unsigned long long* gk = keys + (size_t)f * pool;
  float2* out = corners + (size_t)f * cap;
  if (n <= 0) {
    if (threadIdx.x == 0) counts[f] = 0;
    return;
  }
  const bool in_lds = n <= GF_LDS_KEYS;
  unsigned long long* a = gk;
  if (in_lds) {
    for (int i = threadIdx.x; i < n; i += GF_SELECT_THREADS) s_keys[i] = gk[i];
    __syncthreads();
    a = s_keys;
  }
  gf_sort_desc(a, n);  // ends with a barrier
  if (!suppress) {  // min_dist < 1: every candidate in order
    const int m = min(n, cap);
    for (int i = threadIdx.x; i < m; i += GF_SELECT_THREADS) {
      const uint32_t idx = (uint32_t)a[i];
      const uint32_t y = idx / (uint32_t)w;
      out[i] = make_float2((float)(idx - y * (uint32_t)w), (float)y);
    }
    if (threadIdx.x == 0) counts[f] = m;
    return;
  }
  if (threadIdx.x >= 64) return;  // the walk is the first wave's
  const int lane = threadIdx.x;
  uint32_t* g = grid + (size_t)f * grid_stride;
  int count = 0;
  for (int base = 0; base < n && count < cap; base += 64) {
    const int i = base + lane;
    const bool valid = i < n;
    const uint32_t idx = valid ? (uint32_t)a[i] : 0u;
    const int y = (int)(idx / (uint32_t)w), x = (int)idx - y * w;
    const int cx = x / cell, cy = y / cell;
    bool alive = valid;
    int own = 0;  // corners already in the candidate's own cell
    if (valid) {
      const int cx0 = max(cx - 1, 0), cx1 = min(cx + 1, gw - 1), cy0 = max(cy - 1, 0), cy1 = min(cy + 1, gh - 1);
      for (int yy = cy0; yy <= cy1; yy++)
        for (int xx = cx0; xx <= cx1; xx++) {
          const uint32_t* c = g + (size_t)(yy * gw + xx) * slots;
          for (int s = 0; s < slots; s++) {
            const uint32_t v = c[s];
            if (v == GF_EMPTY) break;  // a cell fills from slot 0
            const int dx = x - (int)(v & 0xffffu), dy = y - (int)(v >> 16);
            if ((float)(dx * dx + dy * dy) < d2) alive = false;
            if (xx == cx && yy == cy) own++;
          }
        }
    }
    // conflicts inside the chunk: the first surviving lane is accepted, rejects the survivors it is too close to
    // (itself among them: distance 0 < d2), and so on -- the order of the sorted list
    unsigned long long live = __ballot(alive);
    while (live != 0ull && count < cap) {
      const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(live));
      const int ax = __builtin_amdgcn_readlane(x, l), ay = __builtin_amdgcn_readlane(y, l);
      if (lane == l) {
        out[count] = make_float2((float)x, (float)y);
        if (own < slots) g[(size_t)(cy * gw + cx) * slots + own] = (uint32_t)x | ((uint32_t)y << 16);
      }
      const int dx = x - ax, dy = y - ay;
      const bool hit = alive && (float)(dx * dx + dy * dy) < d2;
      // the accepted corner took a slot of this lane's cell
      if (alive && lane != l && ax / cell == cx && ay / cell == cy) own++;
      if (hit) alive = false;
      live &= ~__ballot(hit);
      count++;
    }
    // the next chunk reads the cells this one wrote (other lanes of the same wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  if (lane == 0) counts[f] = count;
}

}  // namespace

hipError_t orbx_launch_gftt_response(hipStream_t s, const uint8_t* d_frames, int n, int w, int h, int row_stride,
                                     size_t frame_stride, float* d_map, uint32_t* d_max) {
  const dim3 grid((w + GF_STRIP - 1) / GF_STRIP, ((h + GF_BAND - 1) / GF_BAND + 3) / 4, n);
  hipLaunchKernelGGL(k_gftt_response, grid, dim3(256), 0, s, d_frames, w, h, row_stride, frame_stride, d_map, d_max);
  return hipGetLastError();
}

hipError_t orbx_launch_gftt_candidates(hipStream_t s, const float* d_map, int n, int w, int h, const uint32_t* d_max,
                                       double quality, unsigned long long* d_keys, size_t pool, int32_t* d_ncand) {
  const dim3 grid((w + 63) / 64, (h + 3) / 4, n);
  hipLaunchKernelGGL(k_gftt_candidates, grid, dim3(256), 0, s, d_map, w, h, d_max, quality, d_keys, pool, d_ncand);
  return hipGetLastError();
}

hipError_t orbx_launch_gftt_select(hipStream_t s, int n, int w, unsigned long long* d_keys, size_t pool,
                                   const int32_t* d_ncand, double min_distance, int cell, int gw, int gh, int slots,
                                   uint32_t* d_grid, size_t grid_stride, int cap, int32_t* d_counts,
                                   float* d_corners) {
  const float d2 = (float)(min_distance * min_distance);
  hipLaunchKernelGGL(k_gftt_select, dim3(n), dim3(GF_SELECT_THREADS), 0, s, d_keys, pool, d_ncand, w, d2,
                     min_distance >= 1.0 ? 1 : 0, cell, gw, gh, slots, d_grid, grid_stride, cap, d_counts,
                     reinterpret_cast<float2*>(d_corners));
  return hipGetLastError();
}
