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
// Rank 12 (masked detection that tops up tracked points; rules A-F, tests/gftt_topup_ref.py) adds, further down:
//   k_gftt_seeds, k_gftt_block, k_gftt_mask_bits, k_gftt_masked_max, k_gftt_candidates_blocked, k_gftt_select_topup;
//   the candidate pass and the sort / walk are shared device functions, so the kernels above compute what they did.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

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
// One text for the plain pass and for the pass with blocked pixels (rank 12, rules D-E).  BLOCKED: `fmax` is the
// largest value among the pixels that are not blocked, and a pixel whose bit is set in `bits` (row-major, wp words
// per row, bit x & 31 of word x >> 5) is no candidate; blocked NEIGHBOURS still take part in the 3x3 maximum.
template <bool BLOCKED>
__device__ __forceinline__ void gf_candidates(const float* __restrict__ map, int w, int h,
                                              const uint32_t* __restrict__ fmax, double quality,
                                              unsigned long long* __restrict__ keys, size_t pool,
                                              int32_t* __restrict__ ncand, const uint32_t* __restrict__ bits, int wp) {
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
      if (BLOCKED && cand) cand = !((bits[(size_t)f * ((size_t)wp * h) + (size_t)y * wp + (x >> 5)] >> (x & 31)) & 1u);
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

__global__ __launch_bounds__(256) void k_gftt_candidates(const float* __restrict__ map, int w, int h,
                                                         const uint32_t* __restrict__ fmax, double quality,
                                                         unsigned long long* __restrict__ keys, size_t pool,
                                                         int32_t* __restrict__ ncand) {
  gf_candidates<false>(map, w, h, fmax, quality, keys, pool, ncand, nullptr, 0);
}

__global__ __launch_bounds__(256) void k_gftt_candidates_blocked(const float* __restrict__ map, int w, int h,
                                                                 const uint32_t* __restrict__ fmax, double quality,
                                                                 unsigned long long* __restrict__ keys, size_t pool,
                                                                 int32_t* __restrict__ ncand,
                                                                 const uint32_t* __restrict__ bits, int wp) {
  gf_candidates<true>(map, w, h, fmax, quality, keys, pool, ncand, bits, wp);
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
// The sort and the walk of one frame, shared by k_gftt_select and k_gftt_select_topup: gk / n the frame's keys, g its
// cells, `cap` corners at most to out[0 .. cap), *count = count_base + corners written.
__device__ __forceinline__ void gf_select_frame(unsigned long long* s_keys, unsigned long long* __restrict__ gk, int n,
                                                int w, float d2, int suppress, int cell, int gw, int gh, int slots,
                                                uint32_t* __restrict__ g, int cap, int count_base,
                                                int32_t* __restrict__ count_out, float2* __restrict__ out) {
  if (n <= 0 || cap <= 0) {
    if (threadIdx.x == 0) *count_out = count_base;
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
    if (threadIdx.x == 0) *count_out = count_base + m;
    return;
  }
  if (threadIdx.x >= 64) return;  // the walk is the first wave's
  const int lane = threadIdx.x;
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
  if (lane == 0) *count_out = count_base + count;
}

__global__ __launch_bounds__(GF_SELECT_THREADS) void k_gftt_select(unsigned long long* __restrict__ keys, size_t pool,
                                                                   const int32_t* __restrict__ ncand, int w,
                                                                   float d2, int suppress, int cell, int gw, int gh,
                                                                   int slots, uint32_t* __restrict__ grid,
                                                                   size_t grid_stride, int cap,
                                                                   int32_t* __restrict__ counts,
                                                                   float2* __restrict__ corners) {
  __shared__ unsigned long long s_keys[GF_LDS_KEYS];
  const int f = blockIdx.x;
  gf_select_frame(s_keys, keys + (size_t)f * pool, ncand[f], w, d2, suppress, cell, gw, gh, slots,
                  grid + (size_t)f * grid_stride, cap, 0, counts + f, corners + (size_t)f * cap);
}

// Rule F of rank 12: the frame's cap and output base are read from the device -- max_corners - carried[f] new
// corners behind the carried points (k_gftt_seeds has written those, and zeros with origin -1 behind them).
__global__ __launch_bounds__(GF_SELECT_THREADS) void k_gftt_select_topup(
    unsigned long long* __restrict__ keys, size_t pool, const int32_t* __restrict__ ncand, int w, float d2,
    int suppress, int cell, int gw, int gh, int slots, uint32_t* __restrict__ grid, size_t grid_stride,
    int slot_cap, const int32_t* __restrict__ carried, int32_t* __restrict__ counts, float2* __restrict__ points) {
  __shared__ unsigned long long s_keys[GF_LDS_KEYS];
  const int f = blockIdx.x;
  const int have = min(max(carried[f], 0), slot_cap);
  gf_select_frame(s_keys, keys + (size_t)f * pool, ncand[f], w, d2, suppress, cell, gw, gh, slots,
                  grid + (size_t)f * grid_stride, slot_cap - have, have, counts + f,
                  points + (size_t)f * slot_cap + have);
}

// ---- rank 12: masked detection that tops up tracked points (rules A-F) ----------------------
// The blocked pixels of a frame are ONE bit map (wp = ceil(w / 32) words per row, bit x & 31 of word x >> 5), built
// before the candidate pass from the carried seeds (k_gftt_block) or from a mask (k_gftt_mask_bits); the select walk
// never sees a seed, so the four-slots-per-cell bound above holds as it did.
#define GF_SEED_THREADS 256

// Rules A-B.  One workgroup per frame walks the seed slots in chunks of its size; the order is the slot order by
// ballot and prefix (block_scan_excl), never an atomic's.  Writes the carried points with their float bits, their
// slots to `origin`, carried[f], and behind the carried points zeros with origin -1 (rule F's tail; the select pass
// overwrites the slots of the new corners).  seed_xy == NULL: no seeds.
__global__ __launch_bounds__(GF_SEED_THREADS) void k_gftt_seeds(const float* __restrict__ seed_xy, size_t point_stride,
                                                                size_t frame_stride,
                                                                const int32_t* __restrict__ seed_seen, int seen_min,
                                                                int seed_cap, int w, int h, int slot_cap,
                                                                int32_t* __restrict__ carried,
                                                                float2* __restrict__ points,
                                                                int32_t* __restrict__ origin) {
  __shared__ int s_wave[GF_SEED_THREADS / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  float2* out = points + (size_t)f * slot_cap;
  int32_t* org = origin + (size_t)f * slot_cap;
  const float xmax = (float)(w - 1), ymax = (float)(h - 1);
  int base = 0;
  if (seed_xy != nullptr) {
    const float* sf = seed_xy + (size_t)f * frame_stride;
    for (int s0 = 0; s0 < seed_cap && base < slot_cap; s0 += GF_SEED_THREADS) {  // (base is uniform)
      const int s = s0 + tid;
      bool use = false;
      float x = 0.f, y = 0.f;
      if (s < seed_cap && (seed_seen == nullptr || seed_seen[(size_t)f * seed_cap + s] >= seen_min)) {
        x = sf[(size_t)s * point_stride];
        y = sf[(size_t)s * point_stride + 1];
        // (a NaN fails every compare; an infinity fails one of the bounds)
        use = x >= 0.f && x <= xmax && y >= 0.f && y <= ymax;
      }
      int total;
      const int at = base + block_scan_excl<GF_SEED_THREADS>(use ? 1 : 0, s_wave, &total);
      if (use && at < slot_cap) {
        out[at] = make_float2(x, y);
        org[at] = s;
      }
      base += total;
    }
  }
  const int have = min(base, slot_cap);
  for (int i = have + tid; i < slot_cap; i += GF_SEED_THREADS) {
    out[i] = make_float2(0.f, 0.f);
    org[i] = -1;
  }
  if (tid == 0) carried[f] = have;
}

// Rule C.  A lane takes one (carried seed, row of its box, word of that row): the box floor(s) - R .. floor(s) + 1 + R
// with R = ceil(min_distance), clipped to the frame, holds every pixel that can pass the rule (one beyond it is at
// least R + 1 > d away in one coordinate), and spans `wpr` words of a row at most.  The lane tests the pixels of its
// word and issues ONE atomicOr for them; OR commutes, the map does not depend on the order.
__global__ __launch_bounds__(256) void k_gftt_block(const float2* __restrict__ points, const int32_t* __restrict__ carried,
                                                    int slot_cap, int w, int h, int wp, int R, int wpr, float d2,
                                                    uint32_t* __restrict__ bits) {
  const int f = blockIdx.y;
  const int rows = 2 * R + 2;
  const long long per_seed = (long long)rows * wpr;
  const long long total = (long long)carried[f] * per_seed;
  const float2* pts = points + (size_t)f * slot_cap;
  uint32_t* bm = bits + (size_t)f * ((size_t)wp * h);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int seed = (int)(t / per_seed);
    const int rem = (int)(t - (long long)seed * per_seed);
    const int r = rem / wpr, wi = rem - r * wpr;
    const float2 s = pts[seed];  // usable: 0 <= s.x <= w - 1, 0 <= s.y <= h - 1
    const int fx = (int)floorf(s.x), fy = (int)floorf(s.y);
    const int y = fy - R + r;
    if (y < 0 || y >= h) continue;
    const int x0 = max(fx - R, 0), x1 = min(fx + 1 + R, w - 1);
    const int word = (x0 >> 5) + wi;
    if (word > (x1 >> 5)) continue;  // (x1 <= w - 1: word < wp)
    const int xa = max(x0, word << 5), xb = min(x1, (word << 5) + 31);
    const float dy = __fsub_rn((float)y, s.y);
    const float dy2 = __fmul_rn(dy, dy);
    uint32_t m = 0u;
    for (int X = xa; X <= xb; X++) {
      const float dx = __fsub_rn((float)X, s.x);
      if (__fadd_rn(__fmul_rn(dx, dx), dy2) < d2) m |= 1u << (X & 31);
    }
    if (m != 0u) atomicOr(&bm[(size_t)y * wp + word], m);
  }
}

// The mask entry: a pixel is blocked iff its mask byte is 0.  One lane per word of the map (every word is written).
__global__ __launch_bounds__(256) void k_gftt_mask_bits(const uint8_t* __restrict__ mask, int w, int h, int mask_stride,
                                                        int wp, uint32_t* __restrict__ bits) {
  const int word = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (word >= wp || y >= h) return;
  const uint8_t* row = mask + (size_t)y * mask_stride;
  const int xa = word << 5, xb = min(xa + 31, w - 1);
  uint32_t m = 0u;
  for (int X = xa; X <= xb; X++)
    if (row[X] == 0) m |= 1u << (X & 31);
  bits[(size_t)y * wp + word] = m;
}

// Rule D: the largest response among the pixels of the whole frame that are not blocked, reduced like
// k_gftt_response's (in-wave, then an atomicMax on the bit pattern of a non-negative float); mmax is zeroed by the
// host.  A wave takes 64 columns of GF_MAX_ROWS rows, a lane per pixel and row.  All waves of a frame meet in ONE
// word, so a wave first reads it (device scope; it only grows) and leaves out an atomic that could not raise it: a
// stale value costs an atomic, never the result.
#define GF_MAX_ROWS 16
__global__ __launch_bounds__(256) void k_gftt_masked_max(const float* __restrict__ map, int w, int h,
                                                         const uint32_t* __restrict__ bits, int wp,
                                                         uint32_t* __restrict__ mmax) {
  const int f = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 64 + lane;
  const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * GF_MAX_ROWS, y1 = min(y0 + GF_MAX_ROWS, h);
  float m = 0.f;
  if (x < w) {
    const uint32_t* b = bits + (size_t)f * ((size_t)wp * h) + (x >> 5);
    const float* e = map + (size_t)f * ((size_t)w * h) + x;
    for (int y = y0; y < y1; y++) {
      const float v = e[(size_t)y * w];
      if (!((b[(size_t)y * wp] >> (x & 31)) & 1u) && v > m) m = v;
    }
  }
  uint32_t mb = __float_as_uint(m);  // m >= 0
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) mb = max(mb, (uint32_t)__shfl_xor((int)mb, dlt, 64));
  if (lane == 0 && mb > __hip_atomic_load(&mmax[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&mmax[f], mb);
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

hipError_t orbx_launch_gftt_seeds(hipStream_t s, int n, const float* d_seed_xy, size_t point_stride,
                                  size_t frame_stride, const int32_t* d_seed_seen, int seen_min, int seed_cap, int w,
                                  int h, int slot_cap, int32_t* d_carried, float* d_points, int32_t* d_origin) {
  hipLaunchKernelGGL(k_gftt_seeds, dim3(n), dim3(GF_SEED_THREADS), 0, s, d_seed_xy, point_stride, frame_stride,
                     d_seed_seen, seen_min, seed_cap, w, h, slot_cap, d_carried, reinterpret_cast<float2*>(d_points),
                     d_origin);
  return hipGetLastError();
}

hipError_t orbx_launch_gftt_block(hipStream_t s, int n, const float* d_points, const int32_t* d_carried, int slot_cap,
                                  int max_seeds, int w, int h, double min_distance, uint32_t* d_bits) {
  const int R = (int)ceil(min_distance);
  const int wpr = (2 * R + 2 + 30) / 32 + 1;  // words a run of 2R + 2 pixels can touch
  const long long lanes = (long long)max_seeds * (2 * R + 2) * wpr;
  const unsigned blocks = (unsigned)std::min<long long>(std::max<long long>((lanes + 255) / 256, 1), 2048);
  hipLaunchKernelGGL(k_gftt_block, dim3(blocks, n), dim3(256), 0, s, reinterpret_cast<const float2*>(d_points),
                     d_carried, slot_cap, w, h, (w + 31) / 32, R, wpr, (float)(min_distance * min_distance), d_bits);
  return hipGetLastError();
}

hipError_t orbx_launch_gftt_mask_bits(hipStream_t s, const uint8_t* d_mask, int w, int h, int mask_stride,
                                      uint32_t* d_bits) {
  const int wp = (w + 31) / 32;
  hipLaunchKernelGGL(k_gftt_mask_bits, dim3((wp + 63) / 64, (h + 3) / 4), dim3(256), 0, s, d_mask, w, h, mask_stride,
                     wp, d_bits);
  return hipGetLastError();
}

hipError_t orbx_launch_gftt_masked_max(hipStream_t s, const float* d_map, int n, int w, int h, const uint32_t* d_bits,
                                       uint32_t* d_mmax) {
  const dim3 grid((w + 63) / 64, (h + 4 * GF_MAX_ROWS - 1) / (4 * GF_MAX_ROWS), n);
  hipLaunchKernelGGL(k_gftt_masked_max, grid, dim3(256), 0, s, d_map, w, h, d_bits, (w + 31) / 32, d_mmax);
  return hipGetLastError();
}

hipError_t orbx_launch_gftt_candidates_blocked(hipStream_t s, const float* d_map, int n, int w, int h,
                                               const uint32_t* d_mmax, double quality, unsigned long long* d_keys,
                                               size_t pool, int32_t* d_ncand, const uint32_t* d_bits) {
  const dim3 grid((w + 63) / 64, (h + 3) / 4, n);
  hipLaunchKernelGGL(k_gftt_candidates_blocked, grid, dim3(256), 0, s, d_map, w, h, d_mmax, quality, d_keys, pool,
                     d_ncand, d_bits, (w + 31) / 32);
  return hipGetLastError();
}

hipError_t orbx_launch_gftt_select_topup(hipStream_t s, int n, int w, unsigned long long* d_keys, size_t pool,
                                         const int32_t* d_ncand, double min_distance, int cell, int gw, int gh,
                                         int slots, uint32_t* d_grid, size_t grid_stride, int slot_cap,
                                         const int32_t* d_carried, int32_t* d_counts, float* d_points) {
  const float d2 = (float)(min_distance * min_distance);
  hipLaunchKernelGGL(k_gftt_select_topup, dim3(n), dim3(GF_SELECT_THREADS), 0, s, d_keys, pool, d_ncand, w, d2,
                     min_distance >= 1.0 ? 1 : 0, cell, gw, gh, slots, d_grid, grid_stride, slot_cap, d_carried,
                     d_counts, reinterpret_cast<float2*>(d_points));
  return hipGetLastError();
}
