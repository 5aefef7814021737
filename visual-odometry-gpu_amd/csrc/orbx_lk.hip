// orbx_lk.hip -- pyramidal Lucas-Kanade tracking for gfx950.
//
// Replaces cv::calcOpticalFlowPyrLK(img1, img2, pts1, pts2, status, err, Size(21,21), 3,
// TermCriteria(COUNT+EPS, 30, 0.01)) as called by src/feature_tracking.cpp:175-181.  The
// arithmetic follows OpenCV 4.x's published algorithm (lkpyramid.cpp: 14-bit fixed-point
// bilinear weights, 5 fractional bits on intensities, Scharr derivatives, minimum
// eigenvalue test, epsilon / oscillation stopping rules) with ONE documented difference:
// the window sums are accumulated exactly in integers (wave reduction of 16-bit halves)
// and rounded to float once, where OpenCV accumulates in float in a SIMD-width dependent
// order.  oracle/lk_oracle.c restates the same thing on the CPU; results are bit-identical.
//
// Kernels
//   k_lk_pyrdown  cv::pyrDown (5x5 [1 4 6 4 1]^2 / 256, REFLECT_101), thread per output pixel
//   k_lk_scharr   Scharr (3,10,3) derivative pairs as int16, REFLECT_101, thread per pixel
//                 (both take the frame in blockIdx.z: one launch per level for all frames of a slice)
//   k_lk_track    ONE WAVEFRONT PER POINT walks the levels top -> 0.  The 21x21 template
//                 (intensity + two gradients, int16) and a 26x26 neighbourhood of the next
//                 image live in the wave's LDS slice; every Newton step samples the 441
//                 window pixels from LDS (7 per lane) and reduces the two mismatch sums with
//                 DPP; the neighbourhood is re-fetched only when the window leaves it.  All
//                 control flow is wave-uniform, there is no workgroup barrier.
//   k_lk_track_windows  the same body (lk_track_point) in a loop over the frame pairs of a window: one wavefront
//                 per (window, point slot), the point handed from pair to pair in registers.
//   k_lk_track_windows_fb  that loop with the forward-backward check: every pair tracked forward and back again with
//                 the same body (the two frames swapped), the track ended by the first pair that does not return.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_internal.h"

namespace {

__device__ __forceinline__ int lk_reflect(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// blockIdx.z: the frame (source and destination `sframe` / `dframe` bytes apart; one frame: grid z = 1)
__global__ __launch_bounds__(256) void k_lk_pyrdown(const uint8_t* __restrict__ src, int sw, int sh, int spitch,
                                                    size_t sframe, uint8_t* __restrict__ dst, int dw, int dh,
                                                    int dpitch, size_t dframe) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  src += sframe * blockIdx.z;
  dst += dframe * blockIdx.z;
  int xs[5];
#pragma unroll
  for (int j = 0; j < 5; j++) xs[j] = lk_reflect(2 * x + j - 2, sw);
  int sum = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint8_t* row = src + (size_t)lk_reflect(2 * y + i - 2, sh) * spitch;
    const int hs = row[xs[0]] + 4 * row[xs[1]] + 6 * row[xs[2]] + 4 * row[xs[3]] + row[xs[4]];
    sum += (i == 0 || i == 4) ? hs : (i == 2 ? 6 * hs : 4 * hs);
  }
  dst[(size_t)y * dpitch + x] = (uint8_t)((sum + 128) >> 8);
}

// blockIdx.z: the frame (images `iframe` bytes, derivative maps `dframe` short2 apart)
__global__ __launch_bounds__(256) void k_lk_scharr(const uint8_t* __restrict__ img, int w, int h, int pitch,
                                                   size_t iframe, short2* __restrict__ deriv, size_t dframe) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  img += iframe * blockIdx.z;
  deriv += dframe * blockIdx.z;
  const uint8_t* r0 = img + (size_t)lk_reflect(y - 1, h) * pitch;
  const uint8_t* r1 = img + (size_t)y * pitch;
  const uint8_t* r2 = img + (size_t)lk_reflect(y + 1, h) * pitch;
  const int xl = lk_reflect(x - 1, w), xr = lk_reflect(x + 1, w);
  const int t0l = (r0[xl] + r2[xl]) * 3 + r1[xl] * 10, t0r = (r0[xr] + r2[xr]) * 3 + r1[xr] * 10;
  const int t1l = r2[xl] - r0[xl], t1c = r2[x] - r0[x], t1r = r2[xr] - r0[xr];
  deriv[(size_t)y * w + x] = make_short2((short)(t0r - t0l), (short)((t1r + t1l) * 3 + t1c * 10));
}

__device__ __forceinline__ int lk_wave_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1 /*quad_perm:[1,0,3,2]*/, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E /*quad_perm:[2,3,0,1]*/, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x141 /*row_half_mirror*/, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x140 /*row_mirror*/, 0xf, 0xf, true);
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
         __builtin_amdgcn_readlane(v, 48);
}

// exact sum over the wave of per-lane int32 partials, as the float the oracle gets from
// (float)(double)int64_sum: the 16-bit halves are reduced separately (no overflow), joined
// exactly in double, rounded once
__device__ __forceinline__ float lk_exact_sum_f32(int partial) {
  const int lo = lk_wave_sum(partial & 0xffff), hi = lk_wave_sum(partial >> 16);
  return (float)((double)hi * 65536.0 + (double)lo);
}

__device__ __forceinline__ int lk_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

struct LkWeights {
  int w00, w01, w10, w11;
};
__device__ __forceinline__ LkWeights lk_weights(float a, float b) {
  LkWeights r;
  const float s = (float)(1 << 14);
  r.w00 = (int)rintf(__fmul_rn(__fmul_rn(1.f - a, 1.f - b), s));
  r.w01 = (int)rintf(__fmul_rn(__fmul_rn(a, 1.f - b), s));
  r.w10 = (int)rintf(__fmul_rn(__fmul_rn(1.f - a, b), s));
  r.w11 = (1 << 14) - r.w00 - r.w01 - r.w10;
  return r;
}

// bilinear sample of an 8-bit level at (X, Y)..(X+1, Y+1), 5 fractional bits kept.
// interior: the four pixels are inside the image (wave-uniform fact about the whole window)
__device__ __forceinline__ int lk_sample(const OrbxLkLevel& L, int X, int Y, const LkWeights& w, bool interior) {
  int p00, p01, p10, p11;
  if (interior) {
    const uint8_t* p = L.img + (size_t)Y * L.pitch + X;
    p00 = p[0];
    p01 = p[1];
    p10 = p[L.pitch];
    p11 = p[L.pitch + 1];
  } else {
    const int x0 = lk_reflect(X, L.w), x1 = lk_reflect(X + 1, L.w);
    const uint8_t* r0 = L.img + (size_t)lk_reflect(Y, L.h) * L.pitch;
    const uint8_t* r1 = L.img + (size_t)lk_reflect(Y + 1, L.h) * L.pitch;
    p00 = r0[x0];
    p01 = r0[x1];
    p10 = r1[x0];
    p11 = r1[x1];
  }
  return lk_descale(p00 * w.w00 + p01 * w.w01 + p10 * w.w10 + p11 * w.w11, 14 - 5);
}

__device__ __forceinline__ short2 lk_deriv_at(const OrbxLkLevel& L, int X, int Y, bool interior) {
  if (!interior && (X < 0 || Y < 0 || X >= L.w || Y >= L.h)) return make_short2(0, 0);
  return reinterpret_cast<const short2*>(L.deriv)[(size_t)Y * L.w + X];
}

// The integer origin floor(v) of a window along an axis of `len` samples; false if the window is outside: v is NaN,
// floor(v) does not fit an int32, or floor(v) is not in [-win, len).  (The conversion alone would turn NaN into 0,
// an origin inside the image.)  Wave-uniform.
__device__ __forceinline__ bool lk_origin(float v, int win, int len, int& i) {
  const float f = floorf(v);
  i = (int)f;
  return f >= -2147483648.f && f < 2147483648.f && i >= -win && i < len;
}

#define LK_MAX_WIN 31
// one pass over the window items of a lane: unrolled when the trip count is a template constant
#define LK_ITEM_LOOP                                                                           \
  _Pragma("unroll 8") for (int it_ = 0, idx = lane; it_ < (NIT ? NIT : (nitem + 63) / 64); it_++, idx += 64) \
    if (idx < nitem)
// The Newton steps of a level move the window by fractions of a pixel, so its integer
// origin hardly ever changes: the (win + 1 + 2 * LK_JC_MARGIN)^2 neighbourhood of the next
// image is cached in LDS (border reflection resolved while loading) and re-fetched only when
// the window leaves it.  One global round trip per level instead of one per iteration.
#define LK_JC_MARGIN 2
#define LK_JC_MAX (LK_MAX_WIN + 1 + 2 * LK_JC_MARGIN)  // 36

__device__ __forceinline__ void lk_wave_lds_sync() {
  // LDS operations of one wave execute in order; this only pins the compiler
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct LkCache {
  uint8_t* px;  // jce x jce bytes
  int jce, x0, y0;
  uint32_t rcp;
  bool valid;
};

// makes sure the cache covers [inx, inx + win] x [iny, iny + win]
__device__ __forceinline__ void lk_cache_cover(LkCache& c, const OrbxLkLevel& J, int inx, int iny, int win, int lane) {
  if (c.valid && inx >= c.x0 && iny >= c.y0 && inx + win + 1 <= c.x0 + c.jce && iny + win + 1 <= c.y0 + c.jce) return;
  lk_wave_lds_sync();  // earlier reads of the old contents are done
  c.x0 = inx - LK_JC_MARGIN;
  c.y0 = iny - LK_JC_MARGIN;
  const bool interior = c.x0 >= 0 && c.y0 >= 0 && c.x0 + c.jce <= J.w && c.y0 + c.jce <= J.h;
  for (int idx = lane; idx < c.jce * c.jce; idx += 64) {
    const int y = (int)(((uint32_t)idx * c.rcp) >> 16), x = idx - y * c.jce;
    int v;
    if (interior)
      v = J.img[(size_t)(c.y0 + y) * J.pitch + (c.x0 + x)];
    else
      v = J.img[(size_t)lk_reflect(c.y0 + y, J.h) * J.pitch + lk_reflect(c.x0 + x, J.w)];
    c.px[idx] = (uint8_t)v;
  }
  c.valid = true;
  lk_wave_lds_sync();
}

// bilinear sample of the cached next image at window position (x, y) of origin (inx, iny)
__device__ __forceinline__ int lk_sample_cached(const LkCache& c, int inx, int iny, int x, int y, const LkWeights& w) {
  const uint8_t* p = c.px + (iny - c.y0 + y) * c.jce + (inx - c.x0 + x);
  return lk_descale(p[0] * w.w00 + p[1] * w.w01 + p[c.jce] * w.w10 + p[c.jce + 1] * w.w11, 14 - 5);
}

// What a wave needs besides its point: its LDS slice and the window constants (all wave-uniform)
struct LkWave {
  short4* tpl;  // the template, (intensity, dx, dy) as int16 (4th lane of the short4 unused)
  LkCache jc;
  int lane, win, nitem, max_iters;
  uint32_t rcp;  // idx / win == (idx * rcp) >> 16 for idx < 961
  float half, flt_scale;
  double eps2;
};

__device__ __forceinline__ LkWave lk_wave_setup(short4* tpl, uint8_t* jc_px, int lane, int win, int max_iters,
                                                double eps2) {
  LkWave W;
  W.tpl = tpl;
  W.jc.px = jc_px;
  W.jc.jce = win + 1 + 2 * LK_JC_MARGIN;
  W.jc.rcp = (65536u + (uint32_t)W.jc.jce - 1u) / (uint32_t)W.jc.jce;  // idx / jce for idx < 36^2
  W.jc.x0 = W.jc.y0 = 0;
  W.jc.valid = false;
  W.lane = lane;
  W.win = win;
  W.nitem = win * win;
  W.max_iters = max_iters;
  W.rcp = (65536u + (uint32_t)win - 1u) / (uint32_t)win;
  W.half = (float)(win - 1) * 0.5f;
  W.flt_scale = 1.f / (float)(1 << 20);
  W.eps2 = eps2;
  return W;
}

// The pyramids of one image pair as the kernels hand them to the body: level(l) is wave-uniform
struct LkPyrArg {  // k_lk_track: the kernel argument as it is
  const OrbxLkPyr& P;
  __device__ __forceinline__ OrbxLkLevel level(int l) const { return P.L[l]; }
};
struct LkPyrFrame {  // k_lk_track_windows: frame f of the slice
  const OrbxLkFrames& F;
  int f;
  __device__ __forceinline__ OrbxLkLevel level(int l) const {
    OrbxLkLevel L = F.L[l];
    L.img += l == 0 ? F.frame_stride * (size_t)f : F.img_stride * (size_t)(f - F.first);
    L.deriv += F.der_stride * (size_t)(f - F.first);
    return L;
  }
};

// ONE text of the tracker's arithmetic: the point pp of image P followed into image N, from the top level down to
// the error value.  Used by k_lk_track (one pair) and by k_lk_track_windows (the pairs of a window, one after the
// other).  NIT: passes of the 64 lanes over the win x win window, known at compile time for the reference's
// 21 x 21 window (7: the loops unroll and the LDS / global reads of a pass set are all in flight together),
// 0 = run-time trip count for any other window size.  Everything but `lane` is wave-uniform.
template <int NIT, class Pyr>
__device__ __forceinline__ void lk_track_point(const Pyr& P, const Pyr& N, int top, float2 pp, LkWave& W, float& outx,
                                               float& outy, int& st, float& ev) {
  short4* tpl = W.tpl;
  LkCache& jc = W.jc;
  const int lane = W.lane, win = W.win, nitem = W.nitem, max_iters = W.max_iters;
  const uint32_t rcp = W.rcp;
  const float half = W.half, flt_scale = W.flt_scale;
  const double eps2 = W.eps2;
  st = 1;
  ev = 0.f;
  outx = 0.f;
  outy = 0.f;
  for (int level = top; level >= 0; level--) {
    const OrbxLkLevel I = P.level(level), J = N.level(level);
    jc.valid = false;
    const float sc = (float)(1.0 / (double)(1 << level));
    float px = __fmul_rn(pp.x, sc), py = __fmul_rn(pp.y, sc);
    float nx, ny;
    if (level == top) {
      nx = px;
      ny = py;
    } else {
      nx = __fmul_rn(outx, 2.f);
      ny = __fmul_rn(outy, 2.f);
    }
    outx = nx;
    outy = ny;
    px -= half;
    py -= half;
    int ipx, ipy;
    if (!lk_origin(px, win, I.w, ipx) || !lk_origin(py, win, I.h, ipy)) {
      if (level == 0) {
        st = 0;
        ev = 0.f;
      }
      continue;
    }
    // template + gradient matrix
    const LkWeights wi = lk_weights(px - (float)ipx, py - (float)ipy);
    const bool in_i = ipx >= 0 && ipy >= 0 && ipx + win + 1 <= I.w && ipy + win + 1 <= I.h;
    int a11 = 0, a12 = 0, a22 = 0;
    LK_ITEM_LOOP {
      const int y = (int)(((uint32_t)idx * rcp) >> 16), x = idx - y * win;
      const int X = ipx + x, Y = ipy + y;
      const int iv = lk_sample(I, X, Y, wi, in_i);
      const short2 d00 = lk_deriv_at(I, X, Y, in_i), d01 = lk_deriv_at(I, X + 1, Y, in_i);
      const short2 d10 = lk_deriv_at(I, X, Y + 1, in_i), d11 = lk_deriv_at(I, X + 1, Y + 1, in_i);
      const int ix = lk_descale(d00.x * wi.w00 + d01.x * wi.w01 + d10.x * wi.w10 + d11.x * wi.w11, 14);
      const int iy = lk_descale(d00.y * wi.w00 + d01.y * wi.w01 + d10.y * wi.w10 + d11.y * wi.w11, 14);
      tpl[idx] = make_short4((short)iv, (short)ix, (short)iy, 0);
      a11 += ix * ix;
      a12 += ix * iy;
      a22 += iy * iy;
    }
    const float A11 = __fmul_rn(lk_exact_sum_f32(a11), flt_scale), A12 = __fmul_rn(lk_exact_sum_f32(a12), flt_scale),
                A22 = __fmul_rn(lk_exact_sum_f32(a22), flt_scale);
    float D = __fsub_rn(__fmul_rn(A11, A22), __fmul_rn(A12, A12));
    const float dif = __fsub_rn(A11, A22);
    const float disc = __fadd_rn(__fmul_rn(dif, dif), __fmul_rn(__fmul_rn(4.f, A12), A12));
    const float min_eig = __fdiv_rn(__fsub_rn(__fadd_rn(A22, A11), sqrtf(disc)), (float)(2 * win * win));
    if (min_eig < 1e-4f || D < 1.1920928955078125e-07f) {
      if (level == 0) st = 0;
      continue;
    }
    D = __fdiv_rn(1.f, D);
    nx -= half;
    ny -= half;
    float pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < max_iters; j++) {
      int inx, iny;
      if (!lk_origin(nx, win, J.w, inx) || !lk_origin(ny, win, J.h, iny)) {
        if (level == 0) st = 0;
        break;
      }
      const LkWeights wj = lk_weights(nx - (float)inx, ny - (float)iny);
      lk_cache_cover(jc, J, inx, iny, win, lane);
      int b1 = 0, b2 = 0;
      LK_ITEM_LOOP {
        const int y = (int)(((uint32_t)idx * rcp) >> 16), x = idx - y * win;
        const short4 t = tpl[idx];
        const int diff = lk_sample_cached(jc, inx, iny, x, y, wj) - t.x;
        b1 += diff * t.y;
        b2 += diff * t.z;
      }
      const float B1 = __fmul_rn(lk_exact_sum_f32(b1), flt_scale), B2 = __fmul_rn(lk_exact_sum_f32(b2), flt_scale);
      const float dx = __fmul_rn(__fsub_rn(__fmul_rn(A12, B2), __fmul_rn(A22, B1)), D);
      const float dy = __fmul_rn(__fsub_rn(__fmul_rn(A12, B1), __fmul_rn(A11, B2)), D);
      nx = __fadd_rn(nx, dx);
      ny = __fadd_rn(ny, dy);
      outx = __fadd_rn(nx, half);
      outy = __fadd_rn(ny, half);
      if (__dadd_rn(__dmul_rn((double)dx, (double)dx), __dmul_rn((double)dy, (double)dy)) <= eps2) break;
      if (j > 0 && (double)fabsf(__fadd_rn(dx, pdx)) < 0.01 && (double)fabsf(__fadd_rn(dy, pdy)) < 0.01) {
        outx = __fsub_rn(outx, __fmul_rn(dx, 0.5f));
        outy = __fsub_rn(outy, __fmul_rn(dy, 0.5f));
        break;
      }
      pdx = dx;
      pdy = dy;
    }
    if (st && level == 0) {
      const float ex = __fsub_rn(outx, half), ey = __fsub_rn(outy, half);
      int inx, iny;
      if (!lk_origin(ex, win, J.w, inx) || !lk_origin(ey, win, J.h, iny)) {
        st = 0;
        continue;
      }
      const LkWeights wj = lk_weights(ex - (float)inx, ey - (float)iny);
      lk_cache_cover(jc, J, inx, iny, win, lane);
      int e = 0;
      LK_ITEM_LOOP {
        const int y = (int)(((uint32_t)idx * rcp) >> 16), x = idx - y * win;
        const int diff = lk_sample_cached(jc, inx, iny, x, y, wj) - tpl[idx].x;
        e += diff < 0 ? -diff : diff;
      }
      ev = __fmul_rn(lk_exact_sum_f32(e), __fdiv_rn(1.f, (float)(32 * win * win)));
    }
  }
}

template <int NIT>
__global__ __launch_bounds__(256) void k_lk_track(OrbxLkPyr P, OrbxLkPyr N, int n, const float2* __restrict__ prev_pts,
                                                  float2* __restrict__ next_pts, uint8_t* __restrict__ status,
                                                  float* __restrict__ err, int win, int max_iters, double eps2) {
  __shared__ short4 s_tpl[4][LK_MAX_WIN * LK_MAX_WIN];
  __shared__ uint8_t s_jc[4][LK_JC_MAX * LK_JC_MAX];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;  // whole wave
  LkWave W = lk_wave_setup(s_tpl[wave], s_jc[wave], lane, win, max_iters, eps2);
  // the point is the same in every lane: keep it (and everything derived from it) wave-uniform
  float2 pp = prev_pts[i];
  pp.x = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pp.x)));
  pp.y = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pp.y)));
  int st;
  float ev, outx, outy;
  lk_track_point<NIT>(LkPyrArg{P}, LkPyrArg{N}, P.top, pp, W, outx, outy, st, ev);
  if (lane == 0) {
    next_pts[i] = make_float2(outx, outy);
    status[i] = (uint8_t)st;
    if (err) err[i] = ev;
  }
}

// trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499) for every (window, point slot) of a slice: ONE
// WAVEFRONT per slot follows its point through the pairs (f0, f0 + 1), (f0 + 1, f0 + 2), ... of its window; the point
// that leaves a pair enters the next one from registers, and the wave stops at the first pair that loses it.
// Outputs (lane 0, plain stores): tracks[window][slot][k] = the point in frame f0 + k (k = 0: the input point),
// seen[window][slot] = frames the point was observed in, err[window][slot][k - 1] = the pair's error; everything past
// `seen`, and every slot at or beyond counts[window], is written as 0.  grid (ceil(cap / 4), windows of the slice).
template <int NIT>
__global__ __launch_bounds__(256) void k_lk_track_windows(OrbxLkFrames F, const int32_t* __restrict__ window_first,
                                                          int window_len, const float2* __restrict__ points,
                                                          const int32_t* __restrict__ counts, int cap,
                                                          float2* __restrict__ tracks, int32_t* __restrict__ seen,
                                                          float* __restrict__ err, int win, int max_iters,
                                                          double eps2) {
  __shared__ short4 s_tpl[4][LK_MAX_WIN * LK_MAX_WIN];
  __shared__ uint8_t s_jc[4][LK_JC_MAX * LK_JC_MAX];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + wave, w = blockIdx.y;
  if (slot >= cap) return;  // whole wave
  const size_t at = (size_t)w * cap + slot;
  float2* trk = tracks + at * window_len;
  float* er = err + at * (window_len - 1);
  int count = counts ? counts[w] : cap;
  count = __builtin_amdgcn_readfirstlane(count < cap ? count : cap);
  int k = 0;  // frames the point has been observed in
  if (slot < count) {
    const int f0 = __builtin_amdgcn_readfirstlane(window_first[w]);
    LkWave W = lk_wave_setup(s_tpl[wave], s_jc[wave], lane, win, max_iters, eps2);
    float2 pp = points[at];
    pp.x = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pp.x)));
    pp.y = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pp.y)));
    if (lane == 0) trk[0] = pp;
    for (k = 1; k < window_len; k++) {
      int st;
      float ev, outx, outy;
      lk_track_point<NIT>(LkPyrFrame{F, f0 + k - 1}, LkPyrFrame{F, f0 + k}, F.top, pp, W, outx, outy, st, ev);
      if (!st) break;
      pp = make_float2(outx, outy);
      if (lane == 0) {
        trk[k] = pp;
        er[k - 1] = ev;
      }
    }
  }
  // the zero tail: frames k .. window_len - 1 and their pairs, a lane each
  for (int j = k + lane; j < window_len; j += 64) {
    trk[j] = make_float2(0.f, 0.f);
    if (j > 0) er[j - 1] = 0.f;
  }
  if (lane == 0) seen[at] = k;
}

// k_lk_track_windows with the forward-backward check: the same grid, wave setup and LDS
// slices.  Every pair is tracked twice with the one body: p of frame k - 1 forward into frame k (q), then q of
// frame k back into frame k - 1 (r, from q itself: no initial flow).  The pair passes iff both passes keep the point
// and |r - p|^2 <= thr2 in binary64 (the products exact, the sum rounded once; NaN fails); the first pair that does
// not pass ends the track.  Beside the outputs of k_lk_track_windows: fb_d2[window][slot][k - 1] = (float)|r - p|^2
// of every pair that passed, 0 elsewhere; lost[window][slot] = why the track ended, 1 forward pass, 2 backward pass,
// 3 distance, 0 for a track alive through the window and for the slots at or beyond counts[window].
template <int NIT>
__global__ __launch_bounds__(256) void k_lk_track_windows_fb(OrbxLkFrames F, const int32_t* __restrict__ window_first,
                                                             int window_len, const float2* __restrict__ points,
                                                             const int32_t* __restrict__ counts, int cap,
                                                             float2* __restrict__ tracks, int32_t* __restrict__ seen,
                                                             float* __restrict__ err, float* __restrict__ fb_d2,
                                                             int32_t* __restrict__ lost, int win, int max_iters,
                                                             double eps2, double thr2) {
  __shared__ short4 s_tpl[4][LK_MAX_WIN * LK_MAX_WIN];
  __shared__ uint8_t s_jc[4][LK_JC_MAX * LK_JC_MAX];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + wave, w = blockIdx.y;
  if (slot >= cap) return;  // whole wave
  const size_t at = (size_t)w * cap + slot;
  float2* trk = tracks + at * window_len;
  float* er = err + at * (window_len - 1);
  float* fb = fb_d2 + at * (window_len - 1);
  int count = counts ? counts[w] : cap;
  count = __builtin_amdgcn_readfirstlane(count < cap ? count : cap);
  int k = 0;       // frames the point has been observed in
  int reason = 0;  // why the track ended
  if (slot < count) {
    const int f0 = __builtin_amdgcn_readfirstlane(window_first[w]);
    LkWave W = lk_wave_setup(s_tpl[wave], s_jc[wave], lane, win, max_iters, eps2);
    float2 pp = points[at];
    pp.x = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pp.x)));
    pp.y = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(pp.y)));
    if (lane == 0) trk[0] = pp;
    for (k = 1; k < window_len; k++) {
      int st;
      float ev, qx, qy, rx, ry, eb;
      lk_track_point<NIT>(LkPyrFrame{F, f0 + k - 1}, LkPyrFrame{F, f0 + k}, F.top, pp, W, qx, qy, st, ev);
      if (!st) {
        reason = 1;
        break;
      }
      lk_track_point<NIT>(LkPyrFrame{F, f0 + k}, LkPyrFrame{F, f0 + k - 1}, F.top, make_float2(qx, qy), W, rx, ry, st,
                          eb);
      if (!st) {
        reason = 2;
        break;
      }
      const float dx = __fsub_rn(rx, pp.x), dy = __fsub_rn(ry, pp.y);
      const double d2 = __dadd_rn(__dmul_rn((double)dx, (double)dx), __dmul_rn((double)dy, (double)dy));
      if (!(d2 <= thr2)) {  // (NaN fails)
        reason = 3;
        break;
      }
      pp = make_float2(qx, qy);
      if (lane == 0) {
        trk[k] = pp;
        er[k - 1] = ev;
        fb[k - 1] = (float)d2;
      }
    }
  }
  // the zero tail: frames k .. window_len - 1 and their pairs, a lane each
  for (int j = k + lane; j < window_len; j += 64) {
    trk[j] = make_float2(0.f, 0.f);
    if (j > 0) {
      er[j - 1] = 0.f;
      fb[j - 1] = 0.f;
    }
  }
  if (lane == 0) {
    seen[at] = k;
    lost[at] = reason;
  }
}

}  // namespace

hipError_t orbx_launch_lk_pyrdown(hipStream_t s, const uint8_t* d_src, int sw, int sh, int spitch, uint8_t* d_dst,
                                  int dw, int dh, int dpitch) {
  return orbx_launch_lk_pyrdown_frames(s, 1, d_src, sw, sh, spitch, 0, d_dst, dw, dh, dpitch, 0);
}

hipError_t orbx_launch_lk_pyrdown_frames(hipStream_t s, int frames, const uint8_t* d_src, int sw, int sh, int spitch,
                                         size_t src_frame_stride, uint8_t* d_dst, int dw, int dh, int dpitch,
                                         size_t dst_frame_stride) {
  if (frames < 1 || frames > 65535) return hipErrorInvalidValue;
  dim3 grid((dw + 63) / 64, (dh + 3) / 4, frames);
  hipLaunchKernelGGL(k_lk_pyrdown, grid, dim3(256), 0, s, d_src, sw, sh, spitch, src_frame_stride, d_dst, dw, dh,
                     dpitch, dst_frame_stride);
  return hipGetLastError();
}

hipError_t orbx_launch_lk_scharr(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch, int16_t* d_deriv) {
  return orbx_launch_lk_scharr_frames(s, 1, d_img, w, h, pitch, 0, d_deriv, 0);
}

hipError_t orbx_launch_lk_scharr_frames(hipStream_t s, int frames, const uint8_t* d_img, int w, int h, int pitch,
                                        size_t img_frame_stride, int16_t* d_deriv, size_t deriv_frame_bytes) {
  if (frames < 1 || frames > 65535 || (deriv_frame_bytes & 3)) return hipErrorInvalidValue;
  dim3 grid((w + 63) / 64, (h + 3) / 4, frames);
  hipLaunchKernelGGL(k_lk_scharr, grid, dim3(256), 0, s, d_img, w, h, pitch, img_frame_stride,
                     reinterpret_cast<short2*>(d_deriv), deriv_frame_bytes / 4);
  return hipGetLastError();
}

hipError_t orbx_launch_lk_track(hipStream_t s, const OrbxLkPyr& prev, const OrbxLkPyr& next, int n,
                                const float* d_prev_pts, float* d_next_pts, uint8_t* d_status, float* d_err, int win,
                                int max_iters, double eps2) {
  if (n <= 0) return hipSuccess;
  if (win < 3 || win > LK_MAX_WIN) return hipErrorInvalidValue;
  const float2* pp = reinterpret_cast<const float2*>(d_prev_pts);
  float2* np_ = reinterpret_cast<float2*>(d_next_pts);
  if (win == 21)
    hipLaunchKernelGGL(k_lk_track<7>, dim3((n + 3) / 4), dim3(256), 0, s, prev, next, n, pp, np_, d_status, d_err, win,
                       max_iters, eps2);
  else
    hipLaunchKernelGGL(k_lk_track<0>, dim3((n + 3) / 4), dim3(256), 0, s, prev, next, n, pp, np_, d_status, d_err, win,
                       max_iters, eps2);
  return hipGetLastError();
}

hipError_t orbx_launch_lk_track_windows(hipStream_t s, const OrbxLkFrames& frames, const int32_t* d_window_first,
                                        int n_windows, int window_len, const float* d_points, const int32_t* d_counts,
                                        int slot_capacity, float* d_tracks, int32_t* d_seen, float* d_err, int win,
                                        int max_iters, double eps2) {
  if (n_windows < 1 || n_windows > 65535 || window_len < 2 || slot_capacity < 1) return hipErrorInvalidValue;
  if (win < 3 || win > LK_MAX_WIN) return hipErrorInvalidValue;
  const dim3 grid((slot_capacity + 3) / 4, n_windows);
  const float2* pts = reinterpret_cast<const float2*>(d_points);
  float2* trk = reinterpret_cast<float2*>(d_tracks);
  if (win == 21)
    hipLaunchKernelGGL(k_lk_track_windows<7>, grid, dim3(256), 0, s, frames, d_window_first, window_len, pts, d_counts,
                       slot_capacity, trk, d_seen, d_err, win, max_iters, eps2);
  else
    hipLaunchKernelGGL(k_lk_track_windows<0>, grid, dim3(256), 0, s, frames, d_window_first, window_len, pts, d_counts,
                       slot_capacity, trk, d_seen, d_err, win, max_iters, eps2);
  return hipGetLastError();
}

hipError_t orbx_launch_lk_track_windows_fb(hipStream_t s, const OrbxLkFrames& frames, const int32_t* d_window_first,
                                           int n_windows, int window_len, const float* d_points,
                                           const int32_t* d_counts, int slot_capacity, float* d_tracks, int32_t* d_seen,
                                           float* d_err, float* d_fb_d2, int32_t* d_lost, int win, int max_iters,
                                           double eps2, double thr2) {
  if (n_windows < 1 || n_windows > 65535 || window_len < 2 || slot_capacity < 1) return hipErrorInvalidValue;
  if (win < 3 || win > LK_MAX_WIN || !(thr2 >= 0.0)) return hipErrorInvalidValue;
  const dim3 grid((slot_capacity + 3) / 4, n_windows);
  const float2* pts = reinterpret_cast<const float2*>(d_points);
  float2* trk = reinterpret_cast<float2*>(d_tracks);
  if (win == 21)
    hipLaunchKernelGGL(k_lk_track_windows_fb<7>, grid, dim3(256), 0, s, frames, d_window_first, window_len, pts,
                       d_counts, slot_capacity, trk, d_seen, d_err, d_fb_d2, d_lost, win, max_iters, eps2, thr2);
  else
    hipLaunchKernelGGL(k_lk_track_windows_fb<0>, grid, dim3(256), 0, s, frames, d_window_first, window_len, pts,
                       d_counts, slot_capacity, trk, d_seen, d_err, d_fb_d2, d_lost, win, max_iters, eps2, thr2);
  return hipGetLastError();
}
