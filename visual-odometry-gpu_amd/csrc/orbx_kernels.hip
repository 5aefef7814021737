// orbx_kernels.hip -- hand-written gfx950 (CDNA4) kernels of the ORB front-end.
//
// Design notes (see DESIGN.md §6 for the full picture and the measurements):
//  * 64-lane wavefronts everywhere.  Cross-lane work uses DPP (wave_shr/shl for
//    the blur's left/right neighbours, row scans and reductions, the Harris sum
//    hand-off) and 64-bit ballots (4 ballots == one 256-bit BRIEF descriptor).
//  * Pixels are processed 4 per lane as aligned dwords; the 8-bit stencil math
//    runs on packed 16-bit lanes (v_perm_b32 + v_pk_*_u16).  No MFMA: nothing
//    here is a dense contraction.  Every kernel turned out to be bound by VALU
//    issue (one wave64 instruction per SIMD per 4 clocks), so the designs
//    minimise instructions per pixel first, memory traffic second.
//  * Row-coalesced aligned loads: straight into registers where a stencil can
//    stream (blur, pyramid), into an LDS tile with halo where it needs random
//    access (FAST ring gathers, BRIEF patches).
//  * All levels of all frames of a batch are covered by ONE launch per stage;
//    each workgroup reads its tile from a 64-byte OrbxTileDesc record.
//  * Keypoint order is deterministic (row-major), never atomics-ordered.
//  * Integer arithmetic wherever the reference's float arithmetic is exact, so
//    results are bit-identical to the CPU oracle; the float parts (angles,
//    rotation, Harris) use orbx_math.h and -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "orbx_internal.h"
#include "orbx_math.h"
#include "orbx_wave.h"

__constant__ __attribute__((aligned(16))) int8_t c_pattern[1024] = {
#include "pattern_31.inc"
};

// ---------------------------------------------------------------------------
// helpers

typedef uint16_t __attribute__((aligned(1))) u16_unaligned;

// (level, tile_x, tile_y) of this workgroup
__device__ __forceinline__ void decode_tile(const OrbxTileMap& tm, int nlevels, int& l, int& tx, int& ty) {
  const int t = blockIdx.x;
  l = 0;
#pragma unroll 1
  for (int i = 1; i < nlevels; i++)
    if (t >= tm.begin[i]) l = i;
  const int local = t - tm.begin[l];
  ty = local / tm.tiles_x[l];
  tx = local - ty * tm.tiles_x[l];
}

// BORDER_REFLECT_101 for p in [-len+1, 2*len-2], clamped otherwise
// (src/cuda/GaussianBlur1D.cu:27-32)
__device__ __forceinline__ int reflect101(int p, int len) {
  if (p < 0) p = -p;
  if (p >= len) p = 2 * len - p - 2;
  p = p < 0 ? 0 : p;
  return p >= len ? len - 1 : p;
}

// ---------------------------------------------------------------------------
// 1. pyramid: level 0 copy + fixed-point bilinear resize of every level >= 1
//    straight from level 0 (src/orb.cpp:111-120).  (A first version with one
//    thread per 4 pixels was latency-bound: 416k short waves, each with two
//    dependent memory round trips, tap table -> pixel gathers; 206 us per batch.)
//    Here a wave owns 256 x 4 output pixels: the row index
//     is wave-uniform, so the y tap and the two source-row bases are scalar
//     loads / SGPR addresses; the four x taps of a lane are loaded once and
//     reused for four rows; all 32 pixel-pair gathers of a lane are issued
//     before the first is consumed.
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
struct __attribute__((packed, aligned(1))) uint2_unaligned {
  uint32_t x, y;
  __device__ operator uint2() const { return make_uint2(x, y); }
};

// ROWS output rows of a lane's four pixels.  WIN8: levels with scale <= 2, where the four
// source pairs of a lane lie inside one 8-byte window (host-verified per level), so ONE
// unaligned 8-byte load per source row replaces four 2-byte gathers and v_perm picks each pair
// out of it (only 4 registers per output row are in flight, which is what lets a wave own 8
// rows); else four 2-byte pair gathers per source row.
template <int ROWS, bool WIN8>
__device__ __forceinline__ void pyr_rows(const uint8_t* __restrict__ src, int in_stride, int w0, int h0,
                                         const OrbxResizeTap* __restrict__ ytaps, int yb, int lh,
                                         const uint32_t (&ofs)[4], const uint32_t (&cc)[4],
                                         __amdgpu_buffer_rsrc_t rout, uint32_t voff_st, uint32_t vmask, int pitch) {
  constexpr int NW = WIN8 ? 2 : 4;  // dwords in flight per source row
  uint32_t q0[ROWS][NW], q1[ROWS][NW];
  int b0[ROWS], b1[ROWS];
  uint32_t sel[4];
  uint32_t base = 0;
  if (WIN8) {
    // the window start is clamped so that it never reads past the source row
    base = min(ofs[0], (uint32_t)(w0 - 8));
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t sb = ofs[k] - base;               // 0..6
      sel[k] = 0x0c000c00u | ((sb + 1) << 16) | sb;  // (src[ofs], src[ofs+1]) as two u16 lanes
    }
  }
  // every gather of the wave is in flight before the first is used
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const int y = min(yb + r, lh - 1);         // rows past the level repeat the last one (not stored)
    const OrbxResizeTap ty_ = ytaps[y];        // wave-uniform -> scalar load
    const int sy0 = min(max(ty_.ofs, 0), h0 - 1), sy1 = min(max(ty_.ofs + 1, 0), h0 - 1);
    const uint8_t* S0 = src + (size_t)sy0 * in_stride;
    const uint8_t* S1 = src + (size_t)sy1 * in_stride;
    b0[r] = ty_.c0;
    b1[r] = ty_.c1;
    if (WIN8) {
      const uint2 a = *reinterpret_cast<const uint2_unaligned*>(S0 + base);
      const uint2 b = *reinterpret_cast<const uint2_unaligned*>(S1 + base);
      q0[r][0] = a.x;
      q0[r][1] = a.y;
      q1[r][0] = b.x;
      q1[r][1] = b.y;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        // ofs <= w0-2 always (host table): one unaligned 16-bit load fetches src[ofs], src[ofs+1]
        q0[r][k] = *reinterpret_cast<const u16_unaligned*>(S0 + ofs[k]);
        q1[r][k] = *reinterpret_cast<const u16_unaligned*>(S1 + ofs[k]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    uint32_t out = 0;
    const uint32_t bs0 = ((uint32_t)b0[r] << 12) & 0xffffffu, bs1 = ((uint32_t)b1[r] << 12) & 0xffffffu;  // b <= 2048
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t p0, p1;  // the pixel pair as two u16 lanes
      if (WIN8) {
        p0 = __builtin_amdgcn_perm(q0[r][1], q0[r][0], sel[k]);
        p1 = __builtin_amdgcn_perm(q1[r][1], q1[r][0], sel[k]);
      } else {
        p0 = __builtin_amdgcn_perm(q0[r][k], q0[r][k], 0x0c010c00u);
        p1 = __builtin_amdgcn_perm(q1[r][k], q1[r][k], 0x0c010c00u);
      }
      // horizontal pass: src[ofs] * c0 + src[ofs+1] * c1 is one v_dot2_u32_u16 of the pixel
      // pair with the tap's packed (c0, c1)
      const us2_t cw = __builtin_bit_cast(us2_t, cc[k]);
      const uint32_t r0 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, p0), cw, 0u, false);
      const uint32_t r1 = __builtin_amdgcn_udot2(__builtin_bit_cast(us2_t, p1), cw, 0u, false);
      // vertical pass: (b * (r >> 4)) >> 16 == ((r & ~15) * (b << 12)) >> 32 with both factors
      // below 2^24: one v_and + one full-rate v_mul_hi_u32_u24 per term; the sum is <= 1022
      const uint32_t t0 = (uint32_t)(((u64)(r0 & 0xfffff0u) * (u64)bs0) >> 32);
      const uint32_t t1 = (uint32_t)(((u64)(r1 & 0xfffff0u) * (u64)bs1) >> 32);
      out |= ((t0 + t1 + 2u) >> 2) << (8 * k);
    }
    const int y = yb + r;
    if (y < lh) __builtin_amdgcn_raw_buffer_store_b32(out & vmask, rout, voff_st, y * pitch, 0);
  }
}

__global__ __launch_bounds__(256) void k_pyramid2(const OrbxTileDesc* __restrict__ tiles, int n_tiles, int frame_bytes, int w0,
                                                  int h0, const uint8_t* __restrict__ in, int in_stride,
                                                  size_t in_frame_stride, const OrbxResizeTap* __restrict__ taps,
                                                  uint8_t* __restrict__ pyr) {
  if ((int)blockIdx.x >= n_tiles) return;  // (grid.x is padded to an odd number: orbx_launch_pyramid2)
  const OrbxTileDesc d = tiles[blockIdx.x];  // one scalar load instead of decoding through the plan
  struct {
    int w, h, pitch, xtab_off, ytab_off, win8;
  } L = {d.w, d.h, d.pitch, d.u0, d.u1, d.u2};
  const int l = d.l, tx = d.tx, ty = d.ty;
  const int rpw = d.f;  // rows per wave of this level's tiles: 8 (level 0, 8-byte-window levels) or 4
  const int f = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint8_t* src = in + (size_t)f * in_frame_stride;
  const int x = tx * 256 + lane * 4;
  const int yb = (ty * 4 + wave) * rpw;
  if (yb >= L.h) return;  // whole wave
  const int pitch = L.pitch, w = L.w;
  const __amdgpu_buffer_rsrc_t rout =
      __builtin_amdgcn_make_buffer_rsrc(pyr + (size_t)f * frame_bytes + d.img_off, 0, pitch * L.h, 0x00020000);
  const uint32_t voff_st = x < pitch ? (uint32_t)x : 0xffffffffu;
  const int nvalid = w - x;
  const uint32_t vmask = nvalid >= 4 ? 0xffffffffu : nvalid <= 0 ? 0u : ((1u << (8 * nvalid)) - 1u);

  if (l == 0) {  // level 0 = the input frame (src/orb.cpp:112), re-pitched
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int y = yb + r;
      if (r < rpw && y < L.h) {
        const uint8_t* row = src + (size_t)y * in_stride;
        uint32_t v = 0;
        if (nvalid >= 4 || (nvalid > 0 && y + 1 < L.h)) {
          // (a partial last dword of a row above the last one runs into the next row of the
          // same frame: readable, and vmask drops those bytes)
          v = *reinterpret_cast<const u32_unaligned*>(row + x);
        } else if (nvalid > 0) {  // last dword of the last row: never read past the frame
          for (int k = 0; k < nvalid; k++) v |= (uint32_t)row[x + k] << (8 * k);
        }
        __builtin_amdgcn_raw_buffer_store_b32(v & vmask, rout, voff_st, y * pitch, 0);
      }
    }
    return;
  }

  // x taps of this lane's four pixels (zero taps for lanes right of the image)
  uint32_t ofs[4] = {0, 0, 0, 0}, cc[4] = {0, 0, 0, 0};
  if (nvalid > 0) {
    const uint4* tp = reinterpret_cast<const uint4*>(taps + L.xtab_off + x);
    const uint4 t01 = tp[0], t23 = tp[1];
    ofs[0] = t01.x; ofs[1] = t01.z; ofs[2] = t23.x; ofs[3] = t23.z;
    cc[0] = t01.y; cc[1] = t01.w; cc[2] = t23.y; cc[3] = t23.w;
  }
  const OrbxResizeTap* ytaps = taps + L.ytab_off;
  if (L.win8) {
    if (rpw == 8)
      pyr_rows<8, true>(src, in_stride, w0, h0, ytaps, yb, L.h, ofs, cc, rout, voff_st, vmask, pitch);
    else
      pyr_rows<4, true>(src, in_stride, w0, h0, ytaps, yb, L.h, ofs, cc, rout, voff_st, vmask, pitch);
  } else {
    pyr_rows<4, false>(src, in_stride, w0, h0, ytaps, yb, L.h, ofs, cc, rout, voff_st, vmask, pitch);
  }
}

// ---------------------------------------------------------------------------
// 2. 5x5 Gaussian blur, REFLECT_101.
//    kind 0: separable [1 4 6 4 1]/16 twice then round-half-even
//            == rne(sum_ij w_i w_j p / 256)   (src/cuda/GaussianBlur1D.cu:34-163;
//            every float intermediate there is an exact dyadic, so integer
//            arithmetic reproduces it bit for bit)
//    kind 1: 5x5 /273 kernel, rne(S/273)      (src/cuda/GaussianBlur.cu:21-130;
//            S/273 is never within float error of a .5 tie because 273 is odd)
//    Levels below first_level are copied unchanged.
#define BLUR_SROWS (ORBX_BLUR_TH + 4)
#define BLUR_SPITCH 72  // bytes: x0-4 .. x0+67

__device__ __forceinline__ void blur_load_tile(uint8_t* s_src, const uint8_t* img, const OrbxLevel& L, int x0,
                                               int y0) {
  uint32_t* s32 = reinterpret_cast<uint32_t*>(s_src);
  for (int i = threadIdx.x; i < BLUR_SROWS * (BLUR_SPITCH / 4); i += 256) {
    const int row = i / (BLUR_SPITCH / 4), c = i - row * (BLUR_SPITCH / 4);
    const int gy = reflect101(y0 - 2 + row, L.h);
    const int gx = x0 - 4 + 4 * c;
    uint32_t v = 0;
    if (gx >= 0 && gx + 4 <= L.pitch) v = *reinterpret_cast<const uint32_t*>(img + (size_t)gy * L.pitch + gx);
    s32[i] = v;
  }
  __syncthreads();
  // horizontal REFLECT_101 fix-up of the two halo columns on image borders
  if (threadIdx.x < BLUR_SROWS) {
    uint8_t* row = s_src + threadIdx.x * BLUR_SPITCH;
    if (x0 == 0) {
      row[3] = row[5];  // x=-1 <- x=1
      row[2] = row[6];  // x=-2 <- x=2
    }
    const int rem = L.w - x0;  // valid columns in this tile
    if (rem <= ORBX_BLUR_TW + 1) {
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int x = L.w + k;  // needs reflect
        const int col = x - x0 + 4;
        if (col < BLUR_SPITCH) row[col] = row[(2 * L.w - x - 2) - x0 + 4];
      }
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_blur(OrbxPlan plan, OrbxTileMap tm, const uint8_t* __restrict__ src,
                                              uint8_t* __restrict__ dst, int first_level, int kind) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[BLUR_SROWS * BLUR_SPITCH];
  __shared__ __attribute__((aligned(16))) uint16_t s_h[BLUR_SROWS * ORBX_BLUR_TW];
  int l, tx, ty;
  decode_tile(tm, plan.nlevels, l, tx, ty);
  const OrbxLevel& L = plan.L[l];
  const int f = blockIdx.y;
  const uint8_t* img = src + (size_t)f * plan.frame_bytes + L.img_off;
  uint8_t* out = dst + (size_t)f * plan.frame_bytes + L.img_off;
  const int x0 = tx * ORBX_BLUR_TW, y0 = ty * ORBX_BLUR_TH;
  const int c4 = (threadIdx.x & 15) * 4, r = threadIdx.x >> 4;
  const int gy = y0 + r, gx = x0 + c4;

  if (l < first_level) {  // pass-through copy
    if (gy < L.h && gx < L.pitch)
      *reinterpret_cast<uint32_t*>(out + (size_t)gy * L.pitch + gx) =
          *reinterpret_cast<const uint32_t*>(img + (size_t)gy * L.pitch + gx);
    return;
  }
  blur_load_tile(s_src, img, L, x0, y0);

  uint32_t packed = 0;
  if (kind == 0) {
    // horizontal pass -> u16 (<= 4080)
    for (int i = threadIdx.x; i < BLUR_SROWS * ORBX_BLUR_TW; i += 256) {
      const int row = i >> 6, c = i & 63;
      const uint8_t* p = s_src + row * BLUR_SPITCH + c + 2;  // p[0] is x-2
      s_h[i] = (uint16_t)(p[0] + 4 * p[1] + 6 * p[2] + 4 * p[3] + p[4]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint16_t* h = s_h + r * ORBX_BLUR_TW + c4 + k;  // h[0] is y-2
      const uint32_t S = h[0] + 4u * h[ORBX_BLUR_TW] + 6u * h[2 * ORBX_BLUR_TW] + 4u * h[3 * ORBX_BLUR_TW] +
                         h[4 * ORBX_BLUR_TW];
      const uint32_t v = (S + 127u + ((S >> 8) & 1u)) >> 8;  // round-half-even of S/256
      if (gx + k < L.w) packed |= v << (8 * k);
    }
  } else {
    const int kw[25] = {1, 4, 7, 4, 1, 4, 16, 26, 16, 4, 7, 26, 41, 26, 7, 4, 16, 26, 16, 4, 1, 4, 7, 4, 1};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t S = 0;
#pragma unroll
      for (int i = 0; i < 5; i++)
#pragma unroll
        for (int j = 0; j < 5; j++) S += (uint32_t)kw[i * 5 + j] * s_src[(r + i) * BLUR_SPITCH + c4 + k + 2 + j];
      const uint32_t v = (2u * S + 273u) / 546u;  // nearest integer to S/273 (no ties exist)
      if (gx + k < L.w) packed |= v << (8 * k);
    }
  }
  if (gy < L.h && gx < L.pitch) *reinterpret_cast<uint32_t*>(out + (size_t)gy * L.pitch + gx) = packed;
}

// (2b. register-streaming separable blur: orbx_blur.hip)

// (3. FAST-n segment test + score + NMS: orbx_fast.hip)

// ---------------------------------------------------------------------------
// 4. (stage operators Fast()/NMS() only; the whole path uses the fused kernel below)
//    ordered compaction of the survivor mask: one workgroup per (level,
//    frame) walks the mask words in row-major order, a block-wide exclusive
//    scan of popcounts gives every set bit its row-major rank, the first
//    `cap` are written (src/orb_cpu.cpp:108-110 order and cap -- NOT the
//    atomicAdd order of src/cuda/NMS.cu:123).
__global__ __launch_bounds__(256) void k_compact(OrbxPlan plan, const u64* __restrict__ mask,
                                                 orbx_keypoint* __restrict__ cand,
                                                 int32_t* __restrict__ cand_count,
                                                 int32_t* __restrict__ cand_total, int need_total) {
  __shared__ int s_wsum[4];
  const int l = blockIdx.x, f = blockIdx.y;
  const OrbxLevel& L = plan.L[l];
  const u64* m = mask + (size_t)f * plan.mask_words + L.mask_off;
  orbx_keypoint* out = cand + (size_t)f * plan.cand_total + L.cand_off;
  const int nwords = L.h * L.mask_wpr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int w0 = 0; w0 < nwords; w0 += 256) {
    const int i = w0 + tid;
    u64 v = i < nwords ? m[i] : 0ull;
    const int c = __popcll(v);
    const int incl = wave_scan_incl(c);
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int s = s_wsum[k];
      if (k < wave) woff += s;
      tot += s;
    }
    int pos = base + woff + incl - c;
    if (c && pos < L.cap) {
      const int y = i / L.mask_wpr, xw = i - y * L.mask_wpr;
      while (v && pos < L.cap) {
        const int b = __ffsll((long long)v) - 1;
        v &= v - 1;
        orbx_keypoint kp;
        kp.x = orbx_mask_x(L, xw, b);
        kp.y = y;
        out[pos++] = kp;
      }
    }
    base += tot;
    __syncthreads();
    // the cap is reached (block-uniform): later rows cannot contribute; `total`
    // is then only a lower bound, which the whole-path callers never read
    if (!need_total && base >= L.cap) break;
  }
  if (tid == 0) {
    cand_total[f * plan.nlevels + l] = base;
    cand_count[f * plan.nlevels + l] = base < L.cap ? base : L.cap;
  }
}

// ---------------------------------------------------------------------------
// 5. Harris response at the candidate keypoints (intent of
//    src/cuda/HarrisScore.cu:23-89, DESIGN.md "Harris"): float Sobel with
//    REFLECT_101, window x window Gaussian of Ix^2, IxIy, Iy^2 accumulated in
//    (i,j) row-major order, R = (AC - B^2) - (k*(A+C))*(A+C).
//    Evaluated only in the (window+2)^2 neighbourhood of each candidate
//    instead of 5 full-frame convolutions.
__device__ __forceinline__ float harris_at(const uint8_t* img, int w, int h, int pitch, int x, int y,
                                           const float* __restrict__ g, int K, float kk) {
  const int r = K / 2;
  float a = 0.f, b = 0.f, c = 0.f;
  for (int i = 0; i < K; i++) {
    const int yy = reflect101(y - r + i, h);
    const uint8_t* r0 = img + (size_t)reflect101(yy - 1, h) * pitch;
    const uint8_t* r1 = img + (size_t)yy * pitch;
    const uint8_t* r2 = img + (size_t)reflect101(yy + 1, h) * pitch;
    for (int j = 0; j < K; j++) {
      const int xx = reflect101(x - r + j, w);
      const int xl = reflect101(xx - 1, w), xr = reflect101(xx + 1, w);
      const int p00 = r0[xl], p01 = r0[xx], p02 = r0[xr];
      const int p10 = r1[xl], p12 = r1[xr];
      const int p20 = r2[xl], p21 = r2[xx], p22 = r2[xr];
      const float gx = (float)((p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20));
      const float gy = (float)((p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02));
      const float wgt = g[i * K + j];
      a = __fadd_rn(a, __fmul_rn(__fmul_rn(gx, gx), wgt));
      c = __fadd_rn(c, __fmul_rn(__fmul_rn(gy, gy), wgt));
      b = __fadd_rn(b, __fmul_rn(__fmul_rn(gx, gy), wgt));
    }
  }
  const float det = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b));
  const float trace = __fadd_rn(a, c);
  return __fsub_rn(det, __fmul_rn(__fmul_rn(kk, trace), trace));
}

// Fast path for window K <= 7 and keypoints whose (K+2)^2 pixel neighbourhood leaves
// the image by at most ONE row / column (FAST keypoints keep 3 px from the border,
// so with K = 7 that is every keypoint of the whole path; the reflected row is a
// different row pointer, the reflected column one v_perm per row).  A row of the
// neighbourhood is 3 aligned dword loads, byte-aligned in registers (v_alignbyte)
// and unpacked with v_perm into u16 PAIRS: E[k] = (p[2k], p[2k+1]) and
// O[k] = (p[2k+1], p[2k+2]).  The Sobel sums are formed two at a time on those pairs
// (v_pk_add_u16 / v_pk_sub_i16; a 1-2-1 sum is at most 1020, a difference at most
// 1020 in magnitude), and only gx and gy become floats (v_cvt_f32_i32 on a 16-bit
// half).  The rows are requested a few ahead of the row being consumed, so the live
// set is two packed rows of vertical partial sums, three packed rows of horizontal
// sums and the dwords in flight (the compiler's scheduler moves the loads as the
// register bound of the kernel allows: k_level_select<7> and k_lvl_harris fit 80
// VGPRs without scratch, `make resource-usage`).
// Every integer intermediate is exact, and the weighted accumulation keeps the
// (i,j) order and the separate mul/mul/add roundings of harris_at, so the result
// is bit-identical to it.
#define HARRIS_AHEAD 2  // rows fetched ahead of the row being unpacked
template <int K>
__device__ __forceinline__ float harris_fast(const uint8_t* img, int w, int h, int pitch, int x, int y,
                                             const float* __restrict__ g, float kk) {
  constexpr int r = K / 2, P = K + 2;
  constexpr int NE = (P + 1) / 2, NH = (K + 1) / 2;  // pairs of a pixel row / of a row of Sobel sums
  static_assert(P <= 9, "the third dword of a row supplies pixel 8 only");
  const int xs = x - r - 1;               // >= -1
  const int a0 = xs & ~3, off = xs - a0;  // xs == -1: a0 = -4, off = 3
  // BORDER_REFLECT_101 of the one column that may lie outside: pixel -1 is pixel 1 (window pixel 0 takes window
  // pixel 2), pixel w is pixel w-2 (window pixel P-1 takes window pixel P-3).  perm(a, b, sel): selector bytes
  // 0..3 pick from b, 4..7 from a
  constexpr int dr = P - 1, sr = P - 3;
  constexpr uint32_t id = 0x03020100u;
  constexpr uint32_t rfl = (id & ~(0xffu << (8 * (dr & 3)))) | ((uint32_t)(4 + (sr & 3)) << (8 * (dr & 3)));
  const uint32_t sel_l = xs < 0 ? 0x03020102u : id;
  const uint32_t sel_r = xs + P - 1 >= w ? rfl : id;
  uint32_t raw[P][3];
  auto fetch = [&](int i) {
    int yy = y - r - 1 + i;  // only the first / last row can be outside (by one)
    if (i == 0) yy = yy < 0 ? 1 : yy;
    if (i == P - 1) yy = yy >= h ? h - 2 : yy;
    const int o = yy * pitch + a0;
    // o == -4 only in row 0 with the left column reflected; that dword supplies nothing
    // but the replaced pixel, so any readable address will do
    // (unsigned 32-bit offsets from the level's base: one address register per load, not a 64-bit pair)
    const uint32_t o1 = (uint32_t)(o + 4);
    raw[i][0] = *reinterpret_cast<const uint32_t*>(img + (uint32_t)max(o, 0));
    raw[i][1] = *reinterpret_cast<const uint32_t*>(img + o1);
    raw[i][2] = *reinterpret_cast<const uint32_t*>(img + o1 + 4);  // may run into the next row / the pool's tail slack
  };
  // window pixels a and b of a row as one u16 pair (b past the row: 0)
  auto pair = [&](const uint32_t (&q)[3], int pa, int pb) {
    const uint32_t sel = 0x0c000c00u | (uint32_t)(pa & 3) | (pb < P ? (uint32_t)(4 + (pb & 3)) << 16 : 0x000c0000u);
    return __builtin_amdgcn_perm(q[pb < P ? pb >> 2 : 0], q[pa >> 2], sel);
  };
  // row i: E pairs in e[], horizontal 1-2-1 sums (hs[2k], hs[2k+1]) in hs[]
  auto unpack = [&](int i, uint32_t (&e)[NE], uint32_t (&hs)[NH]) {
    uint32_t q[3] = {__builtin_amdgcn_alignbyte(raw[i][1], raw[i][0], off),
                     __builtin_amdgcn_alignbyte(raw[i][2], raw[i][1], off), raw[i][2] >> (8 * off)};
    q[dr >> 2] = __builtin_amdgcn_perm(q[sr >> 2], q[dr >> 2], sel_r);
    q[0] = __builtin_amdgcn_perm(q[0], q[0], sel_l);
#pragma unroll
    for (int k = 0; k < NE; k++) e[k] = pair(q, 2 * k, 2 * k + 1);
#pragma unroll
    for (int k = 0; k < NH; k++) {
      const uint32_t o = pair(q, 2 * k + 1, 2 * k + 2);
      hs[k] = pk_add(pk_add(e[k], o), pk_add(o, e[k + 1]));
    }
  };
#pragma unroll
  for (int i = 0; i < HARRIS_AHEAD && i < P; i++) fetch(i);
  // t[k]: rows i and i+1 added (vertical partial sum), the window row's 1-2-1 column sum is t(i) + t(i+1)
  uint32_t e0[NE], e1[NE], t[NE], hs[3][NH];
  if (HARRIS_AHEAD < P) fetch(HARRIS_AHEAD);
  unpack(0, e0, hs[0]);
  if (HARRIS_AHEAD + 1 < P) fetch(HARRIS_AHEAD + 1);
  unpack(1, e1, hs[1]);
#pragma unroll
  for (int k = 0; k < NE; k++) t[k] = pk_add(e0[k], e1[k]);
  float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
  for (int i = 0; i < K; i++) {
    // patch rows i, i+1, i+2 feed window row i; their hs live in slots i%3, (i+1)%3, (i+2)%3; e1 is row i+1
    if (i + 2 + HARRIS_AHEAD < P) fetch(i + 2 + HARRIS_AHEAD);
    uint32_t e2[NE], vs[NE];
    unpack(i + 2, e2, hs[(i + 2) % 3]);
#pragma unroll
    for (int k = 0; k < NE; k++) {
      const uint32_t t2 = pk_add(e1[k], e2[k]);
      vs[k] = pk_add(t[k], t2);
      t[k] = t2;
      e1[k] = e2[k];
    }
#pragma unroll
    for (int k = 0; k < NH; k++) {
      const uint32_t gx2 = pk_sub(vs[k + 1], vs[k]);  // (vs[2k+2] - vs[2k], vs[2k+3] - vs[2k+1])
      const uint32_t gy2 = pk_sub(hs[(i + 2) % 3][k], hs[i % 3][k]);
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int j = 2 * k + s;
        if (j >= K) break;
        const float gx = s ? (float)((int32_t)gx2 >> 16) : (float)(int16_t)gx2;
        const float gy = s ? (float)((int32_t)gy2 >> 16) : (float)(int16_t)gy2;
        const float wgt = g[i * K + j];
        a = __fadd_rn(a, __fmul_rn(__fmul_rn(gx, gx), wgt));
        c = __fadd_rn(c, __fmul_rn(__fmul_rn(gy, gy), wgt));
        b = __fadd_rn(b, __fmul_rn(__fmul_rn(gx, gy), wgt));
      }
    }
  }
  const float det = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b));
  const float trace = __fadd_rn(a, c);
  return __fsub_rn(det, __fmul_rn(__fmul_rn(kk, trace), trace));
}

// harris_fast<K> takes (K+2)^2 windows that leave the image by at most one pixel (k_level_select's two Harris passes
// must agree with harris_any on this, bit-identity depends on it)
__device__ __forceinline__ bool harris_fast_ok(int w, int h, int x, int y, int K) {
  const int m = K / 2 + 1;
  return x >= m - 1 && y >= m - 1 && x <= w - m && y <= h - m && w >= 4 && h >= 4;
}

__device__ __forceinline__ float harris_any(const uint8_t* img, int w, int h, int pitch, int x, int y,
                                            const float* __restrict__ g, int K, float kk) {
  if (harris_fast_ok(w, h, x, y, K)) {
    if (K == 7) return harris_fast<7>(img, w, h, pitch, x, y, g, kk);
    if (K == 5) return harris_fast<5>(img, w, h, pitch, x, y, g, kk);
    if (K == 3) return harris_fast<3>(img, w, h, pitch, x, y, g, kk);
  }
  return harris_at(img, w, h, pitch, x, y, g, K, kk);
}

// Eight lanes per keypoint (second generation): lane r of a group computes window
// row r -- three patch rows, the Sobel sums and the 3 x K weighted products of that
// row -- in parallel with its neighbours; the float accumulators then travel
// lane 0 -> 1 -> ... -> K-1 (DPP row_shr:1), each lane adding its K products in
// order, which reproduces the oracle's (i,j) row-major summation bit for bit.
// 8x more waves than thread-per-keypoint (the old kernel had 2 waves per SIMD)
// and a ~6x shorter dependent chain per keypoint.
// RPL window rows per lane, G = lanes per keypoint (power of two >= ceil(K/RPL)).
template <int K, int RPL, int G>
__device__ __forceinline__ float harris_row_group(const uint8_t* img, int pitch, int x, int y,
                                                  const float* __restrict__ g, float kk, int sub) {
  constexpr int r = K / 2, P = K + 2, NR = RPL + 2;  // NR patch rows feed RPL window rows
  constexpr int NL = (K + RPL - 1) / RPL;            // lanes that own rows
  const int row0 = (sub < NL ? sub : NL - 1) * RPL;  // idle lanes shadow the last group (sums never used)
  const int xs = x - r - 1;
  const int a0 = xs & ~3, off = xs - a0;
  float p[NR][P];
#pragma unroll
  for (int i = 0; i < NR; i++) {
    // rows past the window (last lane when K is not a multiple of RPL) repeat the last patch row
    const int pr = min(row0 + i, P - 1);
    const uint32_t* row = reinterpret_cast<const uint32_t*>(img + (size_t)(y - r - 1 + pr) * pitch + a0);
    const uint32_t d0 = row[0], d1 = row[1], d2 = row[2];
    const uint32_t q[3] = {__builtin_amdgcn_alignbyte(d1, d0, off), __builtin_amdgcn_alignbyte(d2, d1, off),
                           d2 >> (8 * off)};
#pragma unroll
    for (int j = 0; j < P; j++) p[i][j] = (float)((q[j >> 2] >> (8 * (j & 3))) & 0xffu);
  }
  float hs[NR][K];
#pragma unroll
  for (int i = 0; i < NR; i++)
#pragma unroll
    for (int j = 0; j < K; j++) hs[i][j] = p[i][j] + 2.0f * p[i][j + 1] + p[i][j + 2];
  float pa[RPL][K], pb[RPL][K], pc[RPL][K];
#pragma unroll
  for (int w = 0; w < RPL; w++) {
    float vs[P];
#pragma unroll
    for (int j = 0; j < P; j++) vs[j] = p[w][j] + 2.0f * p[w + 1][j] + p[w + 2][j];
    const int wr = min(row0 + w, K - 1);
#pragma unroll
    for (int j = 0; j < K; j++) {
      const float gx = vs[j + 2] - vs[j], gy = hs[w + 2][j] - hs[w][j];
      const float wgt = g[wr * K + j];
      pa[w][j] = __fmul_rn(__fmul_rn(gx, gx), wgt);
      pc[w][j] = __fmul_rn(__fmul_rn(gy, gy), wgt);
      pb[w][j] = __fmul_rn(__fmul_rn(gx, gy), wgt);
    }
  }
  float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
  for (int rr = 0; rr < NL; rr++) {
    if (sub == rr) {
#pragma unroll
      for (int w = 0; w < RPL; w++)
        if (rr * RPL + w < K) {
#pragma unroll
          for (int j = 0; j < K; j++) {
            a = __fadd_rn(a, pa[w][j]);
            c = __fadd_rn(c, pc[w][j]);
            b = __fadd_rn(b, pb[w][j]);
          }
        }
    }
    if (rr + 1 < NL) {  // hand the running sums to the next lane of the group
      const float an = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), 0x111, 0xf, 0xf, true));
      const float bn = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, b), 0x111, 0xf, 0xf, true));
      const float cn = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, c), 0x111, 0xf, 0xf, true));
      if (sub == rr + 1) {
        a = an;
        b = bn;
        c = cn;
      }
    }
  }
  const float det = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b));
  const float trace = __fadd_rn(a, c);
  return __fsub_rn(det, __fmul_rn(__fmul_rn(kk, trace), trace));  // valid in lane sub == NL-1
}

// one keypoint per G-lane group; the result is valid in the lane `writer` says
template <int RPL, int G>
__device__ __forceinline__ float harris_group(const uint8_t* img, int w, int h, int pitch, int x, int y,
                                              const float* __restrict__ g, int K, float kk, int sub, bool active,
                                              bool& writer) {
  const int m = K / 2 + 1;
  const bool fast = (K == 7 || K == 5 || K == 3) && x >= m && y >= m && x < w - m && y < h - m;
  float res = 0.f;
  writer = false;
  // the fast path is taken group-wise but executed wave-wide (DPP needs all lanes of the row active)
  const bool any_fast = __any(active && fast);
  if (any_fast) {
    const int xx = (active && fast) ? x : m, yy = (active && fast) ? y : m;  // harmless in-image stand-in
    float v = 0.f;
    int last = 0;
    if (K == 7) {
      v = harris_row_group<7, RPL, G>(img, pitch, xx, yy, g, kk, sub);
      last = (7 + RPL - 1) / RPL - 1;
    } else if (K == 5) {
      v = harris_row_group<5, RPL, G>(img, pitch, xx, yy, g, kk, sub);
      last = (5 + RPL - 1) / RPL - 1;
    } else {
      v = harris_row_group<3, RPL, G>(img, pitch, xx, yy, g, kk, sub);
      last = (3 + RPL - 1) / RPL - 1;
    }
    if (active && fast && sub == last) {
      res = v;
      writer = true;
    }
  }
  if (active && !fast && sub == 0) {
    res = harris_at(img, w, h, pitch, x, y, g, K, kk);
    writer = true;
  }
  return res;
}

__global__ __launch_bounds__(256) void k_harris2_flat(const uint8_t* __restrict__ img, int w, int h, int pitch,
                                                      const orbx_keypoint* __restrict__ kps, int nkp,
                                                      const float* __restrict__ gauss, int K, float kk,
                                                      float* __restrict__ resp) {
  constexpr int G = 8, RPL = 1;
  const int j = blockIdx.x * 32 + (threadIdx.x >> 3), sub = threadIdx.x & 7;
  const bool active = j < nkp;
  orbx_keypoint kp = {4, 4};
  if (active) kp = kps[j];
  bool writer;
  const float v = harris_group<RPL, G>(img, w, h, pitch, kp.x, kp.y, gauss, K, kk, sub, active, writer);
  if (writer) resp[j] = v;
}


// ---------------------------------------------------------------------------
// 4-6 fused: ordered compaction -> Harris -> top-N selection, one 512-thread
// workgroup per group of levels of a frame: all of them in large batches (no
// lane idles but in a level's last run of 64), one in small batches (more
// workgroups than frames; see orbx_launch_level_select).  Ranks come from
// sorted runs instead of n^2 key compares per level.
//   phase 1  wave w walks the masks of the group's levels w, w + 8, ...: row-major order,
//            wave scan of popcounts, first `cap` survivors -> LDS slots of the
//            level (src/orb_cpu.cpp:108-110 order and cap).  Row-major mode:
//            straight to the output slots, done.
//   phase 2  Harris, thread per candidate, a wave per run of 64 candidates of
//            one level (the group's runs dealt over the 8 waves) -> (response desc, index asc)
//            u64 keys, each run sorted in registers (bitonic)
//   phase 3  a key's rank is its place in its run plus a binary search in every
//            other run of its level; ranks < quota are written
// A level owns LVL_RUN-aligned slots [slot_l, slot_l + cap rounded up); keys past
// its count are 0, below every real key (the low word ~index is never 0).
// The selected keypoints of level l go to the STATIC slots [out_off_l, out_off_l
// + quota_l) of the frame (out_off_l = sum of the lower levels' quotas) plus a
// per-level count; k_describe2 compacts them into the final order.
#define LVL_THREADS 512
#define LVL_WAVES (LVL_THREADS / 64)
#define LVL_Q 16    // consecutive mask words a lane owns in a chunk of a compaction walk (1024 per wave and chunk)
#define LVL_RUN 64  // keys per sorted run
#define LVL_MAX_SLOTS 4096  // candidate slots of a frame the kernel holds in LDS (16 B each)

// LDS slots of a plan's frame in k_level_select (each level's cap rounded up to whole runs)
__host__ __device__ inline int lvl_slots(const OrbxPlan& plan, int nl) {
  int s = 0;
  for (int l = 0; l < nl; l++) s += (plan.L[l].cap + LVL_RUN - 1) & ~(LVL_RUN - 1);
  return s;
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)v, m), hi = __shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}

// the 64 keys of a wave, one per lane, sorted descending (lane 0 holds the largest)
__device__ __forceinline__ u64 wave_sort_desc(u64 k, int lane) {
#pragma unroll
  for (int b = 2; b <= 64; b <<= 1)
#pragma unroll
    for (int j = b >> 1; j > 0; j >>= 1) {
      const u64 o = shfl_xor_u64(k, j);
      // the lower lane of a pair keeps the larger key in blocks sorted descending ((lane & b) == 0)
      const bool keep_max = ((lane & j) == 0) == ((lane & b) == 0);
      k = keep_max ? (o > k ? o : k) : (o < k ? o : k);
    }
  return k;
}

// run r of the level-ordered list of runs of levels [l0, l1) -> (level, run within it); uniform
__device__ __forceinline__ int lvl_of_run(const int* s_runs, int l0, int l1, int& r) {
  int l = l0;
  while (l < l1 - 1) {
    const int c = __builtin_amdgcn_readfirstlane(s_runs[l]);
    if (r < c) break;
    r -= c;
    l++;
  }
  return l;
}

// The lane index, worked out again where it is used (v_mbcnt of an all-ones mask) instead of being carried in a
// register from the kernel's entry: the zero it starts from passes through an empty `asm`, so the compiler can neither
// merge this with an earlier copy nor hoist it, and the value is not live before this point
__device__ __forceinline__ int lane_reread() {
  uint32_t z = 0;
  asm volatile("" : "+v"(z));
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
}

// KF: the Harris window of the fast path (3, 5 or 7; 0: none, every candidate through harris_at)
template <int KF>
__global__ __launch_bounds__(LVL_THREADS) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_level_select(
    OrbxPlan plan, int lpg, int mode, const u64* __restrict__ mask, const uint8_t* __restrict__ pyr,
    const float* __restrict__ gauss, int K, float kk, orbx_keypoint* __restrict__ sel_lkp,
    float* __restrict__ sel_resp, int32_t* __restrict__ sel_count, uint32_t* __restrict__ need) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ int s_n[ORBX_MAX_LEVELS];      // candidates of each level
  __shared__ int s_runs[ORBX_MAX_LEVELS];   // runs of 64 keys of each level
  // grid = (frames, level groups), the frame index dispatched fastest: workgroups are dealt round-robin over the 8
  // XCDs.  Workgroup (f, g) selects levels [g * lpg, (g + 1) * lpg) of frame f
  const int f = blockIdx.x, nl = plan.nlevels;
  const int l0 = blockIdx.y * lpg, l1 = min(l0 + lpg, nl);
  const int nslots = lvl_slots(plan, nl);
  u64* s_key = reinterpret_cast<u64*>(s_dyn);                            // [nslots]
  uint32_t* s_kp = reinterpret_cast<uint32_t*>(s_dyn + 8 * (size_t)nslots);  // [nslots]  y << 16 | x
  float* s_r = reinterpret_cast<float*>(s_dyn + 12 * (size_t)nslots);     // [nslots]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t fo = (size_t)f * plan.out_cap;

  // phase 1: ordered compaction, one wave per level
  for (int l = l0 + wave; l < l1; l += LVL_WAVES) {
    const OrbxLevel& L = plan.L[l];
    const int cap = L.cap, slot = lvl_slots(plan, l);
    const u64* m = mask + (size_t)f * plan.mask_words + L.mask_off;
    const int nwords = L.h * L.mask_wpr;
    int base = 0, last = -1;  // last: row of survivor cap - 1 (in the lane that found it)
    // A lane owns LVL_Q consecutive words of the chunk: their popcounts and the prefix over them stay in its
    // registers, ONE wave scan of the lanes' totals places them, and the lane emits its words in order (row-major)
    for (int w0 = 0; w0 < nwords && base < cap; w0 += 64 * LVL_Q) {
      const int i0 = w0 + LVL_Q * lane;
      u64 v[LVL_Q];
      int tot = 0;
#pragma unroll
      for (int q = 0; q < LVL_Q; q++) {
        v[q] = i0 + q < nwords ? m[i0 + q] : 0ull;
        tot += __popcll(v[q]);
      }
      const int incl = wave_scan_incl(tot);
      int pos = base + incl - tot;
      if (tot && pos < cap) {
        int y = i0 / L.mask_wpr, xw = i0 - y * L.mask_wpr;
#pragma unroll
        for (int q = 0; q < LVL_Q; q++) {
          u64 w = v[q];
          while (w && pos < cap) {
            const int b = __ffsll((long long)w) - 1;
            w &= w - 1;
            const int x = orbx_mask_x(L, xw, b);
            if (mode == ORBX_SELECT_ROWMAJOR) {  // cap == quota: the survivor is selected
              orbx_keypoint kp;
              kp.x = x;
              kp.y = y;
              sel_lkp[fo + L.out_off + pos] = kp;
              sel_resp[fo + L.out_off + pos] = 0.0f;
            } else {
              s_kp[slot + pos] = ((uint32_t)y << 16) | (uint32_t)x;
            }
            if (pos == cap - 1) last = y;
            pos++;
          }
          if (++xw == L.mask_wpr) {
            xw = 0;
            y++;
          }
        }
      }
      base += __builtin_amdgcn_readlane(incl, 63);
    }
    const int n = base < cap ? base : cap;
    const int keep = n < L.quota ? n : L.quota;
    const int runs = (n + LVL_RUN - 1) / LVL_RUN;
    const u64 found = __ballot(last >= 0);
    const int last_row = found ? __builtin_amdgcn_readlane(last, __ffsll((long long)found) - 1) : L.h - 1;
    if (lane == 0) {
      s_n[l] = n;
      s_runs[l] = runs;
      sel_count[f * nl + l] = keep;
      // How many rows of the level did it take to fill the cap (all of them if it never filled)?  The maximum over
      // the batch's frames goes to the host, which sizes the first pass of the top-rows-first pipeline by it
      // (orbx_adapt.h, adapt_tile_rows): a heuristic's input, results never depend on it.
      // ... and the frames counted by that row, in buckets (orbx_plan.h, fill_bucket of last_row + 1): where to cut
      // the first pass so that most frames' units of its second tile row exit
      if (need && cap > 0) {
        atomicMax(&need[l], (uint32_t)last_row + 1u);
        atomicAdd(&need[ORBX_MAX_LEVELS + l * ORBX_FILL_BUCKETS + min(last_row / ORBX_FILL_BUCKET_ROWS, ORBX_FILL_BUCKETS - 1)], 1u);
      }
    }
  }
  if (mode == ORBX_SELECT_ROWMAJOR) return;
  __syncthreads();

  int nruns = 0;
  for (int l = l0; l < l1; l++) nruns += s_runs[l];
  nruns = __builtin_amdgcn_readfirstlane(nruns);
  // phases 2 + 3a: a wave takes one run of 64 candidates of one level at a time (the level's image, size and slots
  // stay wave-uniform).  First pass: Harris of the candidates that harris_any would give its window-K fast path.
  // Second pass, over the same runs: the rest through harris_at, then the run's keys are sorted in registers.  With
  // both paths in one loop the kernel spills at 128 registers.
  const uint8_t* img_f = pyr + (size_t)f * plan.frame_bytes;
  if constexpr (KF > 0) {
    for (int t = wave; t < nruns; t += LVL_WAVES) {
      int r = t;
      const int l = lvl_of_run(s_runs, l0, l1, r);
      const OrbxLevel& L = plan.L[l];
      const int slot = lvl_slots(plan, l), i = LVL_RUN * r + lane_reread();
      const bool live = i < __builtin_amdgcn_readfirstlane(s_n[l]);
      const uint32_t p = live ? s_kp[slot + i] : 0u;
      const int x = (int)(p & 0xffffu), y = (int)(p >> 16);
      const bool fast = live && harris_fast_ok(L.w, L.h, x, y, KF);
      if (fast) {
        const float resp = harris_fast<KF>(img_f + L.img_off, L.w, L.h, L.pitch, x, y, gauss, kk);
        // the lane index is read again here instead of being carried through the Harris arithmetic, whose live set
        // decides the kernel's register count (80 VGPRs: 6 waves per SIMD)
        s_r[slot + LVL_RUN * r + lane_reread()] = resp;
      }
    }
  }
  for (int t = wave; t < nruns; t += LVL_WAVES) {
    int r = t;
    const int l = lvl_of_run(s_runs, l0, l1, r);
    const OrbxLevel& L = plan.L[l];
    const int ln = lane_reread();
    const int slot = lvl_slots(plan, l), i = LVL_RUN * r + ln;
    u64 key = 0ull;  // past the level's count: below every real key
    if (i < __builtin_amdgcn_readfirstlane(s_n[l])) {
      const uint32_t p = s_kp[slot + i];
      const int x = (int)(p & 0xffffu), y = (int)(p >> 16);
      const bool fast = KF > 0 && harris_fast_ok(L.w, L.h, x, y, KF);
      float resp;
      if (fast) {
        resp = s_r[slot + i];
      } else {
        resp = harris_at(img_f + L.img_off, L.w, L.h, L.pitch, x, y, gauss, K, kk);
        s_r[slot + i] = resp;
      }
      uint32_t u = orbx_f2u(resp);
      if (u == 0x80000000u) u = 0u;
      u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
      key = ((u64)u << 32) | (uint32_t)~(uint32_t)i;
    }
    s_key[slot + i] = wave_sort_desc(key, ln);
  }
  __syncthreads();
  // phase 3b: rank = place in the own run + keys above it in the level's other runs
  for (int t = wave; t < nruns; t += LVL_WAVES) {
    int r = t;
    const int l = lvl_of_run(s_runs, l0, l1, r);
    const int slot = lvl_slots(plan, l);
    const int runs = __builtin_amdgcn_readfirstlane(s_runs[l]);
    const int ln = lane_reread();
    const u64 k = s_key[slot + LVL_RUN * r + ln];
    int rank = ln;
    for (int o = 0; o < runs; o++) {
      if (o == r) continue;
      const u64* run = s_key + slot + LVL_RUN * o;
      int c = 0;  // keys of run o above k: the largest c <= 63 with run[c - 1] > k, then run[63]
#pragma unroll
      for (int step = LVL_RUN / 2; step > 0; step >>= 1) c += run[c + step - 1] > k ? step : 0;
      c += run[c] > k;
      rank += c;
    }
    const int n = __builtin_amdgcn_readfirstlane(s_n[l]);
    const int keep = n < plan.L[l].quota ? n : plan.L[l].quota;
    if (k != 0ull && rank < keep) {
      const int i = (int)~(uint32_t)k;
      const uint32_t p = s_kp[slot + i];
      orbx_keypoint kp;
      kp.x = (int)(p & 0xffffu);
      kp.y = (int)(p >> 16);
      const size_t so = fo + plan.L[l].out_off + rank;
      sel_lkp[so] = kp;
      sel_resp[so] = s_r[slot + i];
    }
  }
}

// ---------------------------------------------------------------------------
// 6c. The same selection as k_level_select, spread over the whole chip.  k_level_select does
//     everything for one frame in ONE workgroup and holds the frame's candidates in LDS.  Caps
//     above 512 (1920x1080, 4000 features: level 0 has ~1400 candidates), or more candidates per
//     frame than LVL_MAX_SLOTS, go to three short kernels instead (orbx_launch_level_select_auto;
//     measured when k_level_select still had one workgroup per (level, frame): 79 vs 110 us at
//     batch 16):
//       k_lvl_compact  (level, frame)                   first `cap` survivors, row-major
//       k_lvl_harris   (256 candidates, level, frame)   thread per candidate
//       k_lvl_rank     (64 candidates, level, frame)    4 threads per candidate
//     Same arithmetic, same order, same tie rule: results are identical.
__global__ __launch_bounds__(256) void k_lvl_compact(OrbxPlan plan, const u64* __restrict__ mask,
                                                     uint32_t* __restrict__ cand, int32_t* __restrict__ ncand,
                                                     uint32_t* __restrict__ need) {
  __shared__ int s_wsum[4][4];
  const int l = blockIdx.x, f = blockIdx.y;
  const OrbxLevel& L = plan.L[l];
  const int cap = L.cap;
  const u64* m = mask + (size_t)f * plan.mask_words + L.mask_off;
  uint32_t* out = cand + (size_t)f * plan.cand_total + L.cand_off;
  const int nwords = L.h * L.mask_wpr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  // four 256-word chunks per round: their loads are in flight together (one memory
  // round trip per 1024 words); words after the first `cap` survivors are never needed
  for (int w0 = 0; w0 < nwords && base < cap; w0 += 1024) {
    u64 v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int i = w0 + 256 * q + tid;
      v[q] = i < nwords ? m[i] : 0ull;
    }
    int incl[4], c[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      c[q] = __popcll(v[q]);
      incl[q] = wave_scan_incl(c[q]);
      if (lane == 63) s_wsum[q][wave] = incl[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
      int woff = 0, tot = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int sv = s_wsum[q][k];
        if (k < wave) woff += sv;
        tot += sv;
      }
      int pos = base + woff + incl[q] - c[q];
      if (c[q] && pos < cap) {
        const int i = w0 + 256 * q + tid;
        const int y = i / L.mask_wpr, xw = i - y * L.mask_wpr;
        u64 w = v[q];
        while (w && pos < cap) {
          const int b = __ffsll((long long)w) - 1;
          w &= w - 1;
          out[pos++] = ((uint32_t)y << 16) | (uint32_t)orbx_mask_x(L, xw, b);
        }
      }
      base += tot;
    }
    __syncthreads();
  }
  if (tid == 0) ncand[f * plan.nlevels + l] = base < cap ? base : cap;
  // rows the level needed to fill its cap, for the adaptive first pass (see k_level_select; out[] was written by
  // this workgroup before the loop's last barrier)
  if (need && tid == 0 && cap > 0) atomicMax(&need[l], base >= cap ? (out[cap - 1] >> 16) + 1u : (uint32_t)L.h);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 8))) void k_lvl_harris(
    OrbxPlan plan, const uint8_t* __restrict__ pyr, const float* __restrict__ gauss, int K, float kk,
    const uint32_t* __restrict__ cand, const int32_t* __restrict__ ncand, float* __restrict__ resp) {
  const int l = blockIdx.y, f = blockIdx.z;
  const OrbxLevel& L = plan.L[l];
  const int n = ncand[f * plan.nlevels + l];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if ((int)blockIdx.x * 256 >= n) return;  // whole workgroup
  if (i >= n) return;
  const size_t o = (size_t)f * plan.cand_total + L.cand_off + i;
  const uint32_t p = cand[o];
  const uint8_t* img = pyr + (size_t)f * plan.frame_bytes + L.img_off;
  resp[o] = harris_any(img, L.w, L.h, L.pitch, (int)(p & 0xffffu), (int)(p >> 16), gauss, K, kk);
}

#define RANK_SLICE 64
__global__ __launch_bounds__(256) void k_lvl_rank(OrbxPlan plan, const uint32_t* __restrict__ cand,
                                                  const int32_t* __restrict__ ncand, const float* __restrict__ resp,
                                                  orbx_keypoint* __restrict__ sel_lkp, float* __restrict__ sel_resp,
                                                  int32_t* __restrict__ sel_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ int s_part[4][RANK_SLICE];
  u64* s_key = reinterpret_cast<u64*>(s_dyn);  // [n rounded up to 8]
  const int l = blockIdx.y, f = blockIdx.z;
  const OrbxLevel& L = plan.L[l];
  const int n = ncand[f * plan.nlevels + l];
  const int keep = n < L.quota ? n : L.quota;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) sel_count[f * plan.nlevels + l] = keep;
  const int first = blockIdx.x * RANK_SLICE;
  if (first >= n) return;  // whole workgroup
  const size_t co = (size_t)f * plan.cand_total + L.cand_off;
  // all keys of the (level, frame): (response desc, index asc) as one u64, like k_level_select
  const int n8 = (n + 7) & ~7;
  for (int i = tid; i < n8; i += 256) {
    u64 key = 0ull;  // padding: the smallest key, never outranks anything
    if (i < n) {
      uint32_t u = orbx_f2u(resp[co + i]);
      if (u == 0x80000000u) u = 0u;
      u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
      key = ((u64)u << 32) | (uint32_t)~(uint32_t)i;
    }
    s_key[i] = key;
  }
  __syncthreads();
  // thread (ci, part): candidate first + ci against quarter `part` of the keys
  const int ci = tid & (RANK_SLICE - 1), part = tid >> 6;
  const int i = first + ci;
  const u64 ki = s_key[i < n8 ? i : 0];
  const int per = n8 / 4;  // multiple of 2
  int rank = 0;
  for (int j = part * per; j < (part + 1) * per; j += 2) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(&s_key[j]);
    rank += v.x > ki;
    rank += v.y > ki;
  }
  s_part[part][ci] = rank;
  __syncthreads();
  if (part == 0 && i < n) {
    rank = s_part[0][ci] + s_part[1][ci] + s_part[2][ci] + s_part[3][ci];
    if (rank < keep) {
      const uint32_t p = cand[co + i];
      const size_t so = (size_t)f * plan.out_cap + L.out_off;
      orbx_keypoint kp;
      kp.x = (int)(p & 0xffffu);
      kp.y = (int)(p >> 16);
      sel_lkp[so + rank] = kp;
      sel_resp[so + rank] = resp[co + i];
    }
  }
}

__global__ __launch_bounds__(256) void k_select_flat(const float* __restrict__ resp, int n, int keep,
                                                     int32_t* __restrict__ idx) {
  const int m = n < keep ? n : keep;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float ri = resp[i];
    int rank = 0;
    for (int j = 0; j < n; j++) {
      const float rj = resp[j];
      rank += (rj > ri) || (rj == ri && j < i);
    }
    if (rank < m) idx[rank] = i;
  }
}

// ---------------------------------------------------------------------------
// 7. (stage operators Orientations()/Brief() only; the whole path uses 7b)
//    orientation + rotated BRIEF-256, one wavefront per keypoint
//    (src/orb_cpu.cpp:139-258; src/cuda/Orientations.cu:22-63,
//    src/cuda/Brief.cu:40-95).
//    The 41x41 neighbourhood (pattern radius 18 + 5x5 box radius 2, and the
//    orientation patch) is loaded once into LDS with aligned dword loads,
//    zero-filled outside the image.  Moments are exact int32 reduced across
//    the wave; each lane then evaluates 4 of the 256 tests with 5x5 box sums
//    taken straight from the u8 patch (exact integers, no integral image),
//    and 4 ballots assemble the descriptor.
#include "orbx_describe.h"  // DESC_*, DescLds, DescJob, describe_wave

// ---------------------------------------------------------------------------
// 7b. orientation + BRIEF, second generation: a workgroup owns 16 keypoints.
//   The per-keypoint transcendental work (restated atan2f, sinf, cosf: ~350
//   instructions, identical in every lane of a wave-per-keypoint design) is
//   done by 16 THREADS, one per keypoint, between two passes in which each
//   wave serves its four keypoints:
//     pass A  patch -> LDS, exact int32 moments (wave reduce)
//     trig    thread j: angle_j, cos_j, sin_j
//     pass C  patch -> LDS again (L1/L2 hit), separable 5x5 box table,
//             256 rotated tests, 4 ballots
//   No test carries a bounds check.  For a keypoint within 20 px of the border
//   (wave-uniform test) the patch dwords outside the level are zeroed in LDS and
//   the table entries that the reference's skip rule excludes are tagged, so that
//   the comparison itself yields the skipped test's 0.
// KPW keypoints per wave (template parameter of k_describe2): 4 for throughput (the trig runs in 16 of a
// workgroup's threads), 1 for the few-keypoint / single-frame case where the chip is nearly empty and the
// latency of four descriptor passes in a row is what counts


#define DESC_NLD ((DESC_ROWS * (DESC_PITCH / 4) + 63) / 64)  // dwords per lane per patch (8)

// A keypoint whose 41 x 48 neighbourhood (rows py0.., bytes ax0..) crosses the level's border: the rows
// [rlo, rhi] and the byte columns [clo, chi] of the neighbourhood that lie inside the level, all wave-uniform.
// 0 <= y < h and 0 <= x < w <= pitch give rlo <= 20 <= rhi and clo <= 20 <= chi.
struct DescClip {
  int rlo, rhi, clo, chi;
};
__device__ __forceinline__ DescClip desc_clip(const DescJob& jb) {
  const int py0 = jb.y - DESC_R, ax0 = (jb.x - DESC_R) & ~3;
  return {max(-py0, 0), min(jb.h - 1 - py0, DESC_ROWS - 1), max(-ax0, 0), min(jb.pitch - 4 - ax0, DESC_PITCH - 4)};
}
// how a keypoint's neighbourhood lies in its level (wave-uniform): every dword inside the (zero-padded) level /
// only rows above the level missing (keypoints of the top rows: the common border case) / anything else
enum { DESC_INSIDE = 0, DESC_TOP = 1, DESC_CLIPPED = 2 };
__device__ __forceinline__ int desc_kind(const DescJob& jb) {
  const int py0 = jb.y - DESC_R, ax0 = (jb.x - DESC_R) & ~3;
  const bool below = py0 + DESC_ROWS <= jb.h, cols = ax0 >= 0 && ax0 + DESC_PITCH <= jb.pitch;
  return below && cols ? (py0 >= 0 ? DESC_INSIDE : DESC_TOP) : DESC_CLIPPED;
}

// global -> registers for a border keypoint (`base` = the neighbourhood's offset in the level, wrapped where it
// starts before the level): the same unconditional, back-to-back loads as the interior fetch, with row and dword
// column clamped into the level, so that every address stays inside [img, img + pitch * h).  What a clamped
// address delivers is overwritten with zeros in LDS (desc_zero_outside); the moments never see it, they are
// taken only where the whole orientation window is inside the level.  rowk[] never exceeds the last row of the
// neighbourhood, so for KIND == DESC_TOP the lower clamp is all there is.  RB: the constant bit rowk[] carries
// above the row (k_describe2); the clamps carry it too, and `base` is less by RB * pitch.
template <int KIND, uint32_t RB>
__device__ __forceinline__ void desc_fetch_border(const DescJob& jb, uint32_t base, const int (&rowk)[DESC_NLD],
                                                  const int (&c3)[3], uint32_t (&regs)[DESC_NLD]) {
  DescClip cl = desc_clip(jb);
  cl.rlo |= (int)RB;
  cl.rhi |= (int)RB;
  int cb[3];
#pragma unroll
  for (int m = 0; m < 3; m++) cb[m] = KIND == DESC_TOP ? 4 * c3[m] : min(max(4 * c3[m], cl.clo), cl.chi);
#pragma unroll
  for (int k = 0; k < DESC_NLD; k++) {
    const int r = KIND == DESC_TOP ? max(rowk[k], cl.rlo) : min(max(rowk[k], cl.rlo), cl.rhi);
    regs[k] = *reinterpret_cast<const uint32_t*>(
        jb.img + (base + (__umul24((uint32_t)r, (uint32_t)jb.pitch) + (uint32_t)cb[k % 3])));
  }
}

// per-wavefront LDS working set of k_describe2: its box table is written over `hs`, the patch stays intact, so
// there is no separate table (5.1 KB per wave instead of 6.1)
struct DescLds2 {
  uint32_t patch[DESC_ROWS * DESC_PITCH / 4];  // 41 x 48 u8
  uint16_t hs[DESC_ROWS * DESC_HP];            // horizontal 5-sums, then (37 rows) the 5x5 box sums
};

template <class L>
__device__ __forceinline__ void desc_store_patch(L& lds, int lane, const uint32_t (&regs)[DESC_NLD]) {
#pragma unroll
  for (int k = 0; k < DESC_NLD; k++)
    if (lane + 64 * k < DESC_ROWS * (DESC_PITCH / 4)) lds.patch[lane + 64 * k] = regs[k];
}

// After desc_store_patch of a border keypoint: the dwords of the LDS patch that lie outside the level become zero
// (a wave's LDS writes land in order, so these follow the patch without a barrier).  Whole rows above and below
// go 64 dwords at a time, the dword columns left and right one column of 41 rows at a time; every trip count is
// wave-uniform, and none of it needs the lane's patch geometry, whose registers are free again by now.  Left and
// right have to be cleared explicitly: a level whose width is a multiple of 64 has no padding, and a read past a
// row's end delivers the neighbouring row.
template <class L>
__device__ __forceinline__ void desc_zero_outside(L& lds, int lane, const DescClip& cl) {
  constexpr int RD = DESC_PITCH / 4;  // dwords per row
  for (int i = lane; i < RD * cl.rlo; i += 64) lds.patch[i] = 0;
  for (int i = RD * (cl.rhi + 1) + lane; i < RD * DESC_ROWS; i += 64) lds.patch[i] = 0;
  if (lane < DESC_ROWS) {
    for (int c = 0; c < cl.clo / 4; c++) lds.patch[lane * RD + c] = 0;
    for (int c = cl.chi / 4 + 1; c < RD; c++) lds.patch[lane * RD + c] = 0;
  }
}

// The reference skips a test unless both rotated centres lie in [2, w - 1] x [2, h - 1] (src/orb_cpu.cpp:240-245:
// the bit is then 0).  For a keypoint within 20 px of the border, after the box table is complete: every entry
// whose centre is outside that range is overwritten with DESC_TAG.  Entry (r, j) has the centre
// (x - 18 - off + j, y - 18 + r), so the entries to tag are whole rows above and below (20 dwords each, written 64
// dwords at a time) and whole columns left and right (one column of 37 rows at a time); every trip count is
// wave-uniform.  The look-ups then need no bounds test: see the signed / unsigned reads in k_describe2.
#define DESC_TAG 0x8000u
template <class L>
__device__ __forceinline__ void desc_tag_outside(L& lds, int lane, const DescJob& jb, int off) {
  constexpr int RD = DESC_HP / 2;  // dwords per table row
  const int rlo = min(max(DESC_R - jb.y, 0), DESC_BROWS), rhi = max(min(jb.h + 17 - jb.y, DESC_BROWS - 1), -1);
  const int jlo = min(max(DESC_R + off - jb.x, 0), DESC_HP), jhi = max(min(jb.w + 17 + off - jb.x, DESC_HP - 1), -1);
  uint32_t* t32 = reinterpret_cast<uint32_t*>(lds.hs);
  for (int i = lane; i < RD * rlo; i += 64) t32[i] = DESC_TAG * 0x10001u;
  for (int i = RD * (rhi + 1) + lane; i < RD * DESC_BROWS; i += 64) t32[i] = DESC_TAG * 0x10001u;
  if (lane < DESC_BROWS) {
    for (int j = 0; j < jlo; j++) lds.hs[lane * DESC_HP + j] = DESC_TAG;
    for (int j = jhi + 1; j < DESC_HP; j++) lds.hs[lane * DESC_HP + j] = DESC_TAG;
  }
  wave_lds_sync();
}

__device__ __forceinline__ DescJob desc_job(const OrbxPlan& plan, const uint8_t* pyr, int f, orbx_keypoint kp,
                                            int level) {
  const OrbxLevel& L = plan.L[level];
  DescJob jb;
  jb.img = pyr + (size_t)f * plan.frame_bytes + L.img_off;
  jb.w = L.w;
  jb.h = L.h;
  jb.pitch = L.pitch;
  jb.x = kp.x;
  jb.y = kp.y;
  jb.valid = true;
  return jb;
}

// The 5x5 box-sum table of k_describe2, horizontal and vertical pass fused: lane (chunk, g)
// walks 6 (chunk 0: 7) consecutive table rows of column group g (4 columns).  Per patch row it
// reads 8 bytes and gets the four horizontal 5-sums with one v_qsad_pk_u16_u8; the vertical sum
// is a running sum, box[r+1] = box[r] + hs[r+5] - hs[r], with the five live hs rows in
// registers.  The table (37 x DESC_HP u16) is written over lds.hs; the patch stays intact.
// LDS traffic per keypoint: 11 reads + 7 writes per lane instead of 32 accesses for two
// separate passes through an intermediate hs array.
template <class L>
__device__ __forceinline__ void desc_box_table_fused(L& lds, int lane) {
  static_assert(DESC_BROWS == 37, "6 chunks: 7 + 5 x 6 rows");
  const int chunk = lane / 10, g = lane - chunk * 10;
  if (chunk < 6) {
    const int r0 = chunk == 0 ? 0 : 6 * chunk + 1, nrows = chunk == 0 ? 7 : 6;
    const uint32_t* pp = &lds.patch[r0 * (DESC_PITCH / 4) + g];
    uint2* bp = reinterpret_cast<uint2*>(&lds.hs[r0 * DESC_HP + 4 * g]);
    auto hrow = [&](int i) {
      const u64 v = hsum5x4(pp[i * (DESC_PITCH / 4)], pp[i * (DESC_PITCH / 4) + 1]);
      return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    };
    uint2 q[5];
#pragma unroll
    for (int i = 0; i < 5; i++) q[i] = hrow(i);
    uint2 acc;
    acc.x = pk_add(pk_add(pk_add(q[0].x, q[1].x), pk_add(q[2].x, q[3].x)), q[4].x);
    acc.y = pk_add(pk_add(pk_add(q[0].y, q[1].y), pk_add(q[2].y, q[3].y)), q[4].y);
    bp[0] = acc;
#pragma unroll
    for (int i = 1; i < 7; i++) {
      if (i < nrows) {
        const uint2 nw = hrow(i + 4);
        const uint2 od = q[(i - 1) % 5];
        acc.x = pk_sub(pk_add(acc.x, nw.x), od.x);
        acc.y = pk_sub(pk_add(acc.y, nw.y), od.y);
        q[(i - 1) % 5] = nw;
        bp[i * (DESC_HP / 4)] = acc;
      }
    }
  }
  wave_lds_sync();
}

// lroundf (half away from zero) with a float result, for |v| < 2^22: trunc(v) + trunc(2 * (v - trunc(v)));
// every step is exact, so this equals orbx_lroundf
__device__ __forceinline__ float lround_f(float v) {
  const float t = __builtin_truncf(v);
  const float fr = __fsub_rn(v, t);
  return __fadd_rn(t, __builtin_truncf(__fadd_rn(fr, fr)));
}

typedef float f2_t __attribute__((ext_vector_type(2)));
typedef int i2_t __attribute__((ext_vector_type(2)));
// orbx_lround_small of both lanes (|v| < 32): v + copysign(0.5 - 2^-25, v) on the packed-f32 unit, then the
// truncating v_cvt_i32_f32
__device__ __forceinline__ i2_t lround_small2(f2_t v) {
  const f2_t h = {0.5f - 0x1p-25f, 0.5f - 0x1p-25f};
  return __builtin_convertvector(v + __builtin_elementwise_copysign(h, v), i2_t);
}

// The orientation window with a compile-time radius ORAD (rows and columns DESC_R - ORAD ... DESC_R + ORAD of the
// neighbourhood): which of a lane's DESC_NLD dwords (dword lane + 64k of the row-major 41 x 12 patch) lie in it.
// Dword k of every lane in [lane_lo(k), lane_hi(k)) is inside; an empty range is a dword no lane needs.
template <int ORAD>
struct DescWindow {
  static constexpr int RD = DESC_PITCH / 4;
  static constexpr int lo = (DESC_R - ORAD) * RD, hi = (DESC_R + ORAD + 1) * RD;  // the window's dwords [lo, hi)
  static constexpr int lane_lo(int k) { return lo - 64 * k < 0 ? 0 : lo - 64 * k > 64 ? 64 : lo - 64 * k; }
  static constexpr int lane_hi(int k) { return hi - 64 * k < 0 ? 0 : hi - 64 * k > 64 ? 64 : hi - 64 * k; }
  static constexpr bool none(int k) { return lane_lo(k) >= lane_hi(k); }
  static constexpr bool all(int k) { return lane_lo(k) == 0 && lane_hi(k) == 64; }
  static constexpr int count() {
    int n = 0;
    for (int k = 0; k < DESC_NLD; k++) n += !none(k);
    return n;
  }
};
// patch_size 31: rows 5 ... 35.  Dword 7 (rows 37 ...) is never inside, dwords 1 ... 5 always, dword 0 from its
// first dword of row 5 on and dword 6 up to its last dword of row 35.
static_assert(DescWindow<15>::none(7) && DescWindow<15>::count() == 7, "radius 15: dwords 0 ... 6");
static_assert(DescWindow<15>::all(1) && DescWindow<15>::all(2) && DescWindow<15>::all(3) && DescWindow<15>::all(4) &&
                  DescWindow<15>::all(5),
              "radius 15: dwords 1 ... 5 take no mask");
static_assert(DescWindow<15>::lane_lo(0) == (DESC_R - 15) * (DESC_PITCH / 4) && DescWindow<15>::lane_hi(0) == 64,
              "radius 15: dword 0 from the first dword of the window's first row");
static_assert(DescWindow<15>::lane_lo(6) == 0 &&
                  DescWindow<15>::lane_hi(6) == (DESC_R + 15 + 1) * (DESC_PITCH / 4) - 6 * 64,
              "radius 15: dword 6 up to the last dword of the window's last row");
// S and the row-weighted sum M in one 24-bit multiply-add chain, W = sum (row | 1 << DESC_WS) * rs = M + (S << DESC_WS):
// at most DESC_NLD dwords with rs <= 4 * 255 and rows < DESC_ROWS, so M <= 8 * 1020 * 40 = 326 400 < 2^19 and
// S <= 8160 < 2^13; W < 2^32, and both factors stay below 2^24.
#define DESC_WS 19
static_assert(DESC_NLD * 1020 * (DESC_ROWS - 1) < (1 << DESC_WS), "M fits below S in W");
static_assert((long long)DESC_NLD * 1020 < (1ll << (32 - DESC_WS)), "W fits 32 bits");
static_assert(DESC_ROWS <= (1 << DESC_WS) && DESC_WS < 23, "24-bit factors");

// ORAD: the orientation radius patch_size / 2 the kernel was compiled for (15: the window's dwords and masks are
// compile-time, see DescWindow), or 0: any patch_size, window tested at run time.
template <int DESC_KPW, int DESC_NW, int DESC_OCC, int ORAD>
__global__ __launch_bounds__(64 * DESC_NW, DESC_OCC) void k_describe2(OrbxPlan plan, const uint8_t* __restrict__ pyr, int patch_size,
                                                   const int32_t* __restrict__ sel_count,
                                                   const orbx_keypoint* __restrict__ sel_lkp,
                                                   const float* __restrict__ sel_resp,
                                                   int32_t* __restrict__ out_count,
                                                   orbx_keypoint* __restrict__ out_lkp,
                                                   float* __restrict__ out_resp,
                                                   int32_t* __restrict__ out_level,
                                                   orbx_keypoint* __restrict__ out_kp,
                                                   uint32_t* __restrict__ out_kp16,
                                                   float* __restrict__ out_angle,
                                                   orbx_descriptor* __restrict__ out_desc,
                                                   const uint32_t* __restrict__ feedback, uint32_t* __restrict__ feedback_host,
                                                   OrbxHostRecord host) {
  constexpr int DESC_KPB = DESC_NW * DESC_KPW;
  static_assert(2 * DESC_KPB <= 64 * DESC_NW, "trig: two threads per keypoint");
  __shared__ __attribute__((aligned(16))) DescLds2 s_lds[DESC_NW];
  __shared__ int s_m[DESC_KPB][2];
  __shared__ float s_cs[DESC_KPB][2];
  __shared__ uint2 s_mw[4 * (DESC_PITCH / 4)];
  // the workgroup's compact records {x | y << 16, angle, descriptor} on their way to the host (orbx_set_host_results)
  __shared__ __attribute__((aligned(16))) uint32_t s_rec_kp[DESC_KPB], s_rec_angle[DESC_KPB], s_rec_desc[DESC_KPB][8];
  // grid = (frames, keypoint groups), the frame index dispatched fastest: with 8 XCDs dealt round-robin all
  // groups of a frame gather their patches through the same L2 (2.5 % faster than (groups, frames))
  const int f = blockIdx.x, grp = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Final keypoint order = levels back to back (src/orb.cpp:100-102).  The selection
  // kernel left level l's keypoints in static slots; the prefix sums of the per-level
  // counts (lane l holds level l: one load, one DPP scan) map an output slot to them.
  static_assert(ORBX_MAX_LEVELS <= 64, "one lane per level");
  const int lvl_cnt = lane < plan.nlevels ? sel_count[f * plan.nlevels + lane] : 0;
  const int lvl_end = wave_scan_incl(lvl_cnt);  // slots of levels 0..lane
  const int count = __builtin_amdgcn_readlane(lvl_end, 63);
  if (grp == 0 && tid == 0) {
    out_count[f] = count;
    if (host.counts) host.counts[f] = count;
  }
  // (last kernel of a batch: the running totals of the top-rows-first pipeline's second pass go to the host's pinned
  // word pair, which the host reads without waiting when it enqueues later batches -- a copy node less per batch)
  // (+ the rows-needed word of every level: k_level_select above)
  // (+ the fill-row histograms: more words than the workgroup has threads)
  if (feedback_host && grp == 0 && f == 0)
    for (int i = tid; i < ORBX_FEEDBACK_WORDS; i += (int)blockDim.x) feedback_host[i] = feedback[i];
  const int slot0 = grp * DESC_KPB;
  if (slot0 >= count) return;  // whole workgroup
  DescLds2& lds = s_lds[wave];
  const int pr = ORAD != 0 ? ORAD : patch_size / 2;
  // moment weights of the four bytes of patch dword column c when the keypoint's patch starts
  // `off` bytes into its first dword: {x - x_kp + pr for bytes inside the orientation window
  // (else 0), 1 for bytes inside the window (else 0)}, for v_dot4_u32_u8
  if (tid < 4 * (DESC_PITCH / 4)) {
    const int off = tid / (DESC_PITCH / 4), c = tid - off * (DESC_PITCH / 4);
    uint32_t xw = 0, on = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int t = 4 * c + b - off - (DESC_R - pr);
      if (t >= 0 && t <= 2 * pr) {
        xw |= (uint32_t)t << (8 * b);
        on |= 1u << (8 * b);
      }
    }
    s_mw[tid] = make_uint2(xw, on);
  }
  // keypoint-independent geometry of the DESC_NLD patch dwords a lane holds: dword
  // lane + 64k is (row rowk[k], dword column (c0 + 4k) mod 12).  With a compile-time window rowk[] also carries
  // bit DESC_WS, the factor of S in the moments' multiply-add chain: the patch addresses take RB * pitch off their
  // scalar base instead (32-bit offsets wrap, and the 24-bit product keeps the bit: RB + 40 < 2^24).
  constexpr uint32_t RB = ORAD != 0 ? 1u << DESC_WS : 0u;
  int rowk[DESC_NLD], c3[3];
  uint32_t rin = 0;  // bit k: the dword exists and its row is inside the orientation window
  {
    int row = lane / (DESC_PITCH / 4), c = lane - row * (DESC_PITCH / 4);
#pragma unroll
    for (int k = 0; k < DESC_NLD; k++) {
      // (the lane dwords past the neighbourhood's end, rows 41 and 42 at k = 7, take its last row: never stored,
      // weight 0 in the moments, and a border keypoint's unconditional loads stay inside the level)
      rowk[k] = min(row, DESC_ROWS - 1) | (int)RB;
      __builtin_assume(rowk[k] >= (int)RB && rowk[k] < (int)RB + DESC_ROWS);
      if (k < 3) c3[k] = c;
      if (lane + 64 * k < DESC_ROWS * (DESC_PITCH / 4) && row >= DESC_R - pr && row <= DESC_R + pr) rin |= 1u << k;
      row += 5;
      c += 4;
      if (c >= DESC_PITCH / 4) {
        c -= DESC_PITCH / 4;
        row += 1;
      }
    }
  }
  __syncthreads();
  const size_t fo = (size_t)f * plan.out_cap;

  // this wave's keypoints; all their patches are requested before the first is used
  const int nk = min(DESC_KPW, max(0, count - (slot0 + wave * DESC_KPW)));  // wave-uniform
  DescJob jobs[DESC_KPW];
  float scale[DESC_KPW];
  uint32_t regs[DESC_KPW][DESC_NLD];
  int offs[DESC_KPW];
#pragma unroll
  for (int j = 0; j < DESC_KPW; j++) {
    const int slot = min(slot0 + wave * DESC_KPW + j, count - 1);
    // level = number of levels that end at or before the slot (count > slot, so it is < nlevels)
    const int level = __popcll(__ballot(lvl_end <= slot));
    const int lvl_begin = __builtin_amdgcn_readlane(lvl_end - lvl_cnt, level);
    const size_t src = fo + plan.L[level].out_off + (slot - lvl_begin);
    const orbx_keypoint kp = sel_lkp[src];
    jobs[j] = desc_job(plan, pyr, f, kp, level);
    scale[j] = plan.L[level].scale;
    if (j < nk && lane == 0) {  // the compacted per-keypoint records of the result block
      out_lkp[fo + slot] = kp;
      out_resp[fo + slot] = sel_resp[src];
      out_level[fo + slot] = level;
    }
  }
#pragma unroll
  for (int j = 0; j < DESC_KPW; j++) {
    const DescJob& jb = jobs[j];
    const int py0 = jb.y - DESC_R, ax0 = (jb.x - DESC_R) & ~3;
    offs[j] = jb.x - DESC_R - ax0;
    // (wraps for a neighbourhood that starts before the level; the sums below bring it back)
    const uint32_t base = (uint32_t)(py0 * jb.pitch + ax0) - RB * (uint32_t)jb.pitch;
    const int kind = desc_kind(jb);
    if (kind == DESC_INSIDE) {
#pragma unroll
      for (int k = 0; k < DESC_NLD; k++) {
        regs[j][k] = 0;
        if (lane + 64 * k < DESC_ROWS * (DESC_PITCH / 4))
          // (full-rate 24-bit multiply: rows < 41, pitch <= 16384 -- v_mul_lo_u32 is a quarter-rate instruction)
          regs[j][k] = *reinterpret_cast<const uint32_t*>(jb.img + (base + (__umul24((uint32_t)rowk[k], (uint32_t)jb.pitch) + 4u * (uint32_t)c3[k % 3])));
      }
    } else if (kind == DESC_TOP) {
      desc_fetch_border<DESC_TOP, RB>(jb, base, rowk, c3, regs[j]);
    } else {
      desc_fetch_border<DESC_CLIPPED, RB>(jb, base, rowk, c3, regs[j]);
    }
  }

  // pass A: moments.  Per keypoint, every lane's partial sums of m10 and m01 (0 where the keypoint is absent or its
  // window crosses the border); the wave sums follow for all keypoints at once
  int pm[2][DESC_KPW];
#pragma unroll
  for (int j = 0; j < DESC_KPW; j++) {
    const DescJob& jb = jobs[j];
    const int off = offs[j];
    pm[0][j] = pm[1][j] = 0;
    // full patch must lie inside the image, else angle 0 (src/orb_cpu.cpp:152-156)
    if (j < nk && !(jb.x - pr < 0 || jb.x + pr >= jb.w || jb.y - pr < 0 || jb.y + pr >= jb.h)) {
      // straight from the registers: per dword one dot product with the x weights and one
      // with the window mask; exact integers (< 2^24, like the reference's float sums)
      uint2 mw[3];
#pragma unroll
      for (int m = 0; m < 3; m++) mw[m] = s_mw[off * (DESC_PITCH / 4) + c3[m]];
      uint32_t X = 0, S = 0, M = 0;
      if constexpr (ORAD != 0) {
        // compile-time window: only the dwords some lane needs, a lane-range mask only where the range is not the
        // whole wave, and S carried above M in one multiply-add chain (bounds: DESC_WS)
        using Wn = DescWindow<ORAD>;
        uint32_t W = 0;
#pragma unroll
        for (int k = 0; k < DESC_NLD; k++) {
          if (Wn::none(k)) continue;
          const uint32_t z = Wn::all(k) || (lane >= Wn::lane_lo(k) && lane < Wn::lane_hi(k)) ? regs[j][k] : 0u;
          X = __builtin_amdgcn_udot4(z, mw[k % 3].x, X, false);
          const uint32_t rs = __builtin_amdgcn_udot4(z, mw[k % 3].y, 0u, false);
          W += __umul24((uint32_t)rowk[k], rs);  // (rowk[] carries RB)
        }
        S = W >> DESC_WS;
        M = W & ((1u << DESC_WS) - 1);
      } else {
#pragma unroll
        for (int k = 0; k < DESC_NLD; k++) {
          const uint32_t z = regs[j][k] & (uint32_t)(-(int32_t)((rin >> k) & 1u));
          X = __builtin_amdgcn_udot4(z, mw[k % 3].x, X, false);
          const uint32_t rs = __builtin_amdgcn_udot4(z, mw[k % 3].y, 0u, false);
          S += rs;
          M += __umul24((uint32_t)rowk[k], rs);  // (rows < 41, rs <= 1020: the full-rate 24-bit multiply-add)
        }
      }
      pm[0][j] = (int)X - __mul24(pr, (int)S);  // (S <= 8 x 1020, pr <= 20: 24-bit operands)
      pm[1][j] = (int)M - __mul24(DESC_R, (int)S);
    }
  }
  if constexpr (DESC_KPW == 4) {
    // the 8 wave sums as one transposed reduction: v_permlane32_swap + add leaves two of the values summed over
    // the wave's halves in one register (4 x), v_permlane16_swap + add four of them summed over 16-lane rows
    // (2 x), then one 16-lane DPP sum per register -- row r of u[i] holds moment i of keypoint kpr(r)
    int u[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const auto h0 = __builtin_amdgcn_permlane32_swap(pm[i][0], pm[i][1], false, false);  // [kp 0 | kp 1]
      const auto h1 = __builtin_amdgcn_permlane32_swap(pm[i][2], pm[i][3], false, false);  // [kp 2 | kp 3]
      const auto r = __builtin_amdgcn_permlane16_swap(h0[0] + h0[1], h1[0] + h1[1], false, false);
      u[i] = row_sum16(r[0] + r[1]);  // rows: kp 0, 2, 1, 3
    }
    if ((lane & 15) == 0) {
      const int q = wave * DESC_KPW + (((lane >> 4) & 1) << 1 | (lane >> 5));
      s_m[q][0] = u[0];
      s_m[q][1] = u[1];
    }
  } else {
#pragma unroll
    for (int j = 0; j < DESC_KPW; j++) {
      const int m10 = wave_sum(pm[0][j]), m01 = wave_sum(pm[1][j]);
      if (lane == 0) {
        s_m[wave * DESC_KPW + j][0] = m10;
        s_m[wave * DESC_KPW + j][1] = m01;
      }
    }
  }
  __syncthreads();
  // trig: TWO threads per keypoint -- both compute the angle, then the even one its cosine and the odd
  // one its sine through the shared sincosf body (one pass through its two polynomial branches
  // instead of two).  Moments are exact integers < 2^24, so the reference's float accumulation
  // equals them; atan2f(0,0) = 0 covers the border case.
  if (tid < 2 * DESC_KPB && slot0 + (tid >> 1) < count) {
    const int q = tid >> 1, want_sin = tid & 1;
    const float angle = orbx_atan2f((float)s_m[q][1], (float)s_m[q][0]);
    s_cs[q][want_sin] = orbx_sincosf_impl(angle, want_sin ^ 1);
    if (!want_sin) {
      out_angle[fo + slot0 + q] = angle;
      s_rec_angle[q] = __float_as_uint(angle);
    }
  }
  __syncthreads();

  // pass C: descriptors (the patches are still in registers).  A lane evaluates the same
  // four tests for every keypoint: its pattern points are converted to float once.
  f2_t patx[4], paty[4];  // {x1, x2}, {y1, y2} of test 64k + lane
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int32_t pk = reinterpret_cast<const int32_t*>(c_pattern)[k * 64 + lane];
    patx[k] = f2_t{(float)(int8_t)(pk & 0xff), (float)(int8_t)((pk >> 16) & 0xff)};
    paty[k] = f2_t{(float)(int8_t)((pk >> 8) & 0xff), (float)(int8_t)((pk >> 24) & 0xff)};
  }
#pragma unroll
  for (int j = 0; j < DESC_KPW; j++) {
    if (j < nk) {
      const DescJob& jb = jobs[j];
      const int q = wave * DESC_KPW + j, off = offs[j];
      // (opaque copies of the keypoint's coordinates: the border bounds are worked out again here, on the scalar
      // unit, instead of staying live in SGPRs for all four keypoints from the fetch on, which spills)
      DescJob jc = jb;
      asm("" : "+s"(jc.x), "+s"(jc.y));
      desc_store_patch(lds, lane, regs[j]);
      if (desc_kind(jc) != DESC_INSIDE) desc_zero_outside(lds, lane, desc_clip(jc));
      wave_lds_sync();
      desc_box_table_fused(lds, lane);
      const float c = s_cs[q][0], s = s_cs[q][1];
      // every rotated centre is within 18 px of the keypoint; with a 20 px margin no test can be skipped.  For any
      // other keypoint the table entries a skipped test would read are tagged (desc_tag_outside)
      const bool interior = jc.x >= DESC_R && jc.y >= DESC_R && jc.x < jc.w - DESC_R && jc.y < jc.h - DESC_R;
      if (!interior) desc_tag_outside(lds, lane, jc, off);
      u64 d[4];
      // lround as a biased add and a truncating convert (orbx_lround_small: rotated pattern coordinates stay below
      // 26), the table index as one 24-bit multiply-add, the constant part of the index in the instruction offset.
      // |dx|, |dy| <= 18 and the 37 x 40 table make every look-up memory-safe without clamps.
      const uint16_t* tbl = &lds.hs[18 * DESC_HP + 18 + off];
      // entry (x, y): the index as one v_mad_i32_i24 (40 is an inline constant), then one shift-and-add to the
      // address; the empty asm (no instruction) keeps the compiler from distributing the scaling over the
      // multiply-add, which costs a third instruction per look-up
      auto idx = [&](int x, int y) {
        int i = __mul24(y, DESC_HP) + x;
        asm("" : "+v"(i));
        return i;
      };
      // both points of a test side by side in the packed-f32 lanes (v_pk_mul/add_f32);
      // no contraction (the TU is built with -ffp-contract=off), so each product and sum
      // rounds like the reference's scalar code
      const f2_t C2 = {c, c}, S2 = {s, s};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const f2_t X = patx[k], Y = paty[k];
        const i2_t rx = lround_small2(C2 * X - S2 * Y), ry = lround_small2(S2 * X + C2 * Y);
        // the first sum read as u16, the second as i16: sums are <= 6375, so nothing changes for them, and a
        // tagged entry (0x8000) is larger than any sum in the first place and smaller in the second -- the bit
        // of a test that the reference skips comes out as 0 without a compare of its own
        const int s1 = tbl[idx(rx.x, ry.x)], s2 = reinterpret_cast<const int16_t*>(tbl)[idx(rx.y, ry.y)];
        d[k] = __ballot(s1 < s2);
      }
      wave_lds_sync();
      if (lane == 0) {  // the keypoint's record to LDS; the workgroup stores all of them at the end
        // kp.x *= scale on int (src/orb.cpp:94-98), packed as x | y << 16 (coordinates <= 16384)
        const int gx = (int)__fmul_rn((float)jb.x, scale[j]), gy = (int)__fmul_rn((float)jb.y, scale[j]);
        s_rec_kp[q] = (uint32_t)gx | ((uint32_t)gy << 16);
        u64* sd = reinterpret_cast<u64*>(s_rec_desc[q]);
        sd[0] = d[0];
        sd[1] = d[1];
        sd[2] = d[2];
        sd[3] = d[3];
      }
    }
  }
  // The records of the workgroup's keypoints leave in coalesced stores (16 x 32 B of descriptors, 16 x 8 B and
  // 16 x 4 B of keypoints): per keypoint, a lane moves the ballots of its descriptor into vector registers once.
  // With host.desc, the compact record also goes straight into the PINNED HOST mirror of the result block (the
  // descriptors, packed keypoints and angles) and travels the host link while the kernel runs -- no copy kernel
  // afterwards, no wait between two streams (orbx_set_host_results)
  __syncthreads();
  const int nq = min(DESC_KPB, count - slot0);
  if (tid < 2 * nq) {
    const uint4 v = reinterpret_cast<const uint4*>(s_rec_desc[tid >> 1])[tid & 1];
    reinterpret_cast<uint4*>(out_desc + fo + slot0)[tid] = v;
    if (host.desc) reinterpret_cast<uint4*>(host.desc + fo + slot0)[tid] = v;
  }
  if (tid < nq) {
    const uint32_t kp16 = s_rec_kp[tid];
    orbx_keypoint g;
    g.x = (int)(kp16 & 0xffffu);
    g.y = (int)(kp16 >> 16);
    out_kp[fo + slot0 + tid] = g;
    out_kp16[fo + slot0 + tid] = kp16;
    if (host.desc) {
      host.kp16[fo + slot0 + tid] = kp16;
      host.angle[fo + slot0 + tid] = __uint_as_float(s_rec_angle[tid]);
    }
  }
}

__global__ __launch_bounds__(256) void k_describe_flat(const uint8_t* __restrict__ img, int w, int h, int pitch,
                                                       const orbx_keypoint* __restrict__ kps, int nkp,
                                                       int patch_size, int use_given_angles, int do_brief,
                                                       float* __restrict__ angles,
                                                       orbx_descriptor* __restrict__ desc) {
  __shared__ __attribute__((aligned(16))) DescLds s_lds[4];
  const int wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * 4 + wave;
  DescJob jb;
  jb.valid = slot < nkp;
  jb.img = img;
  jb.w = w;
  jb.h = h;
  jb.pitch = pitch;
  jb.x = jb.valid ? kps[slot].x : 0;
  jb.y = jb.valid ? kps[slot].y : 0;
  const float given = (jb.valid && use_given_angles) ? angles[slot] : 0.0f;
  float angle;
  u64 d[4];
  describe_wave(jb, s_lds[wave], patch_size, use_given_angles != 0, given, do_brief != 0, angle, d);
  if (jb.valid && lane_id() == 0) {
    if (!use_given_angles) angles[slot] = angle;
    if (do_brief) {
      u64* dd = reinterpret_cast<u64*>(desc + slot);
      dd[0] = d[0];
      dd[1] = d[1];
      dd[2] = d[2];
      dd[3] = d[3];
    }
  }
}

// ---------------------------------------------------------------------------
// 8. Hamming 2-nearest-neighbour search over 256-bit descriptors + ratio test
//    (next row, SURVEY.md §8f rank 1: flann->knnMatch(des1, des2, matches, 2) and
//    the `m.distance < 0.8 * n.distance` filter, src/feature_matching.cpp:166-181,
//    src/feature_tracking.cpp:203-219 -- exact brute force instead of FLANN's
//    approximate LSH index).
//    One thread owns one query descriptor (4 x u64 in registers); the train set
//    streams through LDS in tiles of 256 descriptors (every lane reads the same
//    16-byte words: broadcast, conflict-free); distance = 4 x popcount(xor).
//    Ties keep the lower train index.  blockIdx.y = pair p: query set p is
//    qbase + p*qstride with qcount[p] entries, train set likewise.
__global__ __launch_bounds__(256) void k_knn2(const orbx_descriptor* __restrict__ qbase,
                                              const int32_t* __restrict__ qcount, size_t qstride,
                                              const orbx_descriptor* __restrict__ tbase,
                                              const int32_t* __restrict__ tcount, size_t tstride, double ratio,
                                              int32_t* __restrict__ knn_idx, int32_t* __restrict__ knn_dist,
                                              int32_t* __restrict__ match, size_t ostride) {
  __shared__ __attribute__((aligned(16))) uint4 s_t[256 * 2];
  const int p = blockIdx.y, tid = threadIdx.x;
  const int nq = qcount[p], nt = tcount[p];
  if ((int)(blockIdx.x * 256) >= nq) return;  // whole workgroup
  const int q = blockIdx.x * 256 + tid;
  const bool valid = q < nq;
  const uint4* qp = reinterpret_cast<const uint4*>(qbase + p * qstride + (valid ? q : 0));
  const uint4 qa = qp[0], qb = qp[1];
  const u64 q0 = ((u64)qa.y << 32) | qa.x, q1 = ((u64)qa.w << 32) | qa.z;
  const u64 q2 = ((u64)qb.y << 32) | qb.x, q3 = ((u64)qb.w << 32) | qb.z;
  int d1 = 1 << 30, d2 = 1 << 30, j1 = -1, j2 = -1;
  const orbx_descriptor* tp = tbase + p * tstride;
  for (int t0 = 0; t0 < nt; t0 += 256) {
    const int m = min(256, nt - t0);
    if (tid < m) {
      const uint4* src = reinterpret_cast<const uint4*>(tp + t0 + tid);
      s_t[2 * tid] = src[0];
      s_t[2 * tid + 1] = src[1];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < m; j++) {
      const uint4 a = s_t[2 * j], b = s_t[2 * j + 1];
      const int d = __popcll(q0 ^ (((u64)a.y << 32) | a.x)) + __popcll(q1 ^ (((u64)a.w << 32) | a.z)) +
                    __popcll(q2 ^ (((u64)b.y << 32) | b.x)) + __popcll(q3 ^ (((u64)b.w << 32) | b.z));
      if (d < d1) {
        d2 = d1;
        j2 = j1;
        d1 = d;
        j1 = t0 + j;
      } else if (d < d2) {
        d2 = d;
        j2 = t0 + j;
      }
    }
    __syncthreads();
  }
  if (valid) {
    const size_t o = p * ostride + q;
    knn_idx[2 * o] = j1;
    knn_idx[2 * o + 1] = j2;
    knn_dist[2 * o] = j1 >= 0 ? d1 : -1;
    knn_dist[2 * o + 1] = j2 >= 0 ? d2 : -1;
    // DMatch::distance is a float; the reference compares in double (0.8 is a double literal)
    const bool pass = j2 >= 0 && (double)(float)d1 < ratio * (double)(float)d2;
    match[o] = pass ? j1 : -1;
  }
}

// ---------------------------------------------------------------------------
// stage-level helpers (not on the batched hot path)

// thresholded NMS of an arbitrary float score map (src/cuda/NMS.cu:21-128):
// border of width r rejected, val > threshold, no strictly greater neighbour.
__global__ __launch_bounds__(256) void k_nms_f32(const float* __restrict__ scores, int w, int h, int r,
                                                 float threshold, u64* __restrict__ mask, int mask_wpr) {
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  bool keep = false;
  if (y < h && x < w && !(x < r || y < r || x >= w - r || y >= h - r)) {
    const float v = scores[(size_t)y * w + x];
    keep = v > threshold;
    if (keep)
      for (int dy = -r; dy <= r; dy++)
        for (int dx = -r; dx <= r; dx++) keep = keep && !(scores[(size_t)(y + dy) * w + (x + dx)] > v);
  }
  const u64 m = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && y < h) mask[(size_t)y * mask_wpr + blockIdx.x] = m;
}

// generic KxK correlation (src/cuda/Convolution.cu:20-55 arithmetic: float
// accumulate in (i,j) row-major order) with the wrapper's CV_8U conversion
// (round-half-even + saturate, :100).  reflect_pad=0: valid correlation of a
// pre-padded image; reflect_pad=1: output same size, REFLECT_101 borders
// (== copyMakeBorder + conv2d, src/GaussianBlur.cpp:44-46, src/Sobel.cpp:29-31).
__global__ __launch_bounds__(256) void k_conv2d(const uint8_t* __restrict__ img, int w, int h, int pitch,
                                                const float* __restrict__ kern, int K, int reflect_pad,
                                                uint8_t* __restrict__ dst, int dst_pitch) {
  const int wo = reflect_pad ? w : w - K + 1, ho = reflect_pad ? h : h - K + 1;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= wo || y >= ho) return;
  const int r = K / 2;
  float sum = 0.f;
  for (int i = 0; i < K; i++)
    for (int j = 0; j < K; j++) {
      int yy, xx;
      if (reflect_pad) {
        yy = reflect101(y - r + i, h);
        xx = reflect101(x - r + j, w);
      } else {
        yy = y + i;
        xx = x + j;
      }
      sum = __fadd_rn(sum, __fmul_rn((float)img[(size_t)yy * pitch + xx], kern[i * K + j]));
    }
  int v = __float2int_rn(sum);
  v = v < 0 ? 0 : (v > 255 ? 255 : v);
  dst[(size_t)y * dst_pitch + x] = (uint8_t)v;
}

// ---------------------------------------------------------------------------
// launchers

#define ORBX_LAUNCH_CHECK() hipGetLastError()

hipError_t orbx_launch_pyramid2(hipStream_t s, const OrbxTileDesc* d_tiles, int n_tiles, int frame_bytes, int w0,
                                int h0, int n_frames, const uint8_t* d_in, int in_stride, size_t in_frame_stride,
                                const OrbxResizeTap* d_taps, uint8_t* d_pyr) {
  if (n_tiles <= 0) return hipSuccess;
  dim3 grid(n_tiles | 1, n_frames);  // odd: the XCD assignment rotates from frame to frame (orbx_blur.hip)
  hipLaunchKernelGGL(k_pyramid2, grid, dim3(256), 0, s, d_tiles, n_tiles, frame_bytes, w0, h0, d_in, in_stride,
                     in_frame_stride, d_taps, d_pyr);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_blur(hipStream_t s, const OrbxPlan& plan, const OrbxTileMap& tm, int n_frames,
                            const uint8_t* d_src, uint8_t* d_dst, int first_level, int kind) {
  dim3 grid(tm.begin[plan.nlevels], n_frames);
  hipLaunchKernelGGL(k_blur, grid, dim3(256), 0, s, plan, tm, d_src, d_dst, first_level, kind);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_compact(hipStream_t s, const OrbxPlan& plan, int n_frames,
                               const unsigned long long* d_mask, orbx_keypoint* d_cand, int32_t* d_cand_count,
                               int32_t* d_cand_total, int need_total) {
  dim3 grid(plan.nlevels, n_frames);
  hipLaunchKernelGGL(k_compact, grid, dim3(256), 0, s, plan, d_mask, d_cand, d_cand_count, d_cand_total,
                     need_total);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_level_select(hipStream_t s, const OrbxPlan& plan, int n_frames, int mode,
                                    const unsigned long long* d_mask, const uint8_t* d_pyr, const float* d_gauss,
                                    int window, float k, orbx_keypoint* d_sel_lkp, float* d_sel_resp,
                                    int32_t* d_sel_count, uint32_t* d_need) {
  // the row-major mode writes its survivors straight to the output slots and needs no LDS
  const int nslots = mode == ORBX_SELECT_ROWMAJOR ? 0 : lvl_slots(plan, plan.nlevels);
  if (nslots > LVL_MAX_SLOTS) return hipErrorInvalidValue;
  const size_t lds = (size_t)nslots * 16;
  // A workgroup per frame and all of its levels from 256 frames (one per CU) on; below that, a workgroup per (level,
  // frame): a few frames' runs queued over one workgroup's 8 waves leave most CUs idle.  Measured: 256 frames per
  // step 545 k frames/s per frame vs 502 k per (level, frame); one frame end to end 0.196 vs 0.160 ms
  const int lpg = n_frames >= 256 ? plan.nlevels : 1;
  dim3 grid(n_frames, (plan.nlevels + lpg - 1) / lpg);
  auto kern = window == 7 ? k_level_select<7> : window == 5 ? k_level_select<5> : window == 3 ? k_level_select<3>
                                                                                   : k_level_select<0>;
  hipLaunchKernelGGL(kern, grid, dim3(LVL_THREADS), lds, s, plan, lpg, mode, d_mask, d_pyr, d_gauss, window, k, d_sel_lkp,
                     d_sel_resp, d_sel_count, d_need);
  return ORBX_LAUNCH_CHECK();
}

// one workgroup per frame or the three spread kernels, whichever suits the shape
// (see 6c); force = 0 fused, 1 spread, -1 automatic
hipError_t orbx_launch_level_select_auto(hipStream_t s, const OrbxPlan& plan, int n_frames, int mode, int force,
                                         const unsigned long long* d_mask, const uint8_t* d_pyr,
                                         const float* d_gauss, int window, float k, uint32_t* d_cand,
                                         int32_t* d_ncand, float* d_cresp, orbx_keypoint* d_sel_lkp,
                                         float* d_sel_resp, int32_t* d_sel_count, uint32_t* d_need) {
  int maxcap = 2;
  for (int l = 0; l < plan.nlevels; l++) maxcap = plan.L[l].cap > maxcap ? plan.L[l].cap : maxcap;
  // the fused kernel holds a frame's candidates in LDS; the spread kernels take larger frames whatever `force` says
  const bool spread = mode == ORBX_SELECT_HARRIS &&
                      (lvl_slots(plan, plan.nlevels) > LVL_MAX_SLOTS ||
                       (force >= 0 ? force != 0 : maxcap > LVL_THREADS));  // more than one candidate per thread
  if (!spread)
    return orbx_launch_level_select(s, plan, n_frames, mode, d_mask, d_pyr, d_gauss, window, k, d_sel_lkp,
                                    d_sel_resp, d_sel_count, d_need);
  hipLaunchKernelGGL(k_lvl_compact, dim3(plan.nlevels, n_frames), dim3(256), 0, s, plan, d_mask, d_cand, d_ncand, d_need);
  hipLaunchKernelGGL(k_lvl_harris, dim3((maxcap + 255) / 256, plan.nlevels, n_frames), dim3(256), 0, s, plan, d_pyr,
                     d_gauss, window, k, d_cand, d_ncand, d_cresp);
  const size_t lds = (size_t)((maxcap + 7) & ~7) * 8;
  hipLaunchKernelGGL(k_lvl_rank, dim3((maxcap + RANK_SLICE - 1) / RANK_SLICE, plan.nlevels, n_frames), dim3(256), lds,
                     s, plan, d_cand, d_ncand, d_cresp, d_sel_lkp, d_sel_resp, d_sel_count);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_describe(hipStream_t s, const OrbxPlan& plan, int n_frames, const uint8_t* d_pyr,
                                int patch_size, const int32_t* d_sel_count, const orbx_keypoint* d_sel_lkp,
                                const float* d_sel_resp, int32_t* d_out_count, orbx_keypoint* d_out_lkp,
                                float* d_out_resp, int32_t* d_out_level, orbx_keypoint* d_out_kp, uint32_t* d_out_kp16,
                                float* d_out_angle, orbx_descriptor* d_out_desc, const uint32_t* d_feedback,
                                uint32_t* h_feedback, const OrbxHostRecord* host_record) {
  const OrbxHostRecord host = host_record ? *host_record : OrbxHostRecord{};
  if (plan.out_cap <= 0) return hipSuccess;
  // few keypoints in flight (single frames, small batches): one keypoint per wave, four times the
  // workgroups, a quarter of the serial work per wave; else four per wave
  // patch_size 31 (the default) runs the kernels compiled for its orientation window, every other size the
  // run-time window
  const bool win31 = patch_size == 31;
  if ((long long)plan.out_cap * n_frames <= 8192) {
    dim3 grid(n_frames, (plan.out_cap + 3) / 4);
    hipLaunchKernelGGL((win31 ? k_describe2<1, 4, 1, 15> : k_describe2<1, 4, 1, 0>), grid, dim3(256), 0, s, plan, d_pyr, patch_size, d_sel_count, d_sel_lkp,
                       d_sel_resp, d_out_count, d_out_lkp, d_out_resp, d_out_level, d_out_kp, d_out_kp16, d_out_angle, d_out_desc, d_feedback,
                       h_feedback, host);
  } else {
    // Four waves of four keypoints, registers capped for 6 waves per SIMD: 78 VGPRs, no scratch.  The 72-register
    // cap of 7 waves per SIMD spills 7 VGPRs + 7 SGPRs (32 B/lane of scratch) and is 4 % slower per 1024 frames
    // (867 vs 831 us).  Earlier, per 256 frames: 8-wave workgroups at 6 waves per SIMD (the trig -- two threads per
    // keypoint -- fills a wave: -1.8 % instructions) 203 us, 7-wave workgroups 221 us.
    dim3 grid(n_frames, (plan.out_cap + 15) / 16);
    hipLaunchKernelGGL((win31 ? k_describe2<4, 4, 6, 15> : k_describe2<4, 4, 6, 0>), grid, dim3(256), 0, s, plan, d_pyr, patch_size, d_sel_count, d_sel_lkp,
                       d_sel_resp, d_out_count, d_out_lkp, d_out_resp, d_out_level, d_out_kp, d_out_kp16, d_out_angle, d_out_desc, d_feedback,
                       h_feedback, host);
  }
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_describe_flat(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch,
                                     const orbx_keypoint* d_kps, int nkp, int patch_size, int use_given_angles,
                                     int do_brief, float* d_angles, orbx_descriptor* d_desc) {
  if (nkp <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_describe_flat, dim3((nkp + 3) / 4), dim3(256), 0, s, d_img, w, h, pitch, d_kps, nkp,
                     patch_size, use_given_angles, do_brief, d_angles, d_desc);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_harris_flat(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch,
                                   const orbx_keypoint* d_kps, int nkp, const float* d_gauss, int K, float kk,
                                   float* d_resp) {
  if (nkp <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_harris2_flat, dim3((nkp + 31) / 32), dim3(256), 0, s, d_img, w, h, pitch, d_kps, nkp,
                     d_gauss, K, kk, d_resp);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_nms_f32(hipStream_t s, const float* d_scores, int w, int h, int radius, float threshold,
                               unsigned long long* d_mask, int mask_wpr) {
  dim3 grid((w + 63) / 64, (h + 3) / 4);
  hipLaunchKernelGGL(k_nms_f32, grid, dim3(256), 0, s, d_scores, w, h, radius, threshold, d_mask, mask_wpr);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_conv2d(hipStream_t s, const uint8_t* d_img, int w, int h, int pitch, const float* d_kernel,
                              int K, int reflect_pad, uint8_t* d_dst, int dst_pitch) {
  const int wo = reflect_pad ? w : w - K + 1, ho = reflect_pad ? h : h - K + 1;
  if (wo <= 0 || ho <= 0) return hipSuccess;
  dim3 grid((wo + 63) / 64, (ho + 3) / 4);
  hipLaunchKernelGGL(k_conv2d, grid, dim3(256), 0, s, d_img, w, h, pitch, d_kernel, K, reflect_pad, d_dst,
                     dst_pitch);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_select_flat(hipStream_t s, const float* d_resp, int n, int keep, int32_t* d_idx) {
  if (n <= 0) return hipSuccess;
  int blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_select_flat, dim3(blocks), dim3(256), 0, s, d_resp, n, keep, d_idx);
  return ORBX_LAUNCH_CHECK();
}

hipError_t orbx_launch_knn2(hipStream_t s, int npairs, int max_nq, const orbx_descriptor* d_q, const int32_t* d_qcount,
                            size_t qstride, const orbx_descriptor* d_t, const int32_t* d_tcount, size_t tstride,
                            double ratio, int32_t* d_idx, int32_t* d_dist, int32_t* d_match, size_t ostride) {
  if (npairs <= 0 || max_nq <= 0) return hipSuccess;
  dim3 grid((max_nq + 255) / 256, npairs);
  hipLaunchKernelGGL(k_knn2, grid, dim3(256), 0, s, d_q, d_qcount, qstride, d_t, d_tcount, tstride, ratio, d_idx,
                     d_dist, d_match, ostride);
  return ORBX_LAUNCH_CHECK();
}
