// orbx_reloc.hip -- gfx950 kernels behind include/orbx_reloc.h: ORB descriptors at points the
// caller holds, and two described point sets joined by descriptor into an `origin` block.
//   k_pd_level0    the level-0 image a keypoint of the ORB path is described on (copy, or the 5x5 blur of either kind),
//                  from the caller's frames into the workspace with a pitch that is a multiple of 4
//   k_pd_classify  rules A-C per slot, the zeros of every slot that is not OK, and the frame's OK slots compacted in
//                  slot order (ballot and prefix, as k_gftt_seeds orders its seeds)
//   k_pd_describe  one wave per OK slot with describe_wave (orbx_describe.h), four per workgroup
//   k_ra_knn2      rules F-H: one lane per query slot, the train set streaming through LDS in tiles of 256
//   k_ra_unique    rules I-J: one workgroup per window
// Why the live slots are compacted first: describe_wave meets its workgroup at barriers, so the wave of a dead slot
// cannot leave on its own; with the list a workgroup holds four OK slots or none, and one without any exits on a
// scalar load before the patch fetch.  Nothing here writes a result through an atomic.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_math.h"
#include "orbx_wave.h"

static __constant__ __attribute__((aligned(16))) int8_t c_pattern[1024] = {
#include "pattern_31.inc"
};

#include "orbx_describe.h"

static_assert(PD_R_MIN == DESC_R, "rule C's 20 is the reach describe_wave's patch covers");

// BORDER_REFLECT_101 for p in [-len + 1, 2 * len - 2], clamped otherwise (src/cuda/GaussianBlur1D.cu:27-32)
__device__ __forceinline__ int pd_reflect101(int p, int len) {
  if (p < 0) p = -p;
  if (p >= len) p = 2 * len - p - 2;
  p = p < 0 ? 0 : p;
  return p >= len ? len - 1 : p;
}

// ---- the level-0 image ----------------------------------------------------------------------------------------------
// A workgroup owns PD_TW x PD_TH pixels of one frame: the tile with its halo of 2 goes through LDS (reflected at the
// frame's borders), then every lane writes four pixels as one dword; the bytes from `w` to the pitch are zeros.  The
// arithmetic is k_blur's: integers, rne(S / 256) for the separable kernel and the nearest integer to S / 273 for the
// 5x5 one (src/cuda/GaussianBlur1D.cu:34-163, src/cuda/GaussianBlur.cu:21-130).
#define PD_TW 64
#define PD_TH 16
#define PD_SROWS (PD_TH + 4)
#define PD_SPITCH (PD_TW + 4)

__global__ __launch_bounds__(256) void k_pd_level0(const uint8_t* __restrict__ frames, int w, int h, int row_stride,
                                                   size_t frame_stride, int kind, uint8_t* __restrict__ dst, int pitch,
                                                   size_t dst_stride) {
  __shared__ uint8_t s_src[PD_SROWS * PD_SPITCH];
  __shared__ uint16_t s_h[PD_SROWS * PD_TW];
  const int f = blockIdx.z, tid = threadIdx.x;
  const uint8_t* img = frames + (size_t)f * frame_stride;
  uint8_t* out = dst + (size_t)f * dst_stride;
  const int x0 = blockIdx.x * PD_TW, y0 = blockIdx.y * PD_TH;
  const int c4 = (tid & 15) * 4, r = tid >> 4;
  const int gx = x0 + c4, gy = y0 + r;
  uint32_t packed = 0;
  if (kind == PD_LEVEL0_COPY) {
    if (gy < h) {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (gx + k < w) packed |= (uint32_t)img[(size_t)gy * row_stride + gx + k] << (8 * k);
    }
  } else {
    for (int i = tid; i < PD_SROWS * PD_SPITCH; i += 256) {
      const int row = i / PD_SPITCH, c = i - row * PD_SPITCH;
      const int sy = pd_reflect101(y0 - 2 + row, h), sx = pd_reflect101(x0 - 2 + c, w);
      s_src[i] = img[(size_t)sy * row_stride + sx];
    }
    __syncthreads();
    if (kind == ORBX_BLUR_SEP16) {
      for (int i = tid; i < PD_SROWS * PD_TW; i += 256) {
        const int row = i >> 6, c = i & 63;
        const uint8_t* p = s_src + row * PD_SPITCH + c;  // p[0] is x - 2
        s_h[i] = (uint16_t)(p[0] + 4 * p[1] + 6 * p[2] + 4 * p[3] + p[4]);
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint16_t* hp = s_h + r * PD_TW + c4 + k;  // hp[0] is y - 2
        const uint32_t S = hp[0] + 4u * hp[PD_TW] + 6u * hp[2 * PD_TW] + 4u * hp[3 * PD_TW] + hp[4 * PD_TW];
        const uint32_t v = (S + 127u + ((S >> 8) & 1u)) >> 8;  // round-half-even of S / 256
        if (gx + k < w) packed |= v << (8 * k);
      }
    } else {
      const int kw[25] = {1, 4, 7, 4, 1, 4, 16, 26, 16, 4, 7, 26, 41, 26, 7, 4, 16, 26, 16, 4, 1, 4, 7, 4, 1};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint32_t S = 0;
#pragma unroll
        for (int i = 0; i < 5; i++)
#pragma unroll
          for (int j = 0; j < 5; j++) S += (uint32_t)kw[i * 5 + j] * s_src[(r + i) * PD_SPITCH + c4 + k + j];
        const uint32_t v = (2u * S + 273u) / 546u;  // nearest integer to S / 273 (273 is odd: no ties)
        if (gx + k < w) packed |= v << (8 * k);
      }
    }
  }
  if (gy < h && gx < pitch) *reinterpret_cast<uint32_t*>(out + (size_t)gy * pitch + gx) = packed;
}

// ---- rules A-C ------------------------------------------------------------------------------------------------------
// rule A's usable test and rule B's pixel of a point; the state by rule C.  (A NaN fails every compare; an infinity
// fails one of the bounds.)
__device__ __forceinline__ int pd_state_of(float x, float y, int w, int h, int R, int& X, int& Y) {
  X = 0;
  Y = 0;
  if (!(x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1))) return PD_NONE;
  X = (int)rintf(x);
  Y = (int)rintf(y);
  return (X >= R && X <= w - 1 - R && Y >= R && Y <= h - 1 - R) ? PD_OK : PD_BORDER;
}

#define PD_THREADS 256
// One workgroup per frame walks the slots in chunks of its size.  state of every slot, zeros in angle and desc of
// every slot that is not OK (k_pd_describe writes the OK ones), the OK slots in slot order in list[f][0 .. n_ok[f]).
__global__ __launch_bounds__(PD_THREADS) void k_pd_classify(const float* __restrict__ xy, size_t point_stride,
                                                            size_t xy_frame_stride, const int32_t* __restrict__ seen,
                                                            int seen_min, const int32_t* __restrict__ counts, int cap,
                                                            int w, int h, int R, int32_t* __restrict__ state,
                                                            float* __restrict__ angle, uint4* __restrict__ desc,
                                                            int32_t* __restrict__ n_ok, int32_t* __restrict__ list) {
  __shared__ int s_wave[PD_THREADS / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  const float* pf = xy + (size_t)f * xy_frame_stride;
  const int live_end = counts ? min(max(counts[f], 0), cap) : cap;
  const size_t row = (size_t)f * cap;
  int base = 0;
  for (int s0 = 0; s0 < cap; s0 += PD_THREADS) {
    const int s = s0 + tid;
    int st = PD_NONE;
    if (s < live_end && (seen == nullptr || seen[row + s] >= seen_min)) {
      int X, Y;
      st = pd_state_of(pf[(size_t)s * point_stride], pf[(size_t)s * point_stride + 1], w, h, R, X, Y);
    }
    int total;
    const int at = base + block_scan_excl<PD_THREADS>(st == PD_OK ? 1 : 0, s_wave, &total);
    if (s < cap) {
      state[row + s] = st;
      if (st == PD_OK) {
        list[row + at] = s;
      } else {
        angle[row + s] = 0.f;
        desc[2 * (row + s)] = make_uint4(0, 0, 0, 0);
        desc[2 * (row + s) + 1] = make_uint4(0, 0, 0, 0);
      }
    }
    base += total;
  }
  if (tid == 0) n_ok[f] = base;
}

// ---- rules D-E ------------------------------------------------------------------------------------------------------
// grid (ceil(cap / 4), frames): wave k of frame f describes the k-th OK slot of the frame; a workgroup whose four are
// all beyond n_ok[f] leaves at once (the test is uniform over the workgroup, so no wave waits at a barrier alone).
__global__ __launch_bounds__(256) void k_pd_describe(const uint8_t* __restrict__ level0, int w, int h, int pitch,
                                                     size_t img_stride, const float* __restrict__ xy,
                                                     size_t point_stride, size_t xy_frame_stride, int cap,
                                                     int patch_size, const int32_t* __restrict__ n_ok,
                                                     const int32_t* __restrict__ list, float* __restrict__ angle,
                                                     orbx_descriptor* __restrict__ desc) {
  __shared__ __attribute__((aligned(16))) DescLds s_lds[4];
  const int f = blockIdx.y, wave = threadIdx.x >> 6;
  const int count = n_ok[f];
  if ((int)(blockIdx.x * 4) >= count) return;  // whole workgroup
  const int k = blockIdx.x * 4 + wave;
  const size_t row = (size_t)f * cap;
  DescJob jb;
  jb.valid = k < count;
  jb.img = level0 + (size_t)f * img_stride;
  jb.w = w;
  jb.h = h;
  jb.pitch = pitch;
  int slot = 0;
  jb.x = 0;
  jb.y = 0;
  if (jb.valid) {
    slot = list[row + k];
    const float* p = xy + (size_t)f * xy_frame_stride + (size_t)slot * point_stride;
    jb.x = (int)rintf(p[0]);
    jb.y = (int)rintf(p[1]);
    // (rule C held when the slot entered the list; the clamp keeps the patch fetch inside the frame whatever a
    // caller does to the points while the call runs)
    jb.x = min(max(jb.x, 0), w - 1);
    jb.y = min(max(jb.y, 0), h - 1);
  }
  float a;
  u64 d[4];
  describe_wave(jb, s_lds[wave], patch_size, false, 0.0f, true, a, d);
  if (jb.valid && lane_id() == 0) {
    angle[row + slot] = a;
    u64* dd = reinterpret_cast<u64*>(desc + row + slot);
    dd[0] = d[0];
    dd[1] = d[1];
    dd[2] = d[2];
    dd[3] = d[3];
  }
}

// ---- rules F-H ------------------------------------------------------------------------------------------------------
// One lane owns one query slot (4 x u64 in registers); the train set streams through LDS in tiles of 256 with its
// states (every lane reads the same words: broadcast); a train slot that is not OK is passed over by every lane at
// once.  Ties keep the lower train slot.  With `unique`, an accepted query also lowers best[w][train slot] to its key
// (d1 << 22 | q): an integer minimum, which does not depend on the order of its operands.
#define RA_KEY_SHIFT 22
__global__ __launch_bounds__(256) void k_ra_knn2(const orbx_descriptor* __restrict__ qdesc,
                                                 const int32_t* __restrict__ qstate, int qcap,
                                                 const orbx_descriptor* __restrict__ tdesc,
                                                 const int32_t* __restrict__ tstate, int tcap, double ratio,
                                                 int max_distance, int unique, int32_t* __restrict__ origin,
                                                 int32_t* __restrict__ dist, uint32_t* __restrict__ best) {
  __shared__ __attribute__((aligned(16))) uint4 s_t[256 * 2];
  __shared__ int32_t s_ok[256];
  const int w = blockIdx.y, tid = threadIdx.x;
  const int q = blockIdx.x * 256 + tid;
  const bool valid = q < qcap;
  const size_t qrow = (size_t)w * qcap, trow = (size_t)w * tcap;
  const bool q_ok = valid && qstate[qrow + q] == PD_OK;
  const uint4* qp = reinterpret_cast<const uint4*>(qdesc + qrow + (valid ? q : 0));
  const uint4 qa = qp[0], qb = qp[1];
  const u64 q0 = ((u64)qa.y << 32) | qa.x, q1 = ((u64)qa.w << 32) | qa.z;
  const u64 q2 = ((u64)qb.y << 32) | qb.x, q3 = ((u64)qb.w << 32) | qb.z;
  int d1 = 1 << 30, d2 = 1 << 30, j1 = -1, j2 = -1;
  for (int t0 = 0; t0 < tcap; t0 += 256) {
    const int m = min(256, tcap - t0);
    if (tid < m) {
      const uint4* src = reinterpret_cast<const uint4*>(tdesc + trow + t0 + tid);
      s_t[2 * tid] = src[0];
      s_t[2 * tid + 1] = src[1];
      s_ok[tid] = tstate[trow + t0 + tid] == PD_OK;
    }
    __syncthreads();
    for (int j = 0; j < m; j++) {
      if (!s_ok[j]) continue;  // (uniform)
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
    // DMatch::distance is a float; the reference compares in double (0.8 is a double literal)
    const bool pass = q_ok && j2 >= 0 && (double)(float)d1 < ratio * (double)(float)d2 && d1 <= max_distance;
    origin[qrow + q] = pass ? j1 : -1;
    dist[qrow + q] = pass ? d1 : -1;
    if (pass && unique) atomicMin(best + trow + j1, ((uint32_t)d1 << RA_KEY_SHIFT) | (uint32_t)q);
  }
}

// One workgroup per window: with `unique`, a query whose key is not its train slot's minimum is rejected; count[w] by
// a prefix over the workgroup, chunk after chunk.
__global__ __launch_bounds__(PD_THREADS) void k_ra_unique(int qcap, int tcap, int unique,
                                                          const uint32_t* __restrict__ best,
                                                          int32_t* __restrict__ origin, int32_t* __restrict__ dist,
                                                          int32_t* __restrict__ count) {
  __shared__ int s_wave[PD_THREADS / 64];
  const int w = blockIdx.x, tid = threadIdx.x;
  const size_t qrow = (size_t)w * qcap, trow = (size_t)w * tcap;
  int base = 0;
  for (int q0 = 0; q0 < qcap; q0 += PD_THREADS) {
    const int q = q0 + tid;
    int keep = 0;
    if (q < qcap) {
      const int j = origin[qrow + q];
      if (j >= 0) {
        keep = 1;
        if (unique && best[trow + j] != (((uint32_t)dist[qrow + q] << RA_KEY_SHIFT) | (uint32_t)q)) {
          keep = 0;
          origin[qrow + q] = -1;
          dist[qrow + q] = -1;
        }
      }
    }
    int total;
    (void)block_scan_excl<PD_THREADS>(keep, s_wave, &total);
    base += total;
  }
  if (tid == 0) count[w] = base;
}

// ---- launchers --------------------------------------------------------------------------------------------------------
hipError_t orbx_launch_pd_level0(hipStream_t s, const uint8_t* d_frames, int n, int w, int h, int row_stride,
                                 size_t frame_stride, int kind, uint8_t* d_level0, int pitch, size_t img_stride) {
  const dim3 grid((pitch + PD_TW - 1) / PD_TW, (h + PD_TH - 1) / PD_TH, n);
  hipLaunchKernelGGL(k_pd_level0, grid, dim3(256), 0, s, d_frames, w, h, row_stride, frame_stride, kind, d_level0,
                     pitch, img_stride);
  return hipGetLastError();
}

hipError_t orbx_launch_pd_describe(hipStream_t s, const uint8_t* d_level0, int n, int w, int h, int pitch,
                                   size_t img_stride, const float* d_xy, size_t point_stride, size_t xy_frame_stride,
                                   const int32_t* d_seen, int seen_min, const int32_t* d_counts, int cap, int patch_size,
                                   int32_t* d_state, float* d_angle, orbx_descriptor* d_desc, int32_t* d_n_ok,
                                   int32_t* d_list) {
  const int R = patch_size / 2 > PD_R_MIN ? patch_size / 2 : PD_R_MIN;
  hipLaunchKernelGGL(k_pd_classify, dim3(n), dim3(PD_THREADS), 0, s, d_xy, point_stride, xy_frame_stride, d_seen,
                     seen_min, d_counts, cap, w, h, R, d_state, d_angle, reinterpret_cast<uint4*>(d_desc), d_n_ok,
                     d_list);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pd_describe, dim3((cap + 3) / 4, n), dim3(256), 0, s, d_level0, w, h, pitch, img_stride, d_xy,
                     point_stride, xy_frame_stride, cap, patch_size, d_n_ok, d_list, d_angle, d_desc);
  return hipGetLastError();
}

hipError_t orbx_launch_reassociate(hipStream_t s, int n_windows, const orbx_descriptor* d_qdesc,
                                   const int32_t* d_qstate, int qcap, const orbx_descriptor* d_tdesc,
                                   const int32_t* d_tstate, int tcap, double ratio, int max_distance, int unique,
                                   uint32_t* d_best, int32_t* d_origin, int32_t* d_dist, int32_t* d_count) {
  if (unique) {
    const hipError_t e = hipMemsetAsync(d_best, 0xff, sizeof(uint32_t) * (size_t)n_windows * tcap, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_ra_knn2, dim3((qcap + 255) / 256, n_windows), dim3(256), 0, s, d_qdesc, d_qstate, qcap, d_tdesc,
                     d_tstate, tcap, ratio, max_distance, unique, d_origin, d_dist, d_best);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ra_unique, dim3(n_windows), dim3(PD_THREADS), 0, s, qcap, tcap, unique, d_best, d_origin,
                     d_dist, d_count);
  return hipGetLastError();
}

hipError_t orbx_launch_ra_unique(hipStream_t s, int n_windows, int qcap, int tcap, int unique, const uint32_t* d_best,
                                 int32_t* d_origin, int32_t* d_dist, int32_t* d_count) {
  hipLaunchKernelGGL(k_ra_unique, dim3(n_windows), dim3(PD_THREADS), 0, s, qcap, tcap, unique, d_best, d_origin,
                     d_dist, d_count);
  return hipGetLastError();
}
