// orbx_search.hip -- gfx950 kernels behind include/orbx_search.h: the landmarks of the current
// block projected into a predicted view, and the re-association of two described sets inside a position gate.  The
// reference keeps no point across a solve (src/with_bundle_adjustment.cpp:586-593) and matches two ORB sets without
// geometry (src/feature_tracking.cpp:203-219).
//   k_sp_project  rules P1-P5: one lane per (window, landmark) scatters to the landmark's slot (a window's slots
//                 ascend: no two lanes write one slot); every other slot keeps the zeros the launcher wrote
//   k_sp_count    one wave per window: count[w] = the slots that are SP_OK, by ballot and popcount
//   k_sg_bin      one workgroup per window: the grid of the window from the bounding box of its positioned OK queries,
//                 then a counting sort of the positioned OK train slots by cell (histogram and prefix in LDS) into the
//                 window's sorted list -- slot, position and descriptor side by side -- with the cell starts
//   k_sg_knn2     rules K-N: one lane per query slot walks the cells its circle touches; cells of one grid row are
//                 neighbours in the list, so a query reads one run of the list per grid row
// The grid decides which pairs are LOOKED AT; whether a pair is a candidate is sp_in_gate's test alone (rule L), and the
// two best candidates are minima of integer keys (rule M), so no result depends on the grid or on the order in which
// the LDS atomics of the sort placed the slots of a cell.  No result is written through an atomic but `best`.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_lm_math.h"  // LM_OK
#include "orbx_search_math.h"
#include "orbx_wave.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SG_THREADS = 256;
constexpr int SG_KEY_SHIFT = 22;  // = k_ra_knn2's and k_ra_unique's key layout: d << 22 | slot

// ---- rules P1-P5 ----------------------------------------------------------------------------------------------------
// grid: `blocks` workgroups of SP_THREADS landmarks per window
__global__ __launch_bounds__(SP_THREADS) void k_sp_project(const OrbxCarryIn in, int cap, int blocks,
                                                            const double* __restrict__ pose6, size_t pose_stride,
                                                            double fx, double fy, double cx, double cy, int width,
                                                            int height, double margin_px, double* __restrict__ xy,
                                                            double* __restrict__ depth, int32_t* __restrict__ state) {
  const int w = blockIdx.x / blocks;
  const int j = (blockIdx.x % blocks) * SP_THREADS + threadIdx.x;
  if (in.status[w] != LM_OK) return;
  const int p0 = in.pt_off[w], np = in.pt_off[w + 1] - p0;
  if (j >= np) return;
  const int s = in.slot[p0 + j];
  if (s < 0 || s >= cap || s >= in.old_cap) return;  // (a landmark's slot always is inside: a damaged block writes nowhere)
  // rule A of the carry joins origin t to the FIRST landmark of slot t
  if (j > 0 && in.slot[p0 + j - 1] == s) return;
  const double* src = in.src + 3 * ((size_t)p0 + j);
  const double X[3] = {src[0], src[1], src[2]};
  if (!(wp_finite(X[0]) && wp_finite(X[1]) && wp_finite(X[2]))) return;
  double P[6], M[PNP_MODEL_DOUBLES];
  const double* pp = pose6 + (size_t)w * pose_stride;
#pragma unroll
  for (int i = 0; i < 6; i++) P[i] = pp[i];
  if (!sp_pose_model(P, M)) return;  // rule P2: the whole window stays SP_NONE
  const double K4[4] = {fx, fy, cx, cy};
  double out[3];
  const int st = sp_project(K4, M, X, width, height, margin_px, out);
  const size_t at = (size_t)w * cap + s;
  state[at] = st;
  if (st == SP_OK) xy[2 * at] = out[0], xy[2 * at + 1] = out[1], depth[at] = out[2];
}

__global__ __launch_bounds__(64) void k_sp_count(const int32_t* __restrict__ state, int cap,
                                                  int32_t* __restrict__ count) {
  const int w = blockIdx.x;
  const int32_t* S = state + (size_t)w * cap;
  int c = 0;
  for (int base = 0; base < cap; base += 64) {  // (uniform trip count: every lane reaches the ballot)
    const int s = base + (int)threadIdx.x;
    c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(s < cap && S[s] == SP_OK));
  }
  if (threadIdx.x == 0) count[w] = c;
}

// ---- the grid ---------------------------------------------------------------------------------------------------------
// cell of coordinate v on an axis of n cells of side 1 / inv that starts at o: monotone in v, clamped into [0, n)
__device__ __forceinline__ int sg_cell(double v, double o, double inv, int n) {
  const double c = floor((v - o) * inv);
  return c >= (double)(n - 1) ? n - 1 : (c > 0.0 ? (int)c : 0);
}

__device__ __forceinline__ bool sg_train_in(const int32_t* tstate, const int32_t* tpstate, const double* txy, size_t at,
                                            double& x, double& y) {
  if (tstate[at] != PD_OK || (tpstate && tpstate[at] != SP_OK)) return false;
  x = txy[2 * at], y = txy[2 * at + 1];
  return wp_finite(x) && wp_finite(y);
}

__device__ __forceinline__ bool finite_f(float v) {
  return (__builtin_bit_cast(unsigned int, v) & 0x7f800000u) != 0x7f800000u;
}

// One workgroup per window.  The grid: the bounding box of the positioned OK queries, grown by the radius; square
// cells of side max(radius, sqrt(area / (ORBX_SG_CELLS_MAX / 2))), at most ORBX_SG_CELLS_MAX of them.  Train slots
// beyond the box land in its border cells.  sorted: per window, n_in records in cell order.
__global__ __launch_bounds__(SG_THREADS) void k_sg_bin(const int32_t* __restrict__ qstate,
                                                        const float* __restrict__ qxy, size_t point_stride,
                                                        size_t xy_frame_stride, int qcap,
                                                        const orbx_descriptor* __restrict__ tdesc,
                                                        const int32_t* __restrict__ tstate,
                                                        const double* __restrict__ txy,
                                                        const int32_t* __restrict__ tpstate, int tcap, double radius,
                                                        OrbxSgGrid* __restrict__ grids, int32_t* __restrict__ starts,
                                                        int32_t* __restrict__ sslot, double* __restrict__ sxy,
                                                        uint4* __restrict__ sdesc) {
  __shared__ int s_cnt[ORBX_SG_CELLS_MAX];
  __shared__ int s_wave[SG_THREADS / 64];
  __shared__ double s_box[4][SG_THREADS / 64];
  __shared__ OrbxSgGrid s_grid;
  const int w = blockIdx.x, tid = threadIdx.x;
  const size_t qrow = (size_t)w * qcap, trow = (size_t)w * tcap;
  const float* qf = qxy + (size_t)w * xy_frame_stride;
  // (a) the queries' box, as maxima of x, -x, y, -y
  const double ninf = -__builtin_huge_val();
  double b[4] = {ninf, ninf, ninf, ninf};
  for (int q = tid; q < qcap; q += SG_THREADS) {
    if (qstate[qrow + q] != PD_OK) continue;
    const float x = qf[(size_t)q * point_stride], y = qf[(size_t)q * point_stride + 1];
    if (!finite_f(x) || !finite_f(y)) continue;
    b[0] = fmax(b[0], (double)x), b[1] = fmax(b[1], -(double)x);
    b[2] = fmax(b[2], (double)y), b[3] = fmax(b[3], -(double)y);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const double m = wave_max_f64(b[i]);
    if ((tid & 63) == 0) s_box[i][tid >> 6] = m;
  }
  for (int c = tid; c < ORBX_SG_CELLS_MAX; c += SG_THREADS) s_cnt[c] = 0;
  __syncthreads();
  if (tid == 0) {
    double m[4];
    for (int i = 0; i < 4; i++) {
      m[i] = s_box[i][0];
      for (int k = 1; k < SG_THREADS / 64; k++) m[i] = fmax(m[i], s_box[i][k]);
    }
    OrbxSgGrid g;
    g.x0 = 0.0, g.y0 = 0.0, g.inv = 0.0, g.nx = 1, g.ny = 1;
    if (m[0] > ninf) {  // there is a positioned OK query
      const double x0 = -m[1] - radius, y0 = -m[3] - radius;
      const double ex = (m[0] + radius) - x0, ey = (m[2] + radius) - y0;
      const double side = fmax(radius, sqrt(ex * ey / (double)(ORBX_SG_CELLS_MAX / 2)));
      const double inv = 1.0 / side;
      if (wp_finite(x0) && wp_finite(y0) && wp_finite(side) && side > 0.0 && wp_finite(inv) && inv > 0.0) {
        const double fx = floor(ex * inv) + 1.0, fy = floor(ey * inv) + 1.0;
        g.nx = fx >= 256.0 ? 256 : (fx >= 1.0 ? (int)fx : 1);
        const int room = ORBX_SG_CELLS_MAX / g.nx;
        g.ny = fy >= (double)room ? room : (fy >= 1.0 ? (int)fy : 1);
        g.x0 = x0, g.y0 = y0, g.inv = inv;
      }
    }
    s_grid = g;
    grids[w] = g;
  }
  __syncthreads();
  const OrbxSgGrid g = s_grid;
  const int ncell = g.nx * g.ny;
  // (b) the histogram
  for (int t = tid; t < tcap; t += SG_THREADS) {
    double x, y;
    if (sg_train_in(tstate, tpstate, txy, trow + t, x, y))
      atomicAdd(&s_cnt[sg_cell(y, g.y0, g.inv, g.ny) * g.nx + sg_cell(x, g.x0, g.inv, g.nx)], 1);
  }
  __syncthreads();
  // (c) its exclusive prefix: every thread owns `per` neighbouring cells
  const int per = (ncell + SG_THREADS - 1) / SG_THREADS;
  const int c0 = min(tid * per, ncell), c1 = min(c0 + per, ncell);
  int sum = 0;
  for (int c = c0; c < c1; c++) sum += s_cnt[c];
  int total;
  int run = block_scan_excl<SG_THREADS>(sum, s_wave, &total);
  int32_t* S = starts + (size_t)w * (ORBX_SG_CELLS_MAX + 1);
  for (int c = c0; c < c1; c++) {
    const int n = s_cnt[c];
    s_cnt[c] = run;
    S[c] = run;
    run += n;
  }
  if (tid == 0) S[ncell] = total;
  __syncthreads();
  // (d) the placement: a slot takes the next free place of its cell
  for (int t = tid; t < tcap; t += SG_THREADS) {
    double x, y;
    if (!sg_train_in(tstate, tpstate, txy, trow + t, x, y)) continue;
    const int at = atomicAdd(&s_cnt[sg_cell(y, g.y0, g.inv, g.ny) * g.nx + sg_cell(x, g.x0, g.inv, g.nx)], 1);
    if (at < 0 || at >= tcap) continue;  // (cannot be: the places of a window are its counted slots)
    const uint4* src = reinterpret_cast<const uint4*>(tdesc + trow + t);
    sslot[trow + at] = t;
    sxy[2 * (trow + at)] = x, sxy[2 * (trow + at) + 1] = y;
    sdesc[2 * (trow + at)] = src[0];
    sdesc[2 * (trow + at) + 1] = src[1];
  }
}

// ---- rules K-N --------------------------------------------------------------------------------------------------------
// grid (ceil(qcap / 256), n_windows).  The window's cell starts go through LDS; a lane whose query is OK and positioned
// walks the grid rows its circle touches, one run of the sorted list per row.  The walk is widened by a hair (1e-9 of
// the radius and 1e-12 of the coordinate) so that a pair which the rounded test of rule L takes is never missed; a
// pair it looks at in vain costs one distance test.
__global__ __launch_bounds__(SG_THREADS) void k_sg_knn2(const orbx_descriptor* __restrict__ qdesc,
                                                         const int32_t* __restrict__ qstate,
                                                         const float* __restrict__ qxy, size_t point_stride,
                                                         size_t xy_frame_stride, int qcap, int tcap,
                                                         const OrbxSgGrid* __restrict__ grids,
                                                         const int32_t* __restrict__ starts,
                                                         const int32_t* __restrict__ sslot,
                                                         const double* __restrict__ sxy,
                                                         const uint4* __restrict__ sdesc, double radius, double ratio,
                                                         int max_distance, int accept_lone, int unique,
                                                         int32_t* __restrict__ origin, int32_t* __restrict__ dist,
                                                         int32_t* __restrict__ candidates,
                                                         uint32_t* __restrict__ best) {
  __shared__ int s_start[ORBX_SG_CELLS_MAX + 1];
  const int w = blockIdx.y, tid = threadIdx.x;
  OrbxSgGrid g = grids[w];
  g.nx = min(max(g.nx, 1), 256);  // (what k_sg_bin wrote; the clamps keep every index inside s_start whatever is there)
  g.ny = min(max(g.ny, 1), ORBX_SG_CELLS_MAX / g.nx);
  const int ncell = g.nx * g.ny;
  const int32_t* S = starts + (size_t)w * (ORBX_SG_CELLS_MAX + 1);
  for (int c = tid; c <= ncell; c += SG_THREADS) s_start[c] = min(max(S[c], 0), tcap);  // (inside the list, whatever)
  __syncthreads();
  const int q = blockIdx.x * SG_THREADS + tid;
  if (q >= qcap) return;
  const size_t qrow = (size_t)w * qcap, trow = (size_t)w * tcap;
  const float* qf = qxy + (size_t)w * xy_frame_stride + (size_t)q * point_stride;
  const float qx = qf[0], qy = qf[1];
  uint32_t k1 = 0xffffffffu, k2 = 0xffffffffu;
  int ncand = 0;
  if (qstate[qrow + q] == PD_OK && finite_f(qx) && finite_f(qy)) {
    const uint4* qp = reinterpret_cast<const uint4*>(qdesc + qrow + q);
    const uint4 qa = qp[0], qb = qp[1];
    const u64 q0 = ((u64)qa.y << 32) | qa.x, q1 = ((u64)qa.w << 32) | qa.z;
    const u64 q2 = ((u64)qb.y << 32) | qb.x, q3 = ((u64)qb.w << 32) | qb.z;
    const double r2 = radius * radius;
    const double X = (double)qx, Y = (double)qy;
    const double px = radius * 1e-9 + (fabs(X) + radius) * 1e-12, py = radius * 1e-9 + (fabs(Y) + radius) * 1e-12;
    const int cx0 = sg_cell(X - radius - px, g.x0, g.inv, g.nx), cx1 = sg_cell(X + radius + px, g.x0, g.inv, g.nx);
    const int cy0 = sg_cell(Y - radius - py, g.y0, g.inv, g.ny), cy1 = sg_cell(Y + radius + py, g.y0, g.inv, g.ny);
    for (int cy = cy0; cy <= cy1; cy++) {
      const int i1 = s_start[cy * g.nx + cx1 + 1];
      for (int i = s_start[cy * g.nx + cx0]; i < i1; i++) {
        if (!sp_in_gate(qx, qy, sxy[2 * (trow + i)], sxy[2 * (trow + i) + 1], r2)) continue;
        ncand++;
        const uint4 a = sdesc[2 * (trow + i)], b = sdesc[2 * (trow + i) + 1];
        const int d = __popcll(q0 ^ (((u64)a.y << 32) | a.x)) + __popcll(q1 ^ (((u64)a.w << 32) | a.z)) +
                      __popcll(q2 ^ (((u64)b.y << 32) | b.x)) + __popcll(q3 ^ (((u64)b.w << 32) | b.z));
        const uint32_t key = ((uint32_t)d << SG_KEY_SHIFT) | (uint32_t)sslot[trow + i];
        if (key < k1) {
          k2 = k1;
          k1 = key;
        } else if (key < k2) {
          k2 = key;
        }
      }
    }
  }
  const int d1 = (int)(k1 >> SG_KEY_SHIFT), d2 = (int)(k2 >> SG_KEY_SHIFT);
  const int j1 = (int)(k1 & ((1u << SG_KEY_SHIFT) - 1u));
  // rule N: two candidates or more -- rule H as k_ra_knn2 has it; exactly one -- accept_lone
  bool pass = false;
  if (ncand >= 2) pass = (double)(float)d1 < ratio * (double)(float)d2 && d1 <= max_distance;
  else if (ncand == 1) pass = accept_lone && d1 <= max_distance;
  origin[qrow + q] = pass ? j1 : -1;
  dist[qrow + q] = pass ? d1 : -1;
  candidates[qrow + q] = ncand;
  if (pass && unique) atomicMin(best + trow + j1, ((uint32_t)d1 << SG_KEY_SHIFT) | (uint32_t)q);
}

}  // namespace

hipError_t orbx_launch_sp_project(hipStream_t s, const OrbxCarryIn& in, int n_windows, int cap, const double* d_pose6,
                                  size_t pose_stride, const double* K4, int width, int height, double margin_px,
                                  double* d_xy, double* d_depth, int32_t* d_state, int32_t* d_count) {
  if (n_windows < 1 || cap < 1 || cap > ORBX_BA_MAX_POINTS) return hipErrorInvalidValue;
  // SP_NONE and the zeros of every slot that no landmark reaches
  const size_t slots = (size_t)n_windows * cap;
  hipError_t e = hipMemsetAsync(d_xy, 0, sizeof(double) * 2 * slots, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_depth, 0, sizeof(double) * slots, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_state, 0, sizeof(int32_t) * slots, s);
  if (e != hipSuccess) return e;
  const int blocks = (cap + SP_THREADS - 1) / SP_THREADS;  // n_windows * blocks <= n_windows * cap < 2^31
  hipLaunchKernelGGL(k_sp_project, dim3((unsigned)n_windows * blocks), dim3(SP_THREADS), 0, s, in, cap, blocks, d_pose6,
                     pose_stride, K4[0], K4[1], K4[2], K4[3], width, height, margin_px, d_xy, d_depth, d_state);
  hipLaunchKernelGGL(k_sp_count, dim3(n_windows), dim3(64), 0, s, d_state, cap, d_count);
  return hipGetLastError();
}

hipError_t orbx_launch_reassociate_gated(hipStream_t s, int n_windows, const orbx_descriptor* d_qdesc,
                                         const int32_t* d_qstate, const float* d_qxy, size_t point_stride,
                                         size_t xy_frame_stride, int qcap, const orbx_descriptor* d_tdesc,
                                         const int32_t* d_tstate, const double* d_txy, const int32_t* d_tpstate,
                                         int tcap, double radius_px, double ratio, int max_distance, int accept_lone,
                                         int unique, OrbxSgGrid* d_grids, int32_t* d_starts, int32_t* d_sslot,
                                         double* d_sxy, orbx_descriptor* d_sdesc, uint32_t* d_best, int32_t* d_origin,
                                         int32_t* d_dist, int32_t* d_candidates, int32_t* d_count) {
  if (n_windows < 1 || n_windows > 65535 || qcap < 1 || tcap < 1 || qcap > (1 << SG_KEY_SHIFT) ||
      tcap > (1 << SG_KEY_SHIFT))
    return hipErrorInvalidValue;
  if (unique) {
    const hipError_t e = hipMemsetAsync(d_best, 0xff, sizeof(uint32_t) * (size_t)n_windows * tcap, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_sg_bin, dim3(n_windows), dim3(SG_THREADS), 0, s, d_qstate, d_qxy, point_stride, xy_frame_stride,
                     qcap, d_tdesc, d_tstate, d_txy, d_tpstate, tcap, radius_px, d_grids, d_starts, d_sslot, d_sxy,
                     reinterpret_cast<uint4*>(d_sdesc));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sg_knn2, dim3((qcap + SG_THREADS - 1) / SG_THREADS, n_windows), dim3(SG_THREADS), 0, s, d_qdesc,
                     d_qstate, d_qxy, point_stride, xy_frame_stride, qcap, tcap, d_grids, d_starts, d_sslot, d_sxy,
                     reinterpret_cast<const uint4*>(d_sdesc), radius_px, ratio, max_distance, accept_lone, unique,
                     d_origin, d_dist, d_candidates, d_best);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return orbx_launch_ra_unique(s, n_windows, qcap, tcap, unique, d_best, d_origin, d_dist, d_count);
}
