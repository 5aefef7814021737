// orbx_pnp.hip -- batched perspective-n-point with RANSAC: the pose of a window's later
// frames from the window's own landmarks.  cv::solvePnPRansac in the reference's terms; the reference calls none (its
// window poses come from the essential-matrix chain alone, src/with_bundle_adjustment.cpp:196-208).
// One launch, one workgroup of 256 lanes per problem (window w, frame k >= 2):
//   prologue  the problem's correspondences out of the landmarks block, in ascending point order
//   RANSAC    chunks of PNP_CHUNK iterations: the first wave solves one sample per lane into LDS, all four waves
//             stride the correspondences to score every model, one lane selects in (iteration, model) order
//   refine    Levenberg-Marquardt on the best model's inliers, sums by rule 9
//   final     mask, inlier count and RMS of the pose that is kept, the record and the seeded pose
// The problems of rank 18 (every frame of a window against landmarks carried from the window before, orbx_carry.hip)
// come gathered and skip the prologue; they differ from the host-array problem in where the count, the seed and the
// mask's index come from, nowhere in the arithmetic.
// All arithmetic comes from orbx_pnp_math.h, compiled with -ffp-contract=off, so each problem's result equals the
// sequential restatement (tests/cpp/pnp_sequential.cpp) bit for bit.  No atomics.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_lm_math.h"
#include "orbx_pnp_math.h"
#include "orbx_wave.h"

namespace {

// samples solved per chunk, one per lane of the first wave: 64 x 4 models x 12 doubles = 24 KB of LDS
constexpr int PNP_CHUNK = 64;
constexpr int PNP_THREADS = PNP_LANES;

struct PnpArgs {
  OrbxPnpIn in;
  double K4[4];
  double prob, thr2;
  uint64_t seed;
  int n_pre;  // the correspondences of a problem that comes gathered (in.status == NULL)
  // not NULL: EVERY problem comes gathered (orbx_carry.hip, rank 18), frames 0 and 1 included: its count, or -1 for a
  // window with nothing carried; the seed is the problem's by its frame and the mask is indexed through cidx
  const int32_t* ncorr;
  int window_len, cap, max_iters, refine_iters, min_inliers;
  OrbxPnpCorr* corr;
  int32_t* cidx;
  OrbxPnpRecord* rec;
  double* seeded6;
  uint8_t* mask;
};

struct PnpShared {
  double model[PNP_CHUNK * PNP_MAX_MODELS * PNP_MODEL_DOUBLES];
  double best[PNP_MODEL_DOUBLES];
  double wave[4 * PNP_NSUM], red[PNP_NSUM];
  PnpLm lm;
  int nmod[PNP_CHUNK];
  int cnt[4 * PNP_CHUNK * PNP_MAX_MODELS];
  int state[3];  // niters, best count, iterations run
  int scan[4];
  int flag;
};

// rule 9: the lanes' partial sums through the xor butterfly of each wave, the four waves as ((g0 + g1) + g2) + g3;
// the sums are in S.red behind the call
template <int N>
__device__ __forceinline__ void pnp_block_sum(double (&v)[N], PnpShared& S) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = wave_sum_f64(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) S.wave[wave * N + k] = v[k];
  }
  __syncthreads();
  if (tid < N) S.red[tid] = ((S.wave[tid] + S.wave[N + tid]) + S.wave[2 * N + tid]) + S.wave[3 * N + tid];
  __syncthreads();
}
// the workgroup's integer sum in every lane
__device__ __forceinline__ int pnp_block_count(int c, PnpShared& S) {
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) S.scan[threadIdx.x >> 6] = c;
  __syncthreads();
  const int all = S.scan[0] + S.scan[1] + S.scan[2] + S.scan[3];
  __syncthreads();
  return all;
}

// one refinement pass at pose6 over the inliers of the best model: the sums are in S.red behind the call
__device__ __forceinline__ void pnp_pass(const PnpArgs& a, const OrbxPnpCorr* C, int n, const double* pose6,
                                         const double* Mbest, PnpShared& S) {
  BaPose P;
  ba_pose_prepare(pose6, &P);
  double acc[PNP_NSUM];
#pragma unroll
  for (int i = 0; i < PNP_NSUM; i++) acc[i] = 0.0;
  for (int p = threadIdx.x; p < n; p += PNP_THREADS) {
    const OrbxPnpCorr q = C[p];
    double e2;
    if (pnp_inlier(a.K4, Mbest, q.X, q.x, q.y, a.thr2, &e2)) pnp_refine_term(a.K4, P, q.X, q.x, q.y, acc);
  }
  if (!P.ok) acc[27] = pose_u2d(0x7ff0000000000000ull);
  pnp_block_sum(acc, S);
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_ransac(const PnpArgs a) {
  __shared__ PnpShared S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool carried = a.ncorr != nullptr;
  const int k0 = carried ? 0 : 2, per_win = a.window_len - k0;
  const int prob_i = blockIdx.x, w = prob_i / per_win, k = k0 + prob_i % per_win;
  const int cap = a.cap;
  const bool gathered = a.in.status == nullptr;
  const bool by_index = gathered && !carried;  // the host-array problem: its own seed, the mask in its own order
  const uint64_t seed = by_index ? a.seed : pnp_problem_seed(a.seed, (uint32_t)k);
  OrbxPnpCorr* C = a.corr + (size_t)prob_i * cap;
  int32_t* CI = a.cidx + (size_t)prob_i * cap;
  uint8_t* M = a.mask + (size_t)prob_i * cap;
  OrbxPnpRecord* rec = a.rec + prob_i;
  const double* built = gathered ? nullptr : a.in.built6 + 6 * (size_t)a.window_len * w;
  double* seeded = gathered ? nullptr : a.seeded6 + 6 * (size_t)a.window_len * w;

  // what every way out leaves behind unless it is overwritten below: an empty mask, the built poses
  for (int p = tid; p < cap; p += PNP_THREADS) M[p] = 0;
  if (!gathered) {
    if (tid < 6) seeded[6 * k + tid] = built[6 * k + tid];
    if (k == 2 && tid < 12) seeded[tid] = built[tid];
  }
  int status = PNP_OK, n = 0, iters = 0;
  if (carried) {
    n = a.ncorr[prob_i];
    if (n < 0) n = 0, status = PNP_SKIPPED;
  } else if (gathered) {
    n = a.n_pre;
  } else if (a.in.status[w] != LM_OK) {
    status = PNP_SKIPPED;
  } else {
    // prologue: point j of the window takes part iff rows[j] + k < rows[j + 1]
    const int p0 = a.in.pt_off[w], np = a.in.pt_off[w + 1] - p0;
    const int32_t* rows = a.in.rows + p0 + w;
    const double* pts = a.in.points3 + 3 * (size_t)p0;
    const double* oxy = a.in.oxy + 2 * (size_t)a.in.obs_off[w];
    for (int j0 = 0; j0 < np; j0 += PNP_THREADS) {
      const int j = j0 + tid;
      int r = 0, has = 0;
      if (j < np) {
        r = rows[j] + k;
        has = r < rows[j + 1] ? 1 : 0;
      }
      int total;
      const int at = n + block_scan_excl<PNP_THREADS>(has, S.scan, &total);
      if (has && at < cap) {
        OrbxPnpCorr q;
        q.X[0] = pts[3 * j], q.X[1] = pts[3 * j + 1], q.X[2] = pts[3 * j + 2];
        q.x = oxy[2 * r], q.y = oxy[2 * r + 1];
        C[at] = q;
        CI[at] = j;
      }
      n += total;
    }
    n = n < cap ? n : cap;  // (a window has at most cap points)
  }
  if (status == PNP_OK && n < a.min_inliers) status = PNP_FEW_POINTS;
  __syncthreads();  // the correspondences are in place for every lane

  const double fx = a.K4[0], fy = a.K4[1], cx = a.K4[2], cy = a.K4[3];
  if (status == PNP_OK) {
    if (tid == 0) {
      S.state[0] = a.max_iters;
      S.state[1] = 0;
      S.state[2] = 0;
    }
    __syncthreads();
    // the lane's first correspondence stays in registers over the chunk's models
    const bool has0 = tid < n;
    OrbxPnpCorr c0 = {};
    if (has0) c0 = C[tid];
    for (int base = 0;; base += PNP_CHUNK) {
      const int niters0 = S.state[0];
      if (base >= niters0) break;
      // 1. solve: lane l of the first wave takes iteration base + l
      if (wave == 0) {
        int nm = 0;
        const int it = base + lane;
        uint32_t idx[3];
        if (it < niters0 && pnp_sample3(seed, (uint32_t)it, (uint32_t)n, idx)) {
          double X[9], xy[6];
#pragma unroll
          for (int i = 0; i < 3; i++) {
            const OrbxPnpCorr q = C[idx[i]];
            X[3 * i] = q.X[0], X[3 * i + 1] = q.X[1], X[3 * i + 2] = q.X[2];
            xy[2 * i] = (q.x - cx) / fx, xy[2 * i + 1] = (q.y - cy) / fy;
          }
          nm = pnp_p3p(X, xy, S.model + lane * PNP_MAX_MODELS * PNP_MODEL_DOUBLES);
        }
        S.nmod[lane] = nm;
      }
      __syncthreads();
      // 2. score: every wave counts its quarter of the correspondences for every model of the chunk
      for (int l = 0; l < PNP_CHUNK; l++) {
        const int nm = S.nmod[l];
        for (int m = 0; m < nm; m++) {
          double Mo[PNP_MODEL_DOUBLES];
#pragma unroll
          for (int e = 0; e < PNP_MODEL_DOUBLES; e++) Mo[e] = S.model[(l * PNP_MAX_MODELS + m) * PNP_MODEL_DOUBLES + e];
          double e2;
          int c = has0 && pnp_inlier(a.K4, Mo, c0.X, c0.x, c0.y, a.thr2, &e2) ? 1 : 0;
          for (int p = tid + PNP_THREADS; p < n; p += PNP_THREADS) {
            const OrbxPnpCorr q = C[p];
            c += pnp_inlier(a.K4, Mo, q.X, q.x, q.y, a.thr2, &e2) ? 1 : 0;
          }
          c = wave_sum(c);
          if (lane == 0) S.cnt[(wave * PNP_CHUNK + l) * PNP_MAX_MODELS + m] = c;
        }
      }
      __syncthreads();
      // 3. the selection, in (iteration, model) order
      if (tid == 0) {
        int niters = S.state[0], best = S.state[1], i = base;
        const int floor_ = a.min_inliers - 1;
        for (; i < base + PNP_CHUNK && i < niters; i++) {
          const int l = i - base;
          for (int m = 0; m < S.nmod[l]; m++) {
            const int at = l * PNP_MAX_MODELS + m;
            const int count = S.cnt[at] + S.cnt[PNP_CHUNK * PNP_MAX_MODELS + at] +
                              S.cnt[2 * PNP_CHUNK * PNP_MAX_MODELS + at] + S.cnt[3 * PNP_CHUNK * PNP_MAX_MODELS + at];
            if (count > (best > floor_ ? best : floor_)) {
              best = count;
              for (int e = 0; e < PNP_MODEL_DOUBLES; e++) S.best[e] = S.model[at * PNP_MODEL_DOUBLES + e];
              niters = pnp_update_niters(a.prob, (double)(n - count) / n, niters);
            }
          }
        }
        S.state[0] = niters;
        S.state[1] = best;
        S.state[2] = i;
      }
      __syncthreads();
    }
    iters = S.state[2];
    if (S.state[1] == 0) status = PNP_NO_MODEL;
  }

  if (status != PNP_OK) {
    if (tid == 0) {
      for (int i = 0; i < 6; i++) rec->pose6[i] = gathered ? 0.0 : built[6 * k + i];
      rec->inliers = 0;
      rec->iters = iters;
      rec->n_corr = n;
      rec->status = status;
      rec->rms_px = 0.0;
    }
    return;
  }

  // 4. refinement over the inliers of the best model
  const int best = S.state[1];
  double Mb[PNP_MODEL_DOUBLES], Mk[PNP_MODEL_DOUBLES], pose_k[6];
#pragma unroll
  for (int e = 0; e < PNP_MODEL_DOUBLES; e++) Mb[e] = S.best[e], Mk[e] = S.best[e];
  pnp_model_to_pose6(Mb, pose_k);
  if (a.refine_iters > 0) {
    pnp_pass(a, C, n, pose_k, Mb, S);
    if (tid == 0) {
      for (int i = 0; i < 6; i++) S.lm.x[i] = pose_k[i];
      for (int i = 0; i < PNP_NSUM; i++) S.lm.acc[i] = S.red[i];
      S.lm.lambda = PNP_LAMBDA0;
    }
    __syncthreads();
    for (int it = 0; it < a.refine_iters; it++) {
      if (tid == 0) S.flag = pnp_lm_propose(&S.lm) ? 1 : 0;
      __syncthreads();
      if (!S.flag) break;
      double cand[6];
#pragma unroll
      for (int i = 0; i < 6; i++) cand[i] = S.lm.cand[i];
      pnp_pass(a, C, n, cand, Mb, S);
      if (tid == 0) pnp_lm_decide(&S.lm, S.red);
      __syncthreads();
    }
    // the refined pose replaces the RANSAC pose only if its inlier count is not smaller
    double xr[6], Mr[PNP_MODEL_DOUBLES];
#pragma unroll
    for (int i = 0; i < 6; i++) xr[i] = S.lm.x[i];
    BaPose P;
    ba_pose_prepare(xr, &P);
    pnp_pose_to_model(P, Mr);
    int c = 0;
    for (int p = tid; p < n; p += PNP_THREADS) {
      const OrbxPnpCorr q = C[p];
      double e2;
      c += pnp_inlier(a.K4, Mr, q.X, q.x, q.y, a.thr2, &e2) ? 1 : 0;
    }
    c = pnp_block_count(c, S);
    if (P.ok && c >= best) {
#pragma unroll
      for (int e = 0; e < PNP_MODEL_DOUBLES; e++) Mk[e] = Mr[e];
#pragma unroll
      for (int i = 0; i < 6; i++) pose_k[i] = xr[i];
    }
  }

  // 5. mask, inlier count and RMS of the pose that is kept
  double sum[1] = {0.0};
  int cnt = 0;
  for (int p = tid; p < n; p += PNP_THREADS) {
    const OrbxPnpCorr q = C[p];
    double e2;
    if (pnp_inlier(a.K4, Mk, q.X, q.x, q.y, a.thr2, &e2)) {
      M[by_index ? p : CI[p]] = 1;
      sum[0] = sum[0] + e2;
      cnt++;
    }
  }
  cnt = pnp_block_count(cnt, S);
  pnp_block_sum(sum, S);
  if (tid == 0) {
    for (int i = 0; i < 6; i++) rec->pose6[i] = pose_k[i];
    rec->inliers = cnt;
    rec->iters = iters;
    rec->n_corr = n;
    rec->status = PNP_OK;
    rec->rms_px = cnt > 0 ? pose_sqrt(S.red[0] / (double)cnt) : 0.0;
    if (!gathered)
      for (int i = 0; i < 6; i++) seeded[6 * k + i] = pose_k[i];
  }
}

}  // namespace

hipError_t orbx_launch_pnp(hipStream_t s, int n_windows, int window_len, int cap, const OrbxPnpIn& in, int n_pre,
                           const double* K4, double prob, double threshold_px, int max_iters, uint64_t seed,
                           int refine_iters, int min_inliers, OrbxPnpCorr* d_corr, int32_t* d_cidx,
                           OrbxPnpRecord* d_rec, double* d_seeded6, uint8_t* d_mask, const int32_t* d_ncorr) {
  const int per_win = window_len - (d_ncorr ? 0 : 2);
  if (n_windows <= 0 || per_win < 1) return hipSuccess;
  PnpArgs a;
  a.in = in;
  for (int i = 0; i < 4; i++) a.K4[i] = K4[i];
  a.prob = prob;
  a.thr2 = threshold_px * threshold_px;
  a.seed = seed;
  a.n_pre = n_pre;
  a.ncorr = d_ncorr;
  a.window_len = window_len, a.cap = cap, a.max_iters = max_iters, a.refine_iters = refine_iters;
  a.min_inliers = min_inliers;
  a.corr = d_corr, a.cidx = d_cidx, a.rec = d_rec, a.seeded6 = d_seeded6, a.mask = d_mask;
  hipLaunchKernelGGL(k_pnp_ransac, dim3(n_windows * per_win), dim3(PNP_THREADS), 0, s, a);
  return hipGetLastError();
}
