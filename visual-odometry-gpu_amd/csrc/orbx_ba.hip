// orbx_ba.hip -- batched sliding-window bundle adjustment.
//
// Replaces the reference's Ceres solve of one window,
//   ReprojectionError (angle-axis pose, pinhole projection)            src/with_bundle_adjustment.cpp:27-68
//   problem set-up, HuberLoss(1.0), pose 0 constant, SPARSE_SCHUR       src/with_bundle_adjustment.cpp:612-679
// with k_ba_lm: one workgroup of 256 lanes per window, the whole Levenberg-Marquardt loop inside one launch.
//   - observations in CSR by landmark; a lane owns landmarks lane, lane + 256, ...
//   - every sum over landmarks (costs, pose blocks, the Schur complement one 6x6 pose-pair block at a time, its right
//     side together with the diagonal blocks) is a lane-strided partial sum, an xor butterfly inside the wave, then
//     the four waves in order (rule 9)
//   - lane 0 assembles and solves the reduced camera system (Cholesky, at most 42 x 42, in LDS) and applies the
//     trust-region rules; all lanes back-substitute and evaluate the candidate
//   - accepted and candidate points, the per-landmark blocks and the per-observation coupling blocks W live in a
//     workspace owned by the workgroup (global memory, reused across the windows the workgroup solves)
// All arithmetic comes from orbx_ba_math.h, compiled with -ffp-contract=off, so every result equals the sequential
// restatement (tests/cpp/ba_sequential.cpp) bit for bit.
#include <hip/hip_runtime.h>

#include "orbx_internal.h"
#include "orbx_ba_math.h"
#include "orbx_wave.h"

namespace {

constexpr int BA_THREADS = BA_LANES;
constexpr int BA_MAXF = ORBX_BA_MAX_POSES - 1;  // free poses
constexpr int BA_LD = 6 * BA_MAXF;              // leading dimension of the reduced system
constexpr int BA_NRED = 36;                     // widest reduction: a 6x6 pose-pair block

// workspace rows per landmark (SoA, stride = the workspace's landmark capacity)
enum { Q_X = 0, Q_CAND = 3, Q_V = 6, Q_GP = 12, Q_SP = 15, Q_VINV = 18, Q_GS = 24, Q_D2 = 27 };
static_assert(Q_D2 + 3 == ORBX_BA_WS_POINT, "workspace rows per landmark");
static_assert(18 == ORBX_BA_WS_OBS, "workspace rows per observation");

struct BaK4 {
  double k[4];
};

struct BaShared {
  double x[ORBX_BA_MAX_POSES * 6], cand[ORBX_BA_MAX_POSES * 6];
  BaPose Px[ORBX_BA_MAX_POSES], Pc[ORBX_BA_MAX_POSES];
  double sc[6 * BA_MAXF], U[27 * BA_MAXF], Dc[6 * BA_MAXF], gcs[6 * BA_MAXF];
  double A[BA_LD * BA_LD], b[BA_LD];
  double wave[4 * BA_NRED], red[BA_NRED];
  BaTrust T;
  BaSummary sum;
  double gmax, pose_model, pose_step2, pose_x2;
  int solved, action, done, bad;
};

template <int N, bool MAX = false>
__device__ __forceinline__ void block_reduce(double (&v)[N], BaShared& S) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = MAX ? wave_max_f64(v[k]) : wave_sum_f64(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) S.wave[wave * N + k] = v[k];
  }
  __syncthreads();
  if (tid < N) {
    const double a = S.wave[tid], b = S.wave[N + tid], c = S.wave[2 * N + tid], d = S.wave[3 * N + tid];
    if (MAX) {
      double m = a > b ? a : b;
      m = m > c ? m : c;
      S.red[tid] = m > d ? m : d;
    } else {
      S.red[tid] = ((a + b) + c) + d;
    }
  }
  __syncthreads();
}

struct BaWin {
  int W, N, cap, ocap;       // poses, landmarks, workspace strides
  const int32_t* row;        // N + 1 offsets into the window's observations
  const uint8_t* opose;      // pose of each observation
  const double* oxy;         // (x, y) of each observation
  double* wp;                // workspace: ORBX_BA_WS_POINT rows of `cap`
  double* wo;                // workspace: ORBX_BA_WS_OBS rows of `ocap`
  unsigned long long* slot;  // byte i: position of pose i's observation in the landmark's row, 0xff: none
  BaK4 K;
  double delta;
};

// cost, point blocks, W blocks, then one pose block per pass; S.red[0] = sum rho on return (before the pose passes),
// S.gmax = max |gradient|.  first: also the Jacobi scales and the depth check.  PRIOR (rank 20): `prior` holds the
// window's anchors and weights, four doubles per landmark; a landmark's prior comes behind its last observation
// (rule P1), so sum rho, V, the gradient and the Jacobi scales all include it.
template <bool PRIOR>
__device__ void ba_linearize(const BaWin& w, BaShared& S, bool first, double* sum_rho, const double* prior) {
  const int tid = threadIdx.x;
  double acc1[1] = {0.0}, gm[1] = {0.0};
  int bad = 0;
  for (int j = tid; j < w.N; j += BA_THREADS) {
    double X[3], V[6] = {0, 0, 0, 0, 0, 0}, gp[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = w.wp[(Q_X + k) * w.cap + j];
    for (int o = w.row[j]; o < w.row[j + 1]; o++) {
      const int i = w.opose[o];
      BaObs ob;
      ba_obs_eval(w.K.k, S.Px[i], X, w.oxy[2 * o], w.oxy[2 * o + 1], w.delta, true, &ob);
      acc1[0] = acc1[0] + ob.rho;
      if (ob.z == 0.0) bad = 1;
      ba_accum_point(ob, V, gp);
      if (i > 0) {
        double Wb[18];
        ba_obs_W(ob, Wb);
#pragma unroll
        for (int k = 0; k < 18; k++) w.wo[k * w.ocap + o] = Wb[k];
      }
    }
    if (PRIOR) {  // (loaded here, behind the loop: the four doubles are not live across the observations)
      const double A[3] = {prior[4 * j], prior[4 * j + 1], prior[4 * j + 2]};
      ba_prior_accum(X, A, prior[4 * j + 3], V, gp, &acc1[0]);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) w.wp[(Q_V + k) * w.cap + j] = V[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      w.wp[(Q_GP + k) * w.cap + j] = gp[k];
      const double a = pose_abs(gp[k]);
      gm[0] = a > gm[0] ? a : gm[0];
    }
    if (first) {
      w.wp[(Q_SP + 0) * w.cap + j] = ba_jacobi_scale(V[0]);
      w.wp[(Q_SP + 1) * w.cap + j] = ba_jacobi_scale(V[3]);
      w.wp[(Q_SP + 2) * w.cap + j] = ba_jacobi_scale(V[5]);
    }
  }
  if (first && bad) S.bad = 1;  // (benign race: every writer stores 1)
  block_reduce<1>(acc1, S);
  *sum_rho = S.red[0];
  block_reduce<1, true>(gm, S);
  double gmax = S.red[0];
  for (int f = 0; f < w.W - 1; f++) {
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0.0;
    for (int j = tid; j < w.N; j += BA_THREADS) {
      const int b = (int)((w.slot[j] >> (8 * (f + 1))) & 0xff);
      if (b == 0xff) continue;
      const int o = w.row[j] + b;
      double X[3];
#pragma unroll
      for (int k = 0; k < 3; k++) X[k] = w.wp[(Q_X + k) * w.cap + j];
      BaObs ob;
      ba_obs_eval(w.K.k, S.Px[f + 1], X, w.oxy[2 * o], w.oxy[2 * o + 1], w.delta, true, &ob);
      ba_accum_pose(ob, acc);
    }
    block_reduce<27>(acc, S);
    if (tid < 27) S.U[f * 27 + tid] = S.red[tid];
    for (int k = 21; k < 27; k++) {  // (S.red is rewritten only behind the next reduction's first barrier)
      const double a = pose_abs(S.red[k]);
      gmax = a > gmax ? a : gmax;
    }
  }
  if (tid == 0) S.gmax = gmax;
  if (first && tid < 6 * (w.W - 1)) {
    const int f = tid / 6, a = tid % 6;
    S.sc[tid] = ba_jacobi_scale(S.U[f * 27 + a * (a + 1) / 2 + a]);
  }
  __syncthreads();
}

// PRIOR = false is the solve of rank 7 and takes none of the prior's paths: prior and start are not read.  PRIOR = true
// (rank 20): prior is [points][4], anchor and weight of every landmark in the batch's point order; start is
// ORBX_PRIOR_START_GIVEN (0) or ORBX_PRIOR_START_ANCHOR (1).
template <bool PRIOR>
__global__ __launch_bounds__(BA_THREADS) void k_ba_lm(int n_windows, int max_iters, BaK4 K, double delta,
                                                      const int32_t* __restrict__ pose_off,
                                                      const int32_t* __restrict__ pt_off,
                                                      const int32_t* __restrict__ obs_off,
                                                      double* __restrict__ poses, double* __restrict__ points,
                                                      const int32_t* __restrict__ rows,
                                                      const uint8_t* __restrict__ obs_pose,
                                                      const double* __restrict__ obs_xy, int cap, int ocap,
                                                      double* __restrict__ ws_pt, double* __restrict__ ws_obs,
                                                      unsigned long long* __restrict__ ws_slot,
                                                      BaSummary* __restrict__ out,
                                                      const double* __restrict__ prior, int start) {
  __shared__ BaShared S;
  const int tid = threadIdx.x;
  BaWin w;
  w.cap = cap, w.ocap = ocap, w.K = K, w.delta = delta;
  w.wp = ws_pt + (size_t)blockIdx.x * ORBX_BA_WS_POINT * cap;
  w.wo = ws_obs + (size_t)blockIdx.x * ORBX_BA_WS_OBS * ocap;
  w.slot = ws_slot + (size_t)blockIdx.x * cap;
  for (int win = blockIdx.x; win < n_windows; win += gridDim.x) {
    __syncthreads();  // the previous window's shared state is dead
    const int W = pose_off[win + 1] - pose_off[win], N = pt_off[win + 1] - pt_off[win];
    if (N == 0) {  // (uniform) an empty window of a landmarks block: nothing of it is read
      if (tid == 0) out[win] = BaSummary{BA_SKIPPED, 0, 0, 0, 0.0, 0.0};
      continue;
    }
    const int P = W - 1;
    w.W = W, w.N = N;
    w.row = rows + pt_off[win] + win;
    w.opose = obs_pose + obs_off[win];
    w.oxy = obs_xy + 2 * (size_t)obs_off[win];
    double* g_pose = poses + 6 * (size_t)pose_off[win];
    double* g_pt = points + 3 * (size_t)pt_off[win];
    const double* g_prior = PRIOR ? prior + 4 * (size_t)pt_off[win] : nullptr;
    // ---- set-up: accepted parameters, the landmark's pose -> observation table
    if (tid < 6 * W) S.x[tid] = g_pose[tid];
    if (tid == 0) S.bad = 0, S.done = 0;
    for (int j = tid; j < N; j += BA_THREADS) {
#pragma unroll
      for (int k = 0; k < 3; k++) w.wp[(Q_X + k) * cap + j] = g_pt[3 * j + k];
      if (PRIOR && start == 1 && g_prior[4 * j + 3] > 0.0) {  // rule P5: an anchored landmark starts at its anchor
#pragma unroll
        for (int k = 0; k < 3; k++) w.wp[(Q_X + k) * cap + j] = g_prior[4 * j + k];
      }
      unsigned long long sl = ~0ull;
      const int r0 = w.row[j];
      for (int o = r0; o < w.row[j + 1]; o++) {
        const int i = w.opose[o];
        sl = (sl & ~(0xffull << (8 * i))) | ((unsigned long long)(o - r0) << (8 * i));
      }
      w.slot[j] = sl;
    }
    __syncthreads();
    if (tid < W) {
      ba_pose_prepare(S.x + 6 * tid, &S.Px[tid]);
      if (!S.Px[tid].ok) S.bad = 1;
    }
    __syncthreads();
    double sum_rho;
    ba_linearize<PRIOR>(w, S, true, &sum_rho, g_prior);
    if (tid == 0) {
      const double cost = 0.5 * sum_rho;
      S.T.radius = BA_RADIUS0, S.T.decrease = 2.0, S.T.cost = cost;
      S.sum.termination = BA_NO_CONVERGENCE, S.sum.iterations = 0, S.sum.successful_steps = 0, S.sum.pad = 0;
      S.sum.initial_cost = cost;
      if (S.bad || !(cost <= BA_DBL_MAX)) {
        S.sum.termination = BA_FAILURE;
        S.done = 1;
      } else if (S.gmax <= BA_GRADIENT_TOL) {
        S.sum.termination = BA_CONVERGENCE;
        S.done = 1;
      }
    }
    __syncthreads();
    for (int it = 1; it <= max_iters; it++) {
      if (S.done) break;  // uniform: S.done changes only between barriers
      const double radius = S.T.radius;
      // ---- S1: damped point blocks, inverted
      for (int j = tid; j < N; j += BA_THREADS) {
        double V[6], gp[3], sp[3], Vi[6], gs[3], D2[3];
#pragma unroll
        for (int k = 0; k < 6; k++) V[k] = w.wp[(Q_V + k) * cap + j];
#pragma unroll
        for (int k = 0; k < 3; k++) gp[k] = w.wp[(Q_GP + k) * cap + j], sp[k] = w.wp[(Q_SP + k) * cap + j];
        ba_point_invert(V, gp, sp, radius, Vi, gs, D2);
#pragma unroll
        for (int k = 0; k < 6; k++) w.wp[(Q_VINV + k) * cap + j] = Vi[k];
#pragma unroll
        for (int k = 0; k < 3; k++) w.wp[(Q_GS + k) * cap + j] = gs[k], w.wp[(Q_D2 + k) * cap + j] = D2[k];
      }
      // (each lane reads back only what it wrote itself: no barrier needed before S2)
      // ---- S2: the Schur complement, one pose-pair block at a time
      for (int f = 0; f < P; f++) {
        for (int g = 0; g < f; g++) {  // two different poses: a full 6x6 block
          double acc[36];
#pragma unroll
          for (int k = 0; k < 36; k++) acc[k] = 0.0;
          for (int j = tid; j < N; j += BA_THREADS) {
            const unsigned long long sl = w.slot[j];
            const int bf = (int)((sl >> (8 * (f + 1))) & 0xff), bg = (int)((sl >> (8 * (g + 1))) & 0xff);
            if (bf == 0xff || bg == 0xff) continue;
            const int r0 = w.row[j];
            double sp[3], Vi[6], Wf[18], Y[18];
#pragma unroll
            for (int k = 0; k < 3; k++) sp[k] = w.wp[(Q_SP + k) * cap + j];
#pragma unroll
            for (int k = 0; k < 6; k++) Vi[k] = w.wp[(Q_VINV + k) * cap + j];
#pragma unroll
            for (int k = 0; k < 18; k++) Wf[k] = w.wo[k * ocap + r0 + bf];
            ba_scale_W(Wf, S.sc + 6 * f, sp, Wf);
            ba_W_Vinv(Wf, Vi, Y);
#pragma unroll
            for (int b = 0; b < 6; b++) {  // Wg one row at a time: 3 live doubles instead of 18
              double wg[3];
#pragma unroll
              for (int k = 0; k < 3; k++) wg[k] = w.wo[(b * 3 + k) * ocap + r0 + bg];
              ba_scale_W_row(wg, S.sc[6 * g + b], sp, wg);
              ba_accum_pair_col(Y, wg, b, acc);
            }
          }
          block_reduce<36>(acc, S);
          if (tid < 36) S.A[(6 * f + tid / 6) * BA_LD + 6 * g + tid % 6] = S.red[tid];
        }
        {  // the pose with itself: the lower triangle and the right side
          double acc[27];
#pragma unroll
          for (int k = 0; k < 27; k++) acc[k] = 0.0;
          for (int j = tid; j < N; j += BA_THREADS) {
            const int bf = (int)((w.slot[j] >> (8 * (f + 1))) & 0xff);
            if (bf == 0xff) continue;
            const int r0 = w.row[j];
            double sp[3], gs[3], Vi[6], Wf[18], Y[18];
#pragma unroll
            for (int k = 0; k < 3; k++) sp[k] = w.wp[(Q_SP + k) * cap + j], gs[k] = w.wp[(Q_GS + k) * cap + j];
#pragma unroll
            for (int k = 0; k < 6; k++) Vi[k] = w.wp[(Q_VINV + k) * cap + j];
#pragma unroll
            for (int k = 0; k < 18; k++) Wf[k] = w.wo[k * ocap + r0 + bf];
            ba_scale_W(Wf, S.sc + 6 * f, sp, Wf);
            ba_W_Vinv(Wf, Vi, Y);
            ba_accum_diag(Y, Wf, acc);
            ba_accum_rhs(Y, gs, acc + 21);
          }
          block_reduce<27>(acc, S);
          if (tid < 21) {
            const int a = tid >= 15 ? 5 : tid >= 10 ? 4 : tid >= 6 ? 3 : tid >= 3 ? 2 : tid >= 1 ? 1 : 0;
            S.A[(6 * f + a) * BA_LD + 6 * f + (tid - a * (a + 1) / 2)] = S.red[tid];
          } else if (tid < 27) {
            S.b[6 * f + tid - 21] = S.red[tid];
          }
        }
      }
      __syncthreads();
      // ---- S3: lane 0 assembles and solves the reduced camera system, forms the candidate poses
      if (tid == 0) {
        ba_assemble(P, S.U, S.sc, radius, S.A, BA_LD, S.b, S.Dc, S.gcs);
        S.solved = ba_cholesky_solve(6 * P, BA_LD, S.A, S.b) ? 1 : 0;
        if (S.solved) ba_pose_step(W, S.x, S.sc, S.b, S.Dc, S.gcs, S.cand, &S.pose_model, &S.pose_step2, &S.pose_x2);
      }
      __syncthreads();
      const int solved = S.solved;
      double acc4[4] = {0.0, 0.0, 0.0, 0.0};
      if (solved) {
        if (tid < W) ba_pose_prepare(S.cand + 6 * tid, &S.Pc[tid]);
        __syncthreads();
        // ---- S4: back-substitution and the candidate's cost
        for (int j = tid; j < N; j += BA_THREADS) {
          double X[3], sp[3], Vi[6], gs[3], D2[3], u[3] = {0.0, 0.0, 0.0}, cd[3];
#pragma unroll
          for (int k = 0; k < 3; k++) {
            X[k] = w.wp[(Q_X + k) * cap + j], sp[k] = w.wp[(Q_SP + k) * cap + j];
            gs[k] = w.wp[(Q_GS + k) * cap + j], D2[k] = w.wp[(Q_D2 + k) * cap + j];
          }
#pragma unroll
          for (int k = 0; k < 6; k++) Vi[k] = w.wp[(Q_VINV + k) * cap + j];
          const int r0 = w.row[j], r1 = w.row[j + 1];
          for (int o = r0; o < r1; o++) {
            const int i = w.opose[o];
            if (i == 0) continue;
            double Wu[18], Ws[18];
#pragma unroll
            for (int k = 0; k < 18; k++) Wu[k] = w.wo[k * ocap + o];
            ba_scale_W(Wu, S.sc + 6 * (i - 1), sp, Ws);
            ba_accum_Wt_step(Ws, S.b + 6 * (i - 1), u);
          }
          ba_point_step(Vi, gs, u, D2, sp, X, cd, acc4);
#pragma unroll
          for (int k = 0; k < 3; k++) w.wp[(Q_CAND + k) * cap + j] = cd[k];
          for (int o = r0; o < r1; o++) {
            double z;
            acc4[3] = acc4[3] + ba_obs_cost(w.K.k, S.Pc[w.opose[o]], cd, w.oxy[2 * o], w.oxy[2 * o + 1], w.delta, &z);
          }
          if (PRIOR) {  // rule P2: the landmark's prior term right behind its observations'
            const double lam = g_prior[4 * j + 3];
            if (lam > 0.0) {
              const double A[3] = {g_prior[4 * j], g_prior[4 * j + 1], g_prior[4 * j + 2]};
              acc4[3] = acc4[3] + ba_prior_cost(cd, A, lam);
            }
          }
        }
      }
      block_reduce<4>(acc4, S);
      // ---- S5: lane 0 decides
      if (tid == 0) {
        double cand_cost = 0.5 * S.red[3];
        if (solved)
          for (int i = 0; i < W; i++)
            if (!S.Pc[i].ok) cand_cost = BA_DBL_MAX * 2.0;  // a rotation out of range: not evaluable
        const int act = ba_trust_decide(&S.T, solved != 0, 0.5 * (S.red[0] + S.pose_model), cand_cost,
                                        S.red[1] + S.pose_step2, S.red[2] + S.pose_x2);
        S.action = act;
        S.sum.iterations = it;
        if (act == BA_STEP_CONVERGED) S.sum.termination = BA_CONVERGENCE, S.done = 1;
        if (act == BA_STEP_ACCEPTED) S.sum.successful_steps++;
      }
      __syncthreads();
      if (S.action == BA_STEP_ACCEPTED) {
        for (int j = tid; j < N; j += BA_THREADS) {
#pragma unroll
          for (int k = 0; k < 3; k++) w.wp[(Q_X + k) * cap + j] = w.wp[(Q_CAND + k) * cap + j];
        }
        if (tid < 6 * W) S.x[tid] = S.cand[tid];
        if (tid < W) S.Px[tid] = S.Pc[tid];
        __syncthreads();
        ba_linearize<PRIOR>(w, S, false, &sum_rho, g_prior);
        if (tid == 0 && S.gmax <= BA_GRADIENT_TOL) S.sum.termination = BA_CONVERGENCE, S.done = 1;
      }
      if (tid == 0 && !S.done && S.T.radius <= BA_RADIUS_MIN) S.sum.termination = BA_CONVERGENCE, S.done = 1;
      __syncthreads();
    }
    // ---- outputs: the blocks are written back only on convergence (src/with_bundle_adjustment.cpp:683)
    if (S.sum.termination == BA_CONVERGENCE) {
      if (tid < 6 * W) g_pose[tid] = S.x[tid];
      for (int j = tid; j < N; j += BA_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; k++) g_pt[3 * j + k] = w.wp[(Q_X + k) * cap + j];
      }
    }
    if (tid == 0) {
      S.sum.final_cost = S.T.cost;
      out[win] = S.sum;
    }
  }
}

}  // namespace

hipError_t orbx_launch_ba(hipStream_t s, int n_windows, int groups, int max_iters, const double* K4, double delta,
                          const int32_t* d_pose_off, const int32_t* d_pt_off, const int32_t* d_obs_off,
                          double* d_poses, double* d_points, const int32_t* d_rows, const uint8_t* d_obs_pose,
                          const double* d_obs_xy, int cap, int ocap, double* d_ws_pt, double* d_ws_obs,
                          unsigned long long* d_ws_slot, void* d_out) {
  if (n_windows <= 0) return hipSuccess;
  if (groups < 1 || groups > n_windows || max_iters < 1 || max_iters > 1000 || cap < 1 || ocap < 1)
    return hipErrorInvalidValue;
  BaK4 K;
  for (int i = 0; i < 4; i++) K.k[i] = K4[i];
  hipLaunchKernelGGL(k_ba_lm<false>, dim3(groups), dim3(BA_THREADS), 0, s, n_windows, max_iters, K, delta, d_pose_off,
                     d_pt_off, d_obs_off, d_poses, d_points, d_rows, d_obs_pose, d_obs_xy, cap, ocap, d_ws_pt,
                     d_ws_obs, d_ws_slot, (BaSummary*)d_out, (const double*)nullptr, 0);
  return hipGetLastError();
}

// the same solve with landmark priors (rank 20): d_prior is [points][4] in the batch's point order, start an
// orbx_prior_start
hipError_t orbx_launch_ba_prior(hipStream_t s, int n_windows, int groups, int max_iters, const double* K4, double delta,
                                const int32_t* d_pose_off, const int32_t* d_pt_off, const int32_t* d_obs_off,
                                double* d_poses, double* d_points, const int32_t* d_rows, const uint8_t* d_obs_pose,
                                const double* d_obs_xy, int cap, int ocap, double* d_ws_pt, double* d_ws_obs,
                                unsigned long long* d_ws_slot, void* d_out, const double* d_prior, int start) {
  if (n_windows <= 0) return hipSuccess;
  if (groups < 1 || groups > n_windows || max_iters < 1 || max_iters > 1000 || cap < 1 || ocap < 1 || !d_prior ||
      (start != 0 && start != 1))
    return hipErrorInvalidValue;
  BaK4 K;
  for (int i = 0; i < 4; i++) K.k[i] = K4[i];
  hipLaunchKernelGGL(k_ba_lm<true>, dim3(groups), dim3(BA_THREADS), 0, s, n_windows, max_iters, K, delta, d_pose_off,
                     d_pt_off, d_obs_off, d_poses, d_points, d_rows, d_obs_pose, d_obs_xy, cap, ocap, d_ws_pt,
                     d_ws_obs, d_ws_slot, (BaSummary*)d_out, d_prior, start);
  return hipGetLastError();
}
