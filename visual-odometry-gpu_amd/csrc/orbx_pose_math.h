// orbx_pose_math.h -- the per-sample arithmetic of the relative-pose step
// (cv::findEssentialMat + cv::recoverPose, src/feature_matching.cpp:185-206,
// src/feature_tracking.cpp:222-242), shared by the gfx950 kernels
// (orbx_pose.hip) and host code.  Everything is binary64 built from IEEE
// + - * / and integer operations only (log and sqrt are restated below), so
// the same source compiled with -ffp-contract=off for gfx950 and for x86-64
// returns the same bits.  The rules are written out in DESIGN.md §9 (rank 5).
//
// Workspace convention: the solver keeps its arrays in a caller-provided
// workspace `w` of POSE_WS doubles, element i at w[i * S].  Host code passes
// S = 1; the kernel passes a lane's slice of LDS with S = lanes, so lanes read
// consecutive words.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ORBX_PHD __host__ __device__ __forceinline__
#else
#define ORBX_PHD static inline
#endif

#if defined(__clang__)
#define ORBX_PNO_CONTRACT _Pragma("clang fp contract(off)")
#define ORBX_PUNROLL _Pragma("unroll")
#else
#define ORBX_PNO_CONTRACT
#define ORBX_PUNROLL
#endif

#define POSE_MAX_MODELS 10
#define POSE_WS 296         // workspace doubles per sample (layout in pose_solve5)
#define POSE_WS_MODELS 36   // models (up to 10 x 9, row-major E) start here after a solve
#define POSE_DIST_THRESH 50.0
#define POSE_JACOBI_SWEEPS 10
#define POSE_ISOLATE_STEPS 64
#define POSE_REFINE_STEPS 64
#define POSE_MAX_DRAWS 4096
#define POSE_POLISH_STEPS 4
#define POSE_ESS_TOL 1e-10  // a unit-norm model is kept only if |det E| and |2EE^T E - tr(EE^T)E| are within this

ORBX_PHD uint64_t pose_d2u(double d) {
  uint64_t u;
  memcpy(&u, &d, 8);
  return u;
}
ORBX_PHD double pose_u2d(uint64_t u) {
  double d;
  memcpy(&d, &u, 8);
  return d;
}
ORBX_PHD double pose_abs(double x) { return x < 0 ? -x : x; }

// ---- sqrt: bit-halved exponent guess + 6 Newton steps (same bits on both sides) --
ORBX_PHD double pose_sqrt(double x) {
  ORBX_PNO_CONTRACT
  if (x != x) return x;
  if (x <= 0) return 0.0;
  if (x > 1.7976931348623157e308) return x;
  double scale = 1.0;
  if (x < 2.2250738585072014e-308) {  // subnormal: scale by 2^104, result by 2^-52
    x = x * 20282409603651670423947251286016.0;
    scale = 2.220446049250313e-16;
  }
  double y = pose_u2d((pose_d2u(x) >> 1) + 0x1ff8000000000000ull);
  for (int k = 0; k < 6; k++) y = 0.5 * (y + x / y);
  return y * scale;
}

// ---- log: fdlibm e_log.c's reduction and polynomial, for normal x > 0 ---------
ORBX_PHD double pose_log(double x) {
  ORBX_PNO_CONTRACT
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
               Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
               Lg7 = 1.479819860511658591e-01;
  const uint64_t b = pose_d2u(x);
  int k = (int)((b >> 52) & 0x7ff) - 1023;
  double m = pose_u2d((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull);  // [1, 2)
  if (m > 1.4142135623730951) {
    m = m * 0.5;  // exact
    k += 1;
  }
  const double f = m - 1.0;  // exact (Sterbenz)
  const double s = f / (2.0 + f);
  const double dk = (double)k;
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1;
  const double hfsq = 0.5 * f * f;
  if (k == 0) return f - (hfsq - s * (hfsq + R));
  return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

// ---- RANSACUpdateNumIters (pow(1 - ep, 5) as four products, cvRound as rint) ----
ORBX_PHD int pose_update_niters(double p, double ep, int max_iters) {
  ORBX_PNO_CONTRACT
  p = p < 0 ? 0.0 : (p > 1 ? 1.0 : p);
  ep = ep < 0 ? 0.0 : (ep > 1 ? 1.0 : ep);
  double num = 1.0 - p;
  if (num < 2.2250738585072014e-308) num = 2.2250738585072014e-308;
  const double q = 1.0 - ep;
  double denom = 1.0 - q * q * q * q * q;
  if (denom < 2.2250738585072014e-308) return 0;
  num = pose_log(num);
  denom = pose_log(denom);
  if (denom >= 0 || -num >= (double)max_iters * (-denom)) return max_iters;
  return (int)__builtin_rint(num / denom);
}

// ---- samples: integer counter hash of (seed, iteration, draw) ---------------
ORBX_PHD uint64_t pose_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
ORBX_PHD uint32_t pose_draw(uint64_t seed, uint32_t iter, uint32_t draw, uint32_t n) {
  const uint64_t h = pose_mix64(seed ^ pose_mix64(((uint64_t)iter << 32) | draw));
  return (uint32_t)(((h >> 32) * (uint64_t)n) >> 32);
}
// 5 distinct indices in [0, n) for RANSAC iteration `iter`; 0 if the draws run out
ORBX_PHD int pose_sample(uint64_t seed, uint32_t iter, uint32_t n, uint32_t idx[5]) {
  uint32_t draw = 0;
ORBX_PUNROLL
  for (int k = 0; k < 5; k++) {
    for (;;) {
      if (draw >= POSE_MAX_DRAWS) return 0;
      const uint32_t v = pose_draw(seed, iter, draw++, n);
      bool dup = false;
ORBX_PUNROLL
      for (int j = 0; j < k; j++) dup = dup || idx[j] == v;
      if (!dup) {
        idx[k] = v;
        break;
      }
    }
  }
  return 1;
}

// ---- score: EMEstimatorCallback::computeError, cast to float ----------------
ORBX_PHD float pose_sampson(const double* E, double x1, double y1, double x2, double y2) {
  ORBX_PNO_CONTRACT
  const double a = E[0] * x1 + E[1] * y1 + E[2];
  const double b = E[3] * x1 + E[4] * y1 + E[5];
  const double c = E[6] * x1 + E[7] * y1 + E[8];
  const double s2 = E[0] * x2 + E[3] * y2 + E[6];
  const double s1 = E[1] * x2 + E[4] * y2 + E[7];
  const double d = x2 * a + y2 * b + c;
  return (float)(d * d / (a * a + b * b + s2 * s2 + s1 * s1));
}

// ---- five-point solver -------------------------------------------------------
// Polynomials in (x, y, z).  Linear: [x, y, z, 1].  Quadratic: [x2, xy, xz, y2, yz, z2, x, y, z, 1].
// Cubic (the column order of the 10x20 system):
//   0 x3, 1 y3, 2 x2y, 3 xy2, 4 x2z, 5 x2, 6 y2z, 7 y2, 8 xyz, 9 xy,
//   10 xz2, 11 xz, 12 x, 13 yz2, 14 yz, 15 y, 16 z3, 17 z2, 18 z, 19 1
ORBX_PHD void pose_lin_mul(const double* a, const double* b, double* q) {
  ORBX_PNO_CONTRACT
  q[0] = a[0] * b[0];
  q[1] = a[0] * b[1] + a[1] * b[0];
  q[2] = a[0] * b[2] + a[2] * b[0];
  q[3] = a[1] * b[1];
  q[4] = a[1] * b[2] + a[2] * b[1];
  q[5] = a[2] * b[2];
  q[6] = a[0] * b[3] + a[3] * b[0];
  q[7] = a[1] * b[3] + a[3] * b[1];
  q[8] = a[2] * b[3] + a[3] * b[2];
  q[9] = a[3] * b[3];
}
// c (+)= q * b  (cubic)
ORBX_PHD void pose_quad_mul_acc(const double* q, const double* b, double* c, bool acc) {
  ORBX_PNO_CONTRACT
  double r[20];
  r[0] = q[0] * b[0];
  r[1] = q[3] * b[1];
  r[2] = q[0] * b[1] + q[1] * b[0];
  r[3] = q[1] * b[1] + q[3] * b[0];
  r[4] = q[0] * b[2] + q[2] * b[0];
  r[5] = q[0] * b[3] + q[6] * b[0];
  r[6] = q[3] * b[2] + q[4] * b[1];
  r[7] = q[3] * b[3] + q[7] * b[1];
  r[8] = q[1] * b[2] + q[2] * b[1] + q[4] * b[0];
  r[9] = q[1] * b[3] + q[6] * b[1] + q[7] * b[0];
  r[10] = q[2] * b[2] + q[5] * b[0];
  r[11] = q[2] * b[3] + q[6] * b[2] + q[8] * b[0];
  r[12] = q[6] * b[3] + q[9] * b[0];
  r[13] = q[4] * b[2] + q[5] * b[1];
  r[14] = q[4] * b[3] + q[7] * b[2] + q[8] * b[1];
  r[15] = q[7] * b[3] + q[9] * b[1];
  r[16] = q[5] * b[2];
  r[17] = q[5] * b[3] + q[8] * b[2];
  r[18] = q[8] * b[3] + q[9] * b[2];
  r[19] = q[9] * b[3];
ORBX_PUNROLL
  for (int i = 0; i < 20; i++) c[i] = acc ? c[i] + r[i] : r[i];
}

// ascending-coefficient univariate polynomials: r = a (deg da) * b (deg db)
template <int DA, int DB>
ORBX_PHD void pose_upoly_mul(const double* a, const double* b, double* r) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int i = 0; i <= DA + DB; i++) r[i] = 0.0;
ORBX_PUNROLL
  for (int i = 0; i <= DA; i++)
ORBX_PUNROLL
    for (int j = 0; j <= DB; j++) r[i + j] = r[i + j] + a[i] * b[j];
}

// Workspace layout (doubles, element i at w[i * S]):
//   [0, 36)    null-space basis X, Y, Z, W (E = xX + yY + zZ + W, row-major 3x3)
//   [36, 236)  10x20 constraint matrix; before it: the 9x5 QR input [36, 81), |v|^2 [81, 86), points [86, 106);
//              after it: Sturm sequence [36, 102), degrees [102, 113), division scratch [113, 124),
//              roots [226, 236), models [36, 126)
//   [236, 296) the 6 quadratics of E E^T; after elimination the 3x3 polynomial matrix [236, 275)
#define PW(i) w[(i) * S]

// Fills the points: x1[5], y1[5], x2[5], y2[5] at [86, 106) before calling pose_solve5.
template <int S>
ORBX_PHD void pose_put_point(double* w, int k, double x1, double y1, double x2, double y2) {
  PW(86 + k) = x1;
  PW(91 + k) = y1;
  PW(96 + k) = x2;
  PW(101 + k) = y2;
}

template <int S>
ORBX_PHD double pose_sturm_eval(const double* w, int k, double t) {
  ORBX_PNO_CONTRACT
  // poly k stored at offset 36 + k*11 - k*(k-1)/2, degree in [102 + k]
  const int off = 36 + k * 11 - (k * (k - 1)) / 2;
  const int d = (int)PW(102 + k);
  double v = PW(off + d);
  for (int i = d - 1; i >= 0; i--) v = v * t + PW(off + i);
  return v;
}
template <int S>
ORBX_PHD int pose_sturm_changes(const double* w, int nseq, double t) {
  int changes = 0;
  double prev = 0.0;
  for (int k = 0; k < nseq; k++) {
    const double v = pose_sturm_eval<S>(w, k, t);
    if (v != 0.0) {
      if ((prev < 0 && v > 0) || (prev > 0 && v < 0)) changes++;
      prev = v;
    }
  }
  return changes;
}

template <int S>
ORBX_PHD void pose_pmat_at(const double* w, double z, double row[3][3]) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int q = 0; q < 3; q++) {
    const int o = 236 + q * 13;
    row[q][0] = ((PW(o + 3) * z + PW(o + 2)) * z + PW(o + 1)) * z + PW(o + 0);
    row[q][1] = ((PW(o + 7) * z + PW(o + 6)) * z + PW(o + 5)) * z + PW(o + 4);
    row[q][2] = (((PW(o + 12) * z + PW(o + 11)) * z + PW(o + 10)) * z + PW(o + 9)) * z + PW(o + 8);
  }
}
template <int S>
ORBX_PHD double pose_pmat_det(const double* w, double z) {
  ORBX_PNO_CONTRACT
  double m[3][3];
  pose_pmat_at<S>(w, z, m);
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// ---- essential-matrix constraints of one E, and their derivative along a direction D ----
// r[0] = det E, r[1 + 3i + j] = (2 E E^T E - tr(E E^T) E)_ij
ORBX_PHD void pose_ess_residual(const double* E, double* r) {
  ORBX_PNO_CONTRACT
  double A[9];
ORBX_PUNROLL
  for (int i = 0; i < 3; i++)
ORBX_PUNROLL
    for (int j = 0; j < 3; j++)
      A[i * 3 + j] = E[i * 3 + 0] * E[j * 3 + 0] + E[i * 3 + 1] * E[j * 3 + 1] + E[i * 3 + 2] * E[j * 3 + 2];
  const double tr = A[0] + A[4] + A[8];
  r[0] = E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) + E[2] * (E[3] * E[7] - E[4] * E[6]);
ORBX_PUNROLL
  for (int i = 0; i < 3; i++)
ORBX_PUNROLL
    for (int j = 0; j < 3; j++)
      r[1 + i * 3 + j] = 2.0 * (A[i * 3 + 0] * E[0 * 3 + j] + A[i * 3 + 1] * E[1 * 3 + j] + A[i * 3 + 2] * E[2 * 3 + j]) -
                         tr * E[i * 3 + j];
}
ORBX_PHD void pose_ess_dir(const double* E, const double* D, double* dr) {
  ORBX_PNO_CONTRACT
  // d det = sum cof(E)_ij D_ij
  dr[0] = (E[4] * E[8] - E[5] * E[7]) * D[0] + (E[5] * E[6] - E[3] * E[8]) * D[1] + (E[3] * E[7] - E[4] * E[6]) * D[2] +
          (E[2] * E[7] - E[1] * E[8]) * D[3] + (E[0] * E[8] - E[2] * E[6]) * D[4] + (E[1] * E[6] - E[0] * E[7]) * D[5] +
          (E[1] * E[5] - E[2] * E[4]) * D[6] + (E[2] * E[3] - E[0] * E[5]) * D[7] + (E[0] * E[4] - E[1] * E[3]) * D[8];
  double A[9], dA[9];
ORBX_PUNROLL
  for (int i = 0; i < 3; i++)
ORBX_PUNROLL
    for (int j = 0; j < 3; j++) {
      A[i * 3 + j] = E[i * 3 + 0] * E[j * 3 + 0] + E[i * 3 + 1] * E[j * 3 + 1] + E[i * 3 + 2] * E[j * 3 + 2];
      dA[i * 3 + j] = D[i * 3 + 0] * E[j * 3 + 0] + D[i * 3 + 1] * E[j * 3 + 1] + D[i * 3 + 2] * E[j * 3 + 2] +
                      E[i * 3 + 0] * D[j * 3 + 0] + E[i * 3 + 1] * D[j * 3 + 1] + E[i * 3 + 2] * D[j * 3 + 2];
    }
  const double tr = A[0] + A[4] + A[8];
  double dtr = 0.0;
ORBX_PUNROLL
  for (int k = 0; k < 9; k++) dtr = dtr + E[k] * D[k];
  dtr = 2.0 * dtr;
ORBX_PUNROLL
  for (int i = 0; i < 3; i++)
ORBX_PUNROLL
    for (int j = 0; j < 3; j++)
      dr[1 + i * 3 + j] =
          2.0 * (dA[i * 3 + 0] * E[0 * 3 + j] + dA[i * 3 + 1] * E[1 * 3 + j] + dA[i * 3 + 2] * E[2 * 3 + j] +
                 A[i * 3 + 0] * D[0 * 3 + j] + A[i * 3 + 1] * D[1 * 3 + j] + A[i * 3 + 2] * D[2 * 3 + j]) -
          dtr * E[i * 3 + j] - tr * D[i * 3 + j];
}

// Nistér's five-point solver.  Returns the number of models (0..10), written to [36, 36 + 9n).
template <int S>
ORBX_PHD int pose_solve5(double* w) {
  ORBX_PNO_CONTRACT
  // 1. the 5x9 epipolar system, transposed into a 9x5 matrix A (column j = point j), at [36, 81) row-major
  for (int j = 0; j < 5; j++) {
    const double x1 = PW(86 + j), y1 = PW(91 + j), x2 = PW(96 + j), y2 = PW(101 + j);
    PW(36 + 0 * 5 + j) = x2 * x1;
    PW(36 + 1 * 5 + j) = x2 * y1;
    PW(36 + 2 * 5 + j) = x2;
    PW(36 + 3 * 5 + j) = y2 * x1;
    PW(36 + 4 * 5 + j) = y2 * y1;
    PW(36 + 5 * 5 + j) = y2;
    PW(36 + 6 * 5 + j) = x1;
    PW(36 + 7 * 5 + j) = y1;
    PW(36 + 8 * 5 + j) = 1.0;
  }
#define PA(r, c) PW(36 + (r) * 5 + (c))
  // 2. Householder QR of A; the last 4 columns of Q span the null space of the 5x9 system
  double colmax = 0.0;
  for (int j = 0; j < 5; j++) {
    double s = 0.0;
    for (int r = 0; r < 9; r++) s = s + PA(r, j) * PA(r, j);
    colmax = s > colmax ? s : colmax;
  }
  const double tol = 1e-12 * pose_sqrt(colmax);
  for (int k = 0; k < 5; k++) {
    double s = 0.0;
    for (int r = k; r < 9; r++) s = s + PA(r, k) * PA(r, k);
    const double nrm = pose_sqrt(s);
    if (!(nrm > tol)) return 0;  // rank-deficient sample
    const double x0 = PA(k, k);
    const double alpha = x0 > 0 ? -nrm : nrm;
    PA(k, k) = x0 - alpha;  // v (stored over column k, rows k..8)
    double vv = 0.0;
    for (int r = k; r < 9; r++) vv = vv + PA(r, k) * PA(r, k);
    PW(81 + k) = vv;
    for (int j = k + 1; j < 5; j++) {
      double d = 0.0;
      for (int r = k; r < 9; r++) d = d + PA(r, k) * PA(r, j);
      const double f = 2.0 * d / vv;
      for (int r = k; r < 9; r++) PA(r, j) = PA(r, j) - f * PA(r, k);
    }
  }
  for (int c = 0; c < 4; c++) {
    for (int r = 0; r < 9; r++) PW(c * 9 + r) = r == 5 + c ? 1.0 : 0.0;
    for (int k = 4; k >= 0; k--) {
      double d = 0.0;
      for (int r = k; r < 9; r++) d = d + PA(r, k) * PW(c * 9 + r);
      const double f = 2.0 * d / PW(81 + k);
      for (int r = k; r < 9; r++) PW(c * 9 + r) = PW(c * 9 + r) - f * PA(r, k);
    }
  }
#undef PA
  // 3. the 10 cubic constraints: det(E) = 0 and 2 E E^T E - tr(E E^T) E = 0
#define PM(r, c) PW(36 + (r) * 20 + (c))
  {
    double lin_a[4], lin_b[4], qa[10], qb[10], cub[20];
    // det E = E00 (E11 E22 - E12 E21) - E01 (E10 E22 - E12 E20) + E02 (E10 E21 - E11 E20)
    const int cof[3][5] = {{0, 4, 8, 5, 7}, {1, 3, 8, 5, 6}, {2, 3, 7, 4, 6}};
ORBX_PUNROLL
    for (int t = 0; t < 3; t++) {
ORBX_PUNROLL
      for (int i = 0; i < 4; i++) {
        lin_a[i] = PW(i * 9 + cof[t][1]);
        lin_b[i] = PW(i * 9 + cof[t][2]);
      }
      pose_lin_mul(lin_a, lin_b, qa);
ORBX_PUNROLL
      for (int i = 0; i < 4; i++) {
        lin_a[i] = PW(i * 9 + cof[t][3]);
        lin_b[i] = PW(i * 9 + cof[t][4]);
      }
      pose_lin_mul(lin_a, lin_b, qb);
ORBX_PUNROLL
      for (int i = 0; i < 10; i++) qa[i] = t == 1 ? qb[i] - qa[i] : qa[i] - qb[i];
ORBX_PUNROLL
      for (int i = 0; i < 4; i++) lin_a[i] = PW(i * 9 + cof[t][0]);
      pose_quad_mul_acc(qa, lin_a, cub, t > 0);
    }
ORBX_PUNROLL
    for (int i = 0; i < 20; i++) PM(0, i) = cub[i];
    // E E^T (symmetric; 6 quadratics at [236, 296): 00, 01, 02, 11, 12, 22), stored as 2 E E^T - tr I
    const int pr[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
ORBX_PUNROLL
    for (int e = 0; e < 6; e++) {
ORBX_PUNROLL
      for (int k = 0; k < 3; k++) {
ORBX_PUNROLL
        for (int i = 0; i < 4; i++) {
          lin_a[i] = PW(i * 9 + pr[e][0] * 3 + k);
          lin_b[i] = PW(i * 9 + pr[e][1] * 3 + k);
        }
        pose_lin_mul(lin_a, lin_b, qb);
ORBX_PUNROLL
        for (int i = 0; i < 10; i++) qa[i] = k == 0 ? qb[i] : qa[i] + qb[i];
      }
ORBX_PUNROLL
      for (int i = 0; i < 10; i++) PW(236 + e * 10 + i) = qa[i];
    }
    double tr[10];
ORBX_PUNROLL
    for (int i = 0; i < 10; i++) tr[i] = PW(236 + 0 * 10 + i) + PW(236 + 3 * 10 + i) + PW(236 + 5 * 10 + i);
ORBX_PUNROLL
    for (int e = 0; e < 6; e++) {
      const bool diag = e == 0 || e == 3 || e == 5;
ORBX_PUNROLL
      for (int i = 0; i < 10; i++) {
        const double v = 2.0 * PW(236 + e * 10 + i);
        PW(236 + e * 10 + i) = diag ? v - tr[i] : v;
      }
    }
    const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
ORBX_PUNROLL
    for (int i = 0; i < 3; i++)
ORBX_PUNROLL
      for (int j = 0; j < 3; j++) {
ORBX_PUNROLL
        for (int k = 0; k < 3; k++) {
ORBX_PUNROLL
          for (int m = 0; m < 10; m++) qa[m] = PW(236 + sym[i][k] * 10 + m);
ORBX_PUNROLL
          for (int m = 0; m < 4; m++) lin_a[m] = PW(m * 9 + k * 3 + j);
          pose_quad_mul_acc(qa, lin_a, cub, k > 0);
        }
ORBX_PUNROLL
        for (int m = 0; m < 20; m++) PM(1 + i * 3 + j, m) = cub[m];
      }
  }
  // 4. Gauss-Jordan with partial pivoting on the left 10x10 block
  double bmax = 0.0;
  for (int r = 0; r < 10; r++)
    for (int c = 0; c < 10; c++) {
      const double a = pose_abs(PM(r, c));
      bmax = a > bmax ? a : bmax;
    }
  const double ptol = 1e-12 * bmax;
  for (int c = 0; c < 10; c++) {
    int piv = c;
    double pmax = pose_abs(PM(c, c));
    for (int r = c + 1; r < 10; r++) {
      const double a = pose_abs(PM(r, c));
      if (a > pmax) {
        pmax = a;
        piv = r;
      }
    }
    if (!(pmax >= ptol) || pmax == 0.0) return 0;
    if (piv != c)
      for (int j = c; j < 20; j++) {
        const double t = PM(c, j);
        PM(c, j) = PM(piv, j);
        PM(piv, j) = t;
      }
    const double p = PM(c, c);
    for (int j = c + 1; j < 20; j++) PM(c, j) = PM(c, j) / p;
    PM(c, c) = 1.0;
    for (int r = 0; r < 10; r++) {
      if (r == c) continue;
      const double f = PM(r, c);
      for (int j = c + 1; j < 20; j++) PM(r, j) = PM(r, j) - f * PM(c, j);
      PM(r, c) = 0.0;
    }
  }
  // 5. the 3x3 polynomial matrix in z: rows <k> = z<x2> - <x2z>, <l> = z<y2> - <y2z>, <m> = z<xy> - <xyz>;
  //    each row: x-coefficient (cubic), y-coefficient (cubic), constant (quartic), ascending, 13 doubles
  {
    const int rows[3][2] = {{5, 4}, {7, 6}, {9, 8}};  // (row of m, row of m*z)
ORBX_PUNROLL
    for (int q = 0; q < 3; q++) {
      const int a = rows[q][0], b = rows[q][1];
      const int o = 236 + q * 13;
      // x: z (B_a[10] z^2 + B_a[11] z + B_a[12]) - (B_b[10] z^2 + B_b[11] z + B_b[12])
      PW(o + 0) = -PM(b, 12);
      PW(o + 1) = PM(a, 12) - PM(b, 11);
      PW(o + 2) = PM(a, 11) - PM(b, 10);
      PW(o + 3) = PM(a, 10);
      PW(o + 4) = -PM(b, 15);
      PW(o + 5) = PM(a, 15) - PM(b, 14);
      PW(o + 6) = PM(a, 14) - PM(b, 13);
      PW(o + 7) = PM(a, 13);
      PW(o + 8) = -PM(b, 19);
      PW(o + 9) = PM(a, 19) - PM(b, 18);
      PW(o + 10) = PM(a, 18) - PM(b, 17);
      PW(o + 11) = PM(a, 17) - PM(b, 16);
      PW(o + 12) = PM(a, 16);
    }
  }
#undef PM
  // 6. the degree-10 polynomial det(...) = kx (ly m1 - l1 my) - ky (lx m1 - l1 mx) + k1 (lx my - ly mx)
  {
    double kx[4], ky[4], k1[5], lx[4], ly[4], l1[5], mx[4], my[4], m1[5];
ORBX_PUNROLL
    for (int i = 0; i < 4; i++) {
      kx[i] = PW(236 + i);
      ky[i] = PW(236 + 4 + i);
      lx[i] = PW(249 + i);
      ly[i] = PW(249 + 4 + i);
      mx[i] = PW(262 + i);
      my[i] = PW(262 + 4 + i);
    }
ORBX_PUNROLL
    for (int i = 0; i < 5; i++) {
      k1[i] = PW(236 + 8 + i);
      l1[i] = PW(249 + 8 + i);
      m1[i] = PW(262 + 8 + i);
    }
    double c0[8], c1[8], c2[7], t7[8], t6[7], d[11], t10[11];
    pose_upoly_mul<3, 4>(ly, m1, c0);
    pose_upoly_mul<4, 3>(l1, my, t7);
ORBX_PUNROLL
    for (int i = 0; i < 8; i++) c0[i] = c0[i] - t7[i];
    pose_upoly_mul<3, 4>(lx, m1, c1);
    pose_upoly_mul<4, 3>(l1, mx, t7);
ORBX_PUNROLL
    for (int i = 0; i < 8; i++) c1[i] = c1[i] - t7[i];
    pose_upoly_mul<3, 3>(lx, my, c2);
    pose_upoly_mul<3, 3>(ly, mx, t6);
ORBX_PUNROLL
    for (int i = 0; i < 7; i++) c2[i] = c2[i] - t6[i];
    pose_upoly_mul<3, 7>(kx, c0, d);
    pose_upoly_mul<3, 7>(ky, c1, t10);
ORBX_PUNROLL
    for (int i = 0; i < 11; i++) d[i] = d[i] - t10[i];
    pose_upoly_mul<4, 6>(k1, c2, t10);
ORBX_PUNROLL
    for (int i = 0; i < 11; i++) PW(36 + i) = d[i] + t10[i];
  }
  // 7. Sturm sequence: p0 = det, p1 = p0', p(k+1) = -rem(p(k-1), p(k)); each scaled to a unit leading coefficient
  int deg = 10;
  while (deg > 0 && PW(36 + deg) == 0.0) deg--;
  if (deg == 0) return 0;
  {
    const double lead = pose_abs(PW(36 + deg));
    for (int i = 0; i <= deg; i++) PW(36 + i) = PW(36 + i) / lead;
  }
  PW(102) = (double)deg;
  int nseq = 1;
  {
    const int off1 = 36 + 11;
    for (int i = 0; i < deg; i++) PW(off1 + i) = (double)(i + 1) * PW(36 + i + 1);
    const double lead = pose_abs(PW(off1 + deg - 1));
    for (int i = 0; i < deg; i++) PW(off1 + i) = PW(off1 + i) / lead;
    PW(103) = (double)(deg - 1);
    nseq = 2;
  }
  while (nseq < 11) {
    const int ka = nseq - 2, kb = nseq - 1;
    const int oa = 36 + ka * 11 - (ka * (ka - 1)) / 2, ob = 36 + kb * 11 - (kb * (kb - 1)) / 2;
    const int on = 36 + nseq * 11 - (nseq * (nseq - 1)) / 2;
    const int da = (int)PW(102 + ka), db = (int)PW(102 + kb);
    if (db == 0) break;
    // remainder of a / b by long division, in the free words [113, 124)
    for (int i = 0; i < 11; i++) PW(113 + i) = i <= da ? PW(oa + i) : 0.0;
    const double lb = PW(ob + db);
    for (int i = da; i >= db; i--) {
      const double q = PW(113 + i) / lb;
      for (int j = 0; j <= db; j++) PW(113 + i - db + j) = PW(113 + i - db + j) - q * PW(ob + j);
    }
    int dr = db - 1;
    while (dr >= 0 && PW(113 + dr) == 0.0) dr--;
    if (dr < 0) break;  // exact division: p(k) is the gcd; the sequence ends
    const double lead = pose_abs(PW(113 + dr));
    for (int i = 0; i <= dr; i++) PW(on + i) = -PW(113 + i) / lead;
    PW(102 + nseq) = (double)dr;
    nseq++;
    if (dr == 0) break;
  }
  // 8. real roots inside the Cauchy bound: isolate root r by Sturm bisection, then fixed sign bisection
  double bound = 0.0;
  for (int i = 0; i < deg; i++) {
    const double a = pose_abs(PW(36 + i));  // leading coefficient is +-1
    bound = a > bound ? a : bound;
  }
  bound = bound + 1.0;
  const int vlo = pose_sturm_changes<S>(w, nseq, -bound), vhi = pose_sturm_changes<S>(w, nseq, bound);
  int nroots = vlo - vhi;
  if (nroots <= 0) return 0;
  if (nroots > 10) nroots = 10;
  for (int r = 0; r < nroots; r++) {
    double lo = -bound, hi = bound;
    int nlo = 0, nhi = nroots;  // roots <= lo, roots <= hi
    for (int s = 0; s < POSE_ISOLATE_STEPS && nhi - nlo > 1; s++) {
      const double mid = 0.5 * (lo + hi);
      const int nm = vlo - pose_sturm_changes<S>(w, nseq, mid);
      if (nm > r) {
        hi = mid;
        nhi = nm;
      } else {
        lo = mid;
        nlo = nm;
      }
    }
    // refinement on the sign of det(M(z)) evaluated from the matrix entries (no expanded coefficients)
    double plo = pose_pmat_det<S>(w, lo);
    for (int s = 0; s < POSE_REFINE_STEPS; s++) {
      const double mid = 0.5 * (lo + hi);
      const double pm = pose_pmat_det<S>(w, mid);
      if (pm == 0.0) {
        lo = hi = mid;
        break;
      }
      if ((pm < 0) == (plo < 0)) {
        lo = mid;
        plo = pm;
      } else {
        hi = mid;
      }
    }
    PW(226 + r) = 0.5 * (lo + hi);
  }
  // 9. back-substitution: (x, y, 1) is the null vector of the 3x3 matrix at z
  int nm = 0;
  for (int r = 0; r < nroots; r++) {
    const double z = PW(226 + r);
    double row[3][3];
    pose_pmat_at<S>(w, z, row);
    // the cross product of the pair of rows with the largest one (first pair on ties)
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, vn = -1.0;
ORBX_PUNROLL
    for (int pr = 0; pr < 3; pr++) {
      const int a = pr == 2 ? 1 : 0, b = pr == 0 ? 1 : 2;
      const double c0 = row[a][1] * row[b][2] - row[a][2] * row[b][1];
      const double c1 = row[a][2] * row[b][0] - row[a][0] * row[b][2];
      const double c2 = row[a][0] * row[b][1] - row[a][1] * row[b][0];
      const double cn = c0 * c0 + c1 * c1 + c2 * c2;
      if (cn > vn) {
        v0 = c0, v1 = c1, v2 = c2, vn = cn;
      }
    }
    if (v2 == 0.0 || v2 != v2) continue;
    // Gauss-Newton on the 10 cubic constraints in (x, y, z), E = xX + yY + zZ + W (fixed step count)
    double px = v0 / v2, py = v1 / v2, pz = z;
    double e[9], res[10], jx[10], jy[10], jz[10], dir[9];
    for (int it = 0; it < POSE_POLISH_STEPS; it++) {
ORBX_PUNROLL
      for (int i = 0; i < 9; i++) e[i] = px * PW(0 * 9 + i) + py * PW(1 * 9 + i) + pz * PW(2 * 9 + i) + PW(3 * 9 + i);
      pose_ess_residual(e, res);
ORBX_PUNROLL
      for (int i = 0; i < 9; i++) dir[i] = PW(0 * 9 + i);
      pose_ess_dir(e, dir, jx);
ORBX_PUNROLL
      for (int i = 0; i < 9; i++) dir[i] = PW(1 * 9 + i);
      pose_ess_dir(e, dir, jy);
ORBX_PUNROLL
      for (int i = 0; i < 9; i++) dir[i] = PW(2 * 9 + i);
      pose_ess_dir(e, dir, jz);
      double n00 = 0.0, n01 = 0.0, n02 = 0.0, n11 = 0.0, n12 = 0.0, n22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
ORBX_PUNROLL
      for (int k = 0; k < 10; k++) {
        n00 = n00 + jx[k] * jx[k];
        n01 = n01 + jx[k] * jy[k];
        n02 = n02 + jx[k] * jz[k];
        n11 = n11 + jy[k] * jy[k];
        n12 = n12 + jy[k] * jz[k];
        n22 = n22 + jz[k] * jz[k];
        g0 = g0 + jx[k] * res[k];
        g1 = g1 + jy[k] * res[k];
        g2 = g2 + jz[k] * res[k];
      }
      const double c00 = n11 * n22 - n12 * n12, c01 = n12 * n02 - n01 * n22, c02 = n01 * n12 - n11 * n02;
      const double dt = n00 * c00 + n01 * c01 + n02 * c02;
      if (!(dt != 0.0) || dt != dt) break;
      const double d0 = g0 * c00 + n01 * (n12 * g2 - g1 * n22) + n02 * (g1 * n12 - n11 * g2);
      const double d1 = n00 * (g1 * n22 - n12 * g2) + g0 * c01 + n02 * (n01 * g2 - g1 * n02);
      const double d2 = n00 * (n11 * g2 - g1 * n12) + n01 * (g1 * n02 - n01 * g2) + g0 * c02;
      const double sx = d0 / dt, sy = d1 / dt, sz = d2 / dt;
      if (sx != sx || sy != sy || sz != sz) break;
      px = px - sx;
      py = py - sy;
      pz = pz - sz;
    }
    double n2 = 0.0;
ORBX_PUNROLL
    for (int i = 0; i < 9; i++) {
      e[i] = px * PW(0 * 9 + i) + py * PW(1 * 9 + i) + pz * PW(2 * 9 + i) + PW(3 * 9 + i);
      n2 = n2 + e[i] * e[i];
    }
    if (!(n2 > 0.0) || n2 > 1.7976931348623157e308) continue;
    const double nrm = pose_sqrt(n2);
ORBX_PUNROLL
    for (int i = 0; i < 9; i++) e[i] = e[i] / nrm;
    // keep only models that are essential matrices to POSE_ESS_TOL (spurious roots of an ill-conditioned sample
    // do not converge and are dropped)
    pose_ess_residual(e, res);
    double f2 = 0.0;
ORBX_PUNROLL
    for (int k = 1; k < 10; k++) f2 = f2 + res[k] * res[k];
    if (!(pose_abs(res[0]) <= POSE_ESS_TOL) || !(f2 <= POSE_ESS_TOL * POSE_ESS_TOL)) continue;
ORBX_PUNROLL
    for (int i = 0; i < 9; i++) PW(POSE_WS_MODELS + nm * 9 + i) = e[i];
    nm++;
  }
  return nm;
}
#undef PW

// ---- recoverPose: decomposeEssentialMat + cheirality -------------------------
// E = U diag(s1, s2, 0) V^T from Jacobi on E^T E (fixed sweeps); det V > 0 (V negated otherwise),
// u1 = E v1 / |E v1|, u2 = Gram-Schmidt(E v2), u3 = u1 x u2 (so det U = +1).
// R1 = U W V^T, R2 = U W^T V^T, t = u3.  Returns 0 if E is degenerate.
ORBX_PHD int pose_decompose(const double* E, double* R1, double* R2, double* t) {
  ORBX_PNO_CONTRACT
  double a[3][3], v[3][3];
ORBX_PUNROLL
  for (int i = 0; i < 3; i++)
ORBX_PUNROLL
    for (int j = 0; j < 3; j++) {
      a[i][j] = E[0 * 3 + i] * E[0 * 3 + j] + E[1 * 3 + i] * E[1 * 3 + j] + E[2 * 3 + i] * E[2 * 3 + j];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sw = 0; sw < POSE_JACOBI_SWEEPS; sw++) {
ORBX_PUNROLL
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double at = pose_abs(theta);
      double tt = at > 1e150 ? 0.5 / at : 1.0 / (at + pose_sqrt(theta * theta + 1.0));
      if (theta < 0) tt = -tt;
      const double c = 1.0 / pose_sqrt(tt * tt + 1.0), s = tt * c;
      const double app = a[p][p] - tt * apq, aqq = a[q][q] + tt * apq;
      const double arp = c * a[r][p] - s * a[r][q], arq = s * a[r][p] + c * a[r][q];
      a[p][p] = app;
      a[q][q] = aqq;
      a[p][q] = a[q][p] = 0.0;
      a[r][p] = a[p][r] = arp;
      a[r][q] = a[q][r] = arq;
ORBX_PUNROLL
      for (int i = 0; i < 3; i++) {
        const double vp = c * v[i][p] - s * v[i][q], vq = s * v[i][p] + c * v[i][q];
        v[i][p] = vp;
        v[i][q] = vq;
      }
    }
  }
  // eigenvalues descending (stable compare-exchange network on columns)
  double d[3] = {a[0][0], a[1][1], a[2][2]};
ORBX_PUNROLL
  for (int st = 0; st < 3; st++) {
    const int i = st == 1 ? 1 : 0, j = i + 1;
    if (d[j] > d[i]) {
      const double td = d[i];
      d[i] = d[j];
      d[j] = td;
ORBX_PUNROLL
      for (int k = 0; k < 3; k++) {
        const double tv = v[k][i];
        v[k][i] = v[k][j];
        v[k][j] = tv;
      }
    }
  }
  const double detv = v[0][2] * (v[1][0] * v[2][1] - v[2][0] * v[1][1]) - v[1][2] * (v[0][0] * v[2][1] - v[2][0] * v[0][1]) +
                      v[2][2] * (v[0][0] * v[1][1] - v[1][0] * v[0][1]);
  if (detv < 0)
ORBX_PUNROLL
    for (int i = 0; i < 3; i++)
ORBX_PUNROLL
      for (int j = 0; j < 3; j++) v[i][j] = -v[i][j];
  double u[3][3];  // columns u1, u2, u3
  double n1 = 0.0;
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
    u[i][0] = E[i * 3 + 0] * v[0][0] + E[i * 3 + 1] * v[1][0] + E[i * 3 + 2] * v[2][0];
    n1 = n1 + u[i][0] * u[i][0];
  }
  if (!(n1 > 0.0)) return 0;
  n1 = pose_sqrt(n1);
  double dot = 0.0;
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
    u[i][0] = u[i][0] / n1;
    u[i][1] = E[i * 3 + 0] * v[0][1] + E[i * 3 + 1] * v[1][1] + E[i * 3 + 2] * v[2][1];
    dot = dot + u[i][0] * u[i][1];
  }
  double n2 = 0.0;
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
    u[i][1] = u[i][1] - dot * u[i][0];
    n2 = n2 + u[i][1] * u[i][1];
  }
  if (!(n2 > 0.0)) return 0;
  n2 = pose_sqrt(n2);
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) u[i][1] = u[i][1] / n2;
  u[0][2] = u[1][0] * u[2][1] - u[2][0] * u[1][1];
  u[1][2] = u[2][0] * u[0][1] - u[0][0] * u[2][1];
  u[2][2] = u[0][0] * u[1][1] - u[1][0] * u[0][1];
  // U W = [-u2, u1, u3], U W^T = [u2, -u1, u3]
ORBX_PUNROLL
  for (int i = 0; i < 3; i++)
ORBX_PUNROLL
    for (int j = 0; j < 3; j++) {
      R1[i * 3 + j] = -u[i][1] * v[j][0] + u[i][0] * v[j][1] + u[i][2] * v[j][2];
      R2[i * 3 + j] = u[i][1] * v[j][0] - u[i][0] * v[j][1] + u[i][2] * v[j][2];
    }
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) t[i] = u[i][2];
  return 1;
}

// Linear least-squares triangulation (3x3 normal equations, Cramer's rule) of one correspondence under
// P1 = [I | 0], P2 = [R | sgn*t]; good iff 0 < depth < 50 in both cameras.
ORBX_PHD bool pose_point_good(const double* R, const double* t, double sgn, double x1, double y1, double x2,
                              double y2) {
  ORBX_PNO_CONTRACT
  const double t0 = sgn * t[0], t1 = sgn * t[1], t2 = sgn * t[2];
  double A[4][3], b[4];
  A[0][0] = 1.0, A[0][1] = 0.0, A[0][2] = -x1, b[0] = 0.0;
  A[1][0] = 0.0, A[1][1] = 1.0, A[1][2] = -y1, b[1] = 0.0;
ORBX_PUNROLL
  for (int j = 0; j < 3; j++) {
    A[2][j] = R[0 * 3 + j] - x2 * R[2 * 3 + j];
    A[3][j] = R[1 * 3 + j] - y2 * R[2 * 3 + j];
  }
  b[2] = x2 * t2 - t0;
  b[3] = y2 * t2 - t1;
  double N[3][3], r[3];
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
ORBX_PUNROLL
    for (int j = 0; j < 3; j++) N[i][j] = A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j] + A[3][i] * A[3][j];
    r[i] = A[0][i] * b[0] + A[1][i] * b[1] + A[2][i] * b[2] + A[3][i] * b[3];
  }
  const double c00 = N[1][1] * N[2][2] - N[1][2] * N[2][1];
  const double c01 = N[1][2] * N[2][0] - N[1][0] * N[2][2];
  const double c02 = N[1][0] * N[2][1] - N[1][1] * N[2][0];
  const double det = N[0][0] * c00 + N[0][1] * c01 + N[0][2] * c02;
  if (det == 0.0) return false;
  // Cramer: X_k = det(N with column k replaced by r) / det
  const double d0 = r[0] * c00 + N[0][1] * (N[1][2] * r[2] - r[1] * N[2][2]) + N[0][2] * (r[1] * N[2][1] - N[1][1] * r[2]);
  const double d1 = N[0][0] * (r[1] * N[2][2] - N[1][2] * r[2]) + r[0] * c01 + N[0][2] * (N[1][0] * r[2] - r[1] * N[2][0]);
  const double d2 = N[0][0] * (N[1][1] * r[2] - r[1] * N[2][1]) + N[0][1] * (r[1] * N[2][0] - N[1][0] * r[2]) + r[0] * c02;
  const double X0 = d0 / det, X1 = d1 / det, X2 = d2 / det;
  const double z2 = R[6] * X0 + R[7] * X1 + R[8] * X2 + t2;
  return X2 > 0.0 && X2 < POSE_DIST_THRESH && z2 > 0.0 && z2 < POSE_DIST_THRESH;
}
