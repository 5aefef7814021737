// orbx_pnp_math.h -- the arithmetic of perspective-n-point with RANSAC (cv::solvePnPRansac; the reference calls none):
// the P3P minimal solver, the three-index sampler, the reprojection score, the iteration update and the
// Levenberg-Marquardt refinement of the six pose parameters.  Shared by the gfx950 kernel (orbx_pnp.hip), the host
// layer and the sequential restatement (tests/cpp/pnp_sequential.cpp).  Binary64 built from IEEE + - * /, integer
// operations, pose_sqrt, ba_sincos and wp_* only, so the same source compiled with -ffp-contract=off for gfx950 and
// for x86-64 returns the same bits.  The rules are DESIGN.md §9 (rank 17).
#pragma once
#include "orbx_ba_math.h"
#include "orbx_wp_math.h"

// = include/orbx_pnp.h: orbx_pnp_status
enum { PNP_OK = 0, PNP_SKIPPED = 1, PNP_FEW_POINTS = 2, PNP_NO_MODEL = 3 };

#define PNP_MAX_MODELS 4      // solutions of one sample
#define PNP_MODEL_DOUBLES 12  // a model: R row-major, then t (world -> camera)
#define PNP_BISECT_STEPS 60   // halvings of a bracket inside [0, 1]: its width ends at 2^-60
#define PNP_POLISH_STEPS 2    // Newton steps on a bisected root
#define PNP_MAX_REFINE 20     // = include/orbx_pnp.h: the largest refine_iters
#define PNP_LANES 256         // lanes of the summation rule (rule 9): the kernel's workgroup size
#define PNP_NSUM 28           // sums of one refinement pass: ba_accum_pose's 27, then the cost
#define PNP_LAMBDA0 1e-3
#define PNP_LAMBDA_MIN 1e-12
#define PNP_LAMBDA_MAX 1e12
#define PNP_DIAG_MIN 1e-6
#define PNP_NO_HUBER 1e150    // the scale handed to ba_obs_eval: every residual is on the squared branch

// ---- polynomials of degree <= 4, coefficients ascending, padded with zeros to 5 -----------------------------------
ORBX_PHD double pnp_poly(const double* c, double x) {
  ORBX_PNO_CONTRACT
  return (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0];
}
ORBX_PHD void pnp_poly_deriv(const double* c, double* d) {
  ORBX_PNO_CONTRACT
  d[0] = c[1], d[1] = 2.0 * c[2], d[2] = 3.0 * c[3], d[3] = 4.0 * c[4], d[4] = 0.0;
}
// the root inside [lo, hi] when c has opposite signs at the ends (rising: c(hi) > 0): PNP_BISECT_STEPS halvings
ORBX_PHD double pnp_bisect(const double* c, double lo, double hi, bool rising) {
  ORBX_PNO_CONTRACT
  for (int i = 0; i < PNP_BISECT_STEPS; i++) {
    const double mid = 0.5 * (lo + hi);
    const double f = pnp_poly(c, mid);
    if (rising ? f > 0.0 : f < 0.0) hi = mid;
    else lo = mid;
  }
  return 0.5 * (lo + hi);
}
// The roots of c on the pieces br[0] < br[1] < ... < br[nb - 1] (nb <= 5), at most one per piece, ascending: piece
// [a, b] holds the root b when c(b) == 0, else a bisected one when c(a) and c(b) have strictly opposite signs.  A
// piece that is not ascending is skipped.
ORBX_PHD int pnp_roots_on_pieces(const double* c, const double* br, int nb, double* out) {
  ORBX_PNO_CONTRACT
  int n = 0;
  double a = br[0], fa = pnp_poly(c, a);
  for (int i = 1; i < 5; i++) {
    if (i >= nb) break;
    const double b = br[i];
    if (!(b > a)) continue;
    const double fb = pnp_poly(c, b);
    if (fb == 0.0) out[n++] = b;
    else if ((fa < 0.0 && fb > 0.0) || (fa > 0.0 && fb < 0.0)) out[n++] = pnp_bisect(c, a, b, fb > 0.0);
    a = b, fa = fb;
  }
  return n;
}
// The real roots of the quartic c in (0, 1], ascending, at most 4, through its derivatives: the roots of c'' (closed
// form) cut [0, 1] into pieces on which c' is monotone, the roots of c' found there cut it into pieces on which c is
// monotone.  A root counts as real iff c changes sign strictly across its piece (or is exactly zero at the piece's
// upper end): a double root, where c only touches zero, is no root.  Each root is polished by PNP_POLISH_STEPS Newton
// steps; a step is taken only if it stays in (0, 1].
ORBX_PHD int pnp_quartic_unit_roots(const double* c, double* roots) {
  ORBX_PNO_CONTRACT
  double d1[5], d2[5], br[5], cr[6];
  pnp_poly_deriv(c, d1);
  pnp_poly_deriv(d1, d2);
  int nb = 0;
  br[nb++] = 0.0;
  const double qa = d2[2], qb = d2[1], qc = d2[0];
  if (qa != 0.0) {
    const double disc = qb * qb - 4.0 * qa * qc;
    if (disc > 0.0) {
      const double s = pose_sqrt(disc);
      double r1 = (-qb - s) / (2.0 * qa), r2 = (-qb + s) / (2.0 * qa);
      if (r1 > r2) {
        const double t = r1;
        r1 = r2, r2 = t;
      }
      if (r1 > 0.0 && r1 < 1.0) br[nb++] = r1;
      if (r2 > 0.0 && r2 < 1.0 && r2 > r1) br[nb++] = r2;
    }
  } else if (qb != 0.0) {
    const double r = -qc / qb;
    if (r > 0.0 && r < 1.0) br[nb++] = r;
  }
  br[nb++] = 1.0;
  cr[0] = 0.0;
  int nc = 1 + pnp_roots_on_pieces(d1, br, nb, cr + 1);
  cr[nc++] = 1.0;
  const int n = pnp_roots_on_pieces(c, cr, nc, roots);
  for (int i = 0; i < 4; i++) {
    if (i >= n) break;
    double x = roots[i];
    for (int k = 0; k < PNP_POLISH_STEPS; k++) {
      const double f = pnp_poly(c, x), d = pnp_poly(d1, x);
      const double xn = x - f / d;
      if (xn > 0.0 && xn <= 1.0) x = xn;  // (a NaN or an infinite step fails the test)
    }
    roots[i] = x;
  }
  return n;
}
// a (degree da) times b (degree db), da + db <= 4, into r[0 .. 4]; each coefficient summed in ascending index of a
ORBX_PHD void pnp_poly_mul(const double* a, int da, const double* b, int db, double* r) {
  ORBX_PNO_CONTRACT
  for (int k = 0; k < 5; k++) {
    double s = 0.0;
    for (int i = 0; i <= da; i++) {
      const int j = k - i;
      if (j >= 0 && j <= db) s = s + a[i] * b[j];
    }
    r[k] = s;
  }
}

ORBX_PHD void pnp_cross(const double* a, const double* b, double* c) {
  ORBX_PNO_CONTRACT
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}
// the right-handed orthonormal triad of the triangle (p0, p1, p2): e1 along p1 - p0, e3 along its normal, e2 = e3 x e1,
// as the rows of e; false when the squared length of an edge or of the normal is not > 0
ORBX_PHD bool pnp_triad(const double* p0, const double* p1, const double* p2, double* e) {
  ORBX_PNO_CONTRACT
  const double d1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double d2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  double n[3];
  pnp_cross(d1, d2, n);
  const double l1 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2], ln = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  if (!(l1 > 0.0) || !(ln > 0.0)) return false;
  const double s1 = pose_sqrt(l1), sn = pose_sqrt(ln);
  for (int i = 0; i < 3; i++) e[i] = d1[i] / s1, e[6 + i] = n[i] / sn;
  pnp_cross(e + 6, e, e + 3);
  return true;
}

// ---- P3P: Grunert's distance equations, reduced to one quartic in v = s2 / s0 -------------------------------------
// X: three world points (9 doubles); xy: their normalised image points (6 doubles).  With unit bearings j_i, distances
// s_i along them, s1 = u s0, s2 = v s0 and the squared side lengths a2 = |X1 - X2|^2, b2 = |X0 - X2|^2,
// c2 = |X0 - X1|^2 the law of cosines gives two conics in (u, v); their difference is linear in u:
//   u = N(v) / D(v),  N = (k - 1) v^2 - 2 k cb v + (1 + k),  D = 2 (cg - ca v),  k = (a2 - c2) / b2
// and the second conic becomes  N^2 - 2 cg N D + (1 - m q) D^2 = 0,  q = 1 - 2 cb v + v^2,  m = c2 / b2,
// formed by polynomial products.  Positive roots only (s2 > 0): those in (0, 1] of the quartic, then the reciprocals
// of those in (0, 1) of its reversal, which puts the solutions in ascending v.  Per root: s0^2 = b2 / q, the camera
// points s_i j_i, R from the triads of the two triangles, t = C0 - R X0.  Dropped: a root with s0^2, s1 or s2 not
// > 0, a camera triangle without a triad, a model with an entry that is not finite, a model that puts a sample point
// at a depth that is not > 0.  No solutions at all: b2 not > 0 or collinear world points (no triad).
// models: PNP_MAX_MODELS x PNP_MODEL_DOUBLES; returns the number of models.
ORBX_PHD int pnp_p3p(const double* X, const double* xy, double* models) {
  ORBX_PNO_CONTRACT
  double j[9], ew[9];
  for (int i = 0; i < 3; i++) {
    const double x = xy[2 * i], y = xy[2 * i + 1];
    const double n = pose_sqrt(x * x + y * y + 1.0);
    j[3 * i] = x / n, j[3 * i + 1] = y / n, j[3 * i + 2] = 1.0 / n;
  }
  if (!pnp_triad(X, X + 3, X + 6, ew)) return 0;
  const double ca = j[3] * j[6] + j[4] * j[7] + j[5] * j[8];
  const double cb = j[0] * j[6] + j[1] * j[7] + j[2] * j[8];
  const double cg = j[0] * j[3] + j[1] * j[4] + j[2] * j[5];
  double a2 = 0.0, b2 = 0.0, c2 = 0.0;
  for (int i = 0; i < 3; i++) {
    const double da = X[3 + i] - X[6 + i], db = X[i] - X[6 + i], dc = X[i] - X[3 + i];
    a2 = a2 + da * da, b2 = b2 + db * db, c2 = c2 + dc * dc;
  }
  if (!(b2 > 0.0)) return 0;
  const double k = (a2 - c2) / b2, m = c2 / b2;
  const double N[3] = {1.0 + k, -2.0 * k * cb, k - 1.0};
  const double D[2] = {2.0 * cg, -2.0 * ca};
  const double Q[3] = {1.0 - m, 2.0 * m * cb, -m};  // 1 - m q
  double N2[5], ND[5], D2[5], QD2[5], c[5], rev[5];
  pnp_poly_mul(N, 2, N, 2, N2);
  pnp_poly_mul(N, 2, D, 1, ND);
  pnp_poly_mul(D, 1, D, 1, D2);
  pnp_poly_mul(Q, 2, D2, 2, QD2);
  for (int i = 0; i < 5; i++) c[i] = (N2[i] - 2.0 * cg * ND[i]) + QD2[i];
  for (int i = 0; i < 5; i++) rev[i] = c[4 - i];
  double v[8], w[4];
  int nv = pnp_quartic_unit_roots(c, v);
  const int nw = pnp_quartic_unit_roots(rev, w);
  for (int i = nw - 1; i >= 0; i--)
    if (w[i] < 1.0) v[nv++] = 1.0 / w[i];
  int nm = 0;
  for (int r = 0; r < 8; r++) {
    if (r >= nv || nm >= PNP_MAX_MODELS) break;
    const double vv = v[r];
    const double u = ((N[2] * vv + N[1]) * vv + N[0]) / (D[1] * vv + D[0]);
    const double q = (vv - 2.0 * cb) * vv + 1.0;
    const double s0sq = b2 / q;
    if (!(s0sq > 0.0)) continue;
    const double s0 = pose_sqrt(s0sq), s1 = u * s0, s2 = vv * s0;
    if (!(s1 > 0.0) || !(s2 > 0.0)) continue;
    double C[9], ec[9];
    for (int i = 0; i < 3; i++) C[i] = s0 * j[i], C[3 + i] = s1 * j[3 + i], C[6 + i] = s2 * j[6 + i];
    if (!pnp_triad(C, C + 3, C + 6, ec)) continue;
    double* M = models + nm * PNP_MODEL_DOUBLES;
    bool ok = true;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        M[3 * a + b] = (ec[a] * ew[b] + ec[3 + a] * ew[3 + b]) + ec[6 + a] * ew[6 + b];
        ok = ok && wp_finite(M[3 * a + b]);
      }
    for (int a = 0; a < 3; a++) {
      M[9 + a] = C[a] - ((M[3 * a] * X[0] + M[3 * a + 1] * X[1]) + M[3 * a + 2] * X[2]);
      ok = ok && wp_finite(M[9 + a]);
    }
    for (int i = 0; i < 3; i++) {
      const double z = ((M[6] * X[3 * i] + M[7] * X[3 * i + 1]) + M[8] * X[3 * i + 2]) + M[11];
      ok = ok && z > 0.0;
    }
    if (ok) nm++;
  }
  return nm;
}

// ---- sampler: pose_sample's rejection rule with three indices ------------------------------------------------------
ORBX_PHD int pnp_sample3(uint64_t seed, uint32_t iter, uint32_t n, uint32_t idx[3]) {
  uint32_t draw = 0;
ORBX_PUNROLL
  for (int k = 0; k < 3; k++) {
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
// the seed of problem (window w, frame k) of a batch: a function of the frame alone, so that a window's result does
// not depend on its place in the batch
ORBX_PHD uint64_t pnp_problem_seed(uint64_t seed, uint32_t k) { return pose_mix64(seed ^ pose_mix64((uint64_t)k)); }

// ---- score: THE inlier comparison, written down once ---------------------------------------------------------------
// M: a model; K4 = fx, fy, cx, cy; thr2 = threshold_px * threshold_px in binary64.  p = R X + t, each row summed left
// to right; inlier iff p[2] > 0 and e2 = (fx p0 / p2 + cx - ox)^2 + (fy p1 / p2 + cy - oy)^2 <= thr2.  *e2 is written
// whenever p[2] > 0.
ORBX_PHD bool pnp_inlier(const double* K4, const double* M, const double* X, double ox, double oy, double thr2,
                         double* e2) {
  ORBX_PNO_CONTRACT
  const double p0 = ((M[0] * X[0] + M[1] * X[1]) + M[2] * X[2]) + M[9];
  const double p1 = ((M[3] * X[0] + M[4] * X[1]) + M[5] * X[2]) + M[10];
  const double p2 = ((M[6] * X[0] + M[7] * X[1]) + M[8] * X[2]) + M[11];
  if (!(p2 > 0.0)) return false;
  const double r0 = (K4[0] * p0 / p2 + K4[2]) - ox, r1 = (K4[1] * p1 / p2 + K4[3]) - oy;
  *e2 = r0 * r0 + r1 * r1;
  return *e2 <= thr2;
}

// ---- pose_update_niters with exponent 3 ----------------------------------------------------------------------------
ORBX_PHD int pnp_update_niters(double p, double ep, int max_iters) {
  ORBX_PNO_CONTRACT
  p = p < 0 ? 0.0 : (p > 1 ? 1.0 : p);
  ep = ep < 0 ? 0.0 : (ep > 1 ? 1.0 : ep);
  double num = 1.0 - p;
  if (num < 2.2250738585072014e-308) num = 2.2250738585072014e-308;
  const double q = 1.0 - ep;
  double denom = 1.0 - q * q * q;
  if (denom < 2.2250738585072014e-308) return 0;
  num = pose_log(num);
  denom = pose_log(denom);
  if (denom >= 0 || -num >= (double)max_iters * (-denom)) return max_iters;
  return (int)__builtin_rint(num / denom);
}

// ---- a model <-> the 6-double block (angle-axis, t) ------------------------------------------------------------------
ORBX_PHD void pnp_model_to_pose6(const double* M, double* pose6) {
  wp_rodrigues_inv(M, pose6);
  pose6[3] = M[9], pose6[4] = M[10], pose6[5] = M[11];
}
// the model of a prepared pose: the rotation of the branch ba_pose_prepare took
ORBX_PHD void pnp_pose_to_model(const BaPose& P, double* M) {
  for (int i = 0; i < 9; i++) M[i] = P.R[i];
  M[9] = P.t[0], M[10] = P.t[1], M[11] = P.t[2];
}

// ---- refinement: Levenberg-Marquardt on the six pose parameters, squared loss ----------------------------------------
// one inlier's share of a pass at the prepared pose P: acc[0, 27) as ba_accum_pose has them, acc[27] += |r|^2, or +inf
// when the point's depth is not > 0
ORBX_PHD void pnp_refine_term(const double* K4, const BaPose& P, const double* X, double ox, double oy, double* acc) {
  ORBX_PNO_CONTRACT
  BaObs o;
  ba_obs_eval(K4, P, X, ox, oy, PNP_NO_HUBER, false, &o);
  ba_accum_pose(o, acc);
  const double e = o.r[0] * o.r[0] + o.r[1] * o.r[1];
  acc[27] = acc[27] + (o.z > 0.0 ? e : pose_u2d(0x7ff0000000000000ull));
}
struct PnpLm {
  double x[6], cand[6], acc[PNP_NSUM];  // the pose, the candidate, the sums of the pass at x
  double lambda;
};
// the candidate of the sums at x: (H + lambda max(diag H, PNP_DIAG_MIN)) step = -g by ba_cholesky_solve; false when
// the system cannot be factored or the candidate is not finite (the refinement ends there)
ORBX_PHD bool pnp_lm_propose(PnpLm* S) {
  ORBX_PNO_CONTRACT
  double A[36], b[6];
  int k = 0;
  for (int a = 0; a < 6; a++)
    for (int c = 0; c <= a; c++, k++) A[a * 6 + c] = S->acc[k], A[c * 6 + a] = S->acc[k];
  for (int a = 0; a < 6; a++) {
    const double d = A[a * 6 + a];
    A[a * 6 + a] = d + S->lambda * (d > PNP_DIAG_MIN ? d : PNP_DIAG_MIN);
    b[a] = -S->acc[21 + a];
  }
  if (!ba_cholesky_solve(6, 6, A, b)) return false;
  bool fin = true;
  for (int a = 0; a < 6; a++) {
    S->cand[a] = S->x[a] + b[a];
    fin = fin && wp_finite(S->cand[a]);
  }
  return fin;
}
// the sums of the pass at the candidate: it is taken iff its cost is strictly below the cost at x (a NaN is not);
// taken: lambda / 10, refused: lambda * 10, inside [PNP_LAMBDA_MIN, PNP_LAMBDA_MAX]
ORBX_PHD void pnp_lm_decide(PnpLm* S, const double* cacc) {
  ORBX_PNO_CONTRACT
  if (cacc[27] < S->acc[27]) {
    for (int a = 0; a < 6; a++) S->x[a] = S->cand[a];
    for (int a = 0; a < PNP_NSUM; a++) S->acc[a] = cacc[a];
    const double l = S->lambda * 0.1;
    S->lambda = l < PNP_LAMBDA_MIN ? PNP_LAMBDA_MIN : l;
  } else {
    const double l = S->lambda * 10.0;
    S->lambda = l > PNP_LAMBDA_MAX ? PNP_LAMBDA_MAX : l;
  }
}
