// orbx_ba_math.h -- the arithmetic of sliding-window bundle adjustment
// (src/with_bundle_adjustment.cpp: ReprojectionError :27-68, run_bundle_adjustment :577-722), shared by the gfx950
// kernel (orbx_ba.hip) and the sequential restatement (tests/cpp/ba_sequential.cpp).  Binary64 built from IEEE
// + - * / and integer operations only (sin, cos are restated below, sqrt is pose_sqrt), so the same source compiled
// with -ffp-contract=off for gfx950 and for x86-64 returns the same bits.  The rules are DESIGN.md §9 (rank 7).
#pragma once
#include "orbx_pose_math.h"

#ifndef ORBX_BA_MAX_POSES
#define ORBX_BA_MAX_POSES 8  // = include/orbx.h
#endif
#define BA_LANES 256             // lanes of the summation rule (rule 9): the kernel's workgroup size
#define BA_MAX_THETA 1.0e5       // ba_sincos is exact-reduction-safe up to here; a larger rotation angle is `failure`
#define BA_EPS 2.220446049250313e-16  // DBL_EPSILON: the small-angle switch of ceres::AngleAxisRotatePoint
#define BA_DBL_MAX 1.7976931348623157e308
// Ceres' trust-region defaults (rule 5-8)
#define BA_RADIUS0 1e4
#define BA_RADIUS_MAX 1e16
#define BA_RADIUS_MIN 1e-32
#define BA_DIAG_MIN 1e-6
#define BA_DIAG_MAX 1e32
#define BA_MIN_REL_DECREASE 1e-3
#define BA_FUNCTION_TOL 1e-6
#define BA_GRADIENT_TOL 1e-10
#define BA_PARAMETER_TOL 1e-8

enum { BA_CONVERGENCE = 0, BA_NO_CONVERGENCE = 1, BA_FAILURE = 2, BA_SKIPPED = 3 };

// ---- sin / cos for x in [0, BA_MAX_THETA]: Cody-Waite reduction by pi/2 in three 33-bit pieces (n * piece is
// exact for n < 2^20), then fdlibm's __kernel_sin / __kernel_cos on the reduced (head, tail) pair ----------------
ORBX_PHD double ba_ksin(double x, double y) {
  ORBX_PNO_CONTRACT
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double z = x * x;
  const double v = z * x;
  const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
  return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
ORBX_PHD double ba_kcos(double x, double y) {
  ORBX_PNO_CONTRACT
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double z = x * x;
  const double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
  const uint32_t ix = (uint32_t)(pose_d2u(x) >> 32) & 0x7fffffffu;
  if (ix < 0x3FD33333u) return 1.0 - (0.5 * z - (z * r - x * y));
  const double qx = ix > 0x3fe90000u ? 0.28125 : pose_u2d((uint64_t)(ix - 0x00200000u) << 32);
  const double hz = 0.5 * z - qx;
  const double a = 1.0 - qx;
  return a - (hz - (z * r - x * y));
}
ORBX_PHD void ba_sincos(double x, double* sn, double* cs) {
  ORBX_PNO_CONTRACT
  const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
               pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;
  double y0 = x, y1 = 0.0;
  int n = 0;
  if (x > 0.78539816339744828) {
    n = (int)(x * invpio2 + 0.5);
    const double fn = (double)n;
    const double t = x - fn * pio2_1;
    const double w = fn * pio2_2;
    const double r = t - w;
    const double w2 = fn * pio2_2t - ((t - r) - w);
    y0 = r - w2;
    y1 = (r - y0) - w2;
  }
  const double ks = ba_ksin(y0, y1), kc = ba_kcos(y0, y1);
  switch (n & 3) {
    case 0: *sn = ks, *cs = kc; break;
    case 1: *sn = kc, *cs = -ks; break;
    case 2: *sn = -ks, *cs = -kc; break;
    default: *sn = -kc, *cs = ks; break;
  }
}

// ---- one pose, prepared once per evaluation point (rule 1) ------------------------------------------------------
struct BaPose {
  double w[3];  // unit axis (general branch) or the angle-axis vector itself (small-angle branch)
  double t[3];
  double c, s, theta;
  double R[9];  // d p / d X of the branch taken
  int small, ok;
};

ORBX_PHD void ba_pose_prepare(const double* pose6, BaPose* P) {
  ORBX_PNO_CONTRACT
  const double a0 = pose6[0], a1 = pose6[1], a2 = pose6[2];
  const double th2 = a0 * a0 + a1 * a1 + a2 * a2;
  P->t[0] = pose6[3], P->t[1] = pose6[4], P->t[2] = pose6[5];
  P->ok = 1;
  if (th2 > BA_EPS) {
    const double th = pose_sqrt(th2);
    P->small = 0;
    P->theta = th;
    if (!(th <= BA_MAX_THETA)) {  // also a NaN
      P->ok = 0;
      P->c = 1.0, P->s = 0.0;
    } else {
      ba_sincos(th, &P->s, &P->c);
    }
    const double w0 = a0 / th, w1 = a1 / th, w2 = a2 / th;
    P->w[0] = w0, P->w[1] = w1, P->w[2] = w2;
    const double c = P->c, s = P->s, k = 1.0 - c;
    P->R[0] = c + k * w0 * w0, P->R[1] = k * w0 * w1 - s * w2, P->R[2] = k * w0 * w2 + s * w1;
    P->R[3] = k * w1 * w0 + s * w2, P->R[4] = c + k * w1 * w1, P->R[5] = k * w1 * w2 - s * w0;
    P->R[6] = k * w2 * w0 - s * w1, P->R[7] = k * w2 * w1 + s * w0, P->R[8] = c + k * w2 * w2;
  } else {
    if (!(th2 == th2)) P->ok = 0;
    P->small = 1;
    P->theta = 0.0, P->c = 1.0, P->s = 0.0;
    P->w[0] = a0, P->w[1] = a1, P->w[2] = a2;
    P->R[0] = 1.0, P->R[1] = -a2, P->R[2] = a1;
    P->R[3] = a2, P->R[4] = 1.0, P->R[5] = -a0;
    P->R[6] = -a1, P->R[7] = a0, P->R[8] = 1.0;
  }
}

// ceres::AngleAxisRotatePoint(pose, X) + t
ORBX_PHD void ba_transform(const BaPose& P, const double* X, double* p) {
  ORBX_PNO_CONTRACT
  const double* w = P.w;
  const double x0 = w[1] * X[2] - w[2] * X[1], x1 = w[2] * X[0] - w[0] * X[2], x2 = w[0] * X[1] - w[1] * X[0];
  if (!P.small) {
    const double tmp = (w[0] * X[0] + w[1] * X[1] + w[2] * X[2]) * (1.0 - P.c);
    p[0] = (X[0] * P.c + x0 * P.s + w[0] * tmp) + P.t[0];
    p[1] = (X[1] * P.c + x1 * P.s + w[1] * tmp) + P.t[1];
    p[2] = (X[2] * P.c + x2 * P.s + w[2] * tmp) + P.t[2];
  } else {
    p[0] = (X[0] + x0) + P.t[0];
    p[1] = (X[1] + x1) + P.t[1];
    p[2] = (X[2] + x2) + P.t[2];
  }
}

// Huber on s = |r|^2 with scale delta (rule 3): rho, and sqrt(rho') -- the factor Ceres' corrector puts on the
// residual and the Jacobian when rho'' <= 0
ORBX_PHD double ba_huber(double s, double delta, double* sqrt_rho1) {
  ORBX_PNO_CONTRACT
  const double b = delta * delta;
  if (s <= b) {
    *sqrt_rho1 = 1.0;
    return s;
  }
  const double r = pose_sqrt(s);
  *sqrt_rho1 = pose_sqrt(delta / r);
  return 2.0 * delta * r - b;
}

// rho of one observation at (P, X); K4 = fx, fy, cx, cy.  *z receives the depth p2.
ORBX_PHD double ba_obs_cost(const double* K4, const BaPose& P, const double* X, double ox, double oy, double delta,
                            double* z) {
  ORBX_PNO_CONTRACT
  double p[3], w;
  ba_transform(P, X, p);
  *z = p[2];
  const double r0 = (K4[0] * p[0] / p[2] + K4[2]) - ox, r1 = (K4[1] * p[1] / p[2] + K4[3]) - oy;
  return ba_huber(r0 * r0 + r1 * r1, delta, &w);
}

struct BaObs {
  double r[2];    // residual, times sqrt(rho') when weighted
  double Jc[12];  // 2 x 6: d r / d (angle-axis, t), the same
  double Jp[6];   // 2 x 3: d r / d X, the same
  double rho, z;
};

// residual, Jacobians of the branch taken, loss (rules 1-3)
ORBX_PHD void ba_obs_eval(const double* K4, const BaPose& P, const double* X, double ox, double oy, double delta,
                          bool weighted, BaObs* o) {
  ORBX_PNO_CONTRACT
  double p[3];
  ba_transform(P, X, p);
  o->z = p[2];
  const double r0 = (K4[0] * p[0] / p[2] + K4[2]) - ox, r1 = (K4[1] * p[1] / p[2] + K4[3]) - oy;
  double wt;
  o->rho = ba_huber(r0 * r0 + r1 * r1, delta, &wt);
  if (!weighted) wt = 1.0;
  // d (u, v) / d p
  const double a0 = K4[0] / p[2], a2 = -(K4[0] * p[0]) / (p[2] * p[2]);
  const double b1 = K4[1] / p[2], b2 = -(K4[1] * p[1]) / (p[2] * p[2]);
  const double* w = P.w;
  double dp[3][3];  // dp[k] = d p / d omega_k
  if (!P.small) {
    const double c = P.c, s = P.s, k1 = 1.0 - c, th = P.theta;
    const double wx[3] = {w[1] * X[2] - w[2] * X[1], w[2] * X[0] - w[0] * X[2], w[0] * X[1] - w[1] * X[0]};
    const double wd = w[0] * X[0] + w[1] * X[1] + w[2] * X[2];
ORBX_PUNROLL
    for (int k = 0; k < 3; k++) {
      double dw[3];
ORBX_PUNROLL
      for (int j = 0; j < 3; j++) dw[j] = ((j == k ? 1.0 : 0.0) - w[k] * w[j]) / th;
      const double dx[3] = {dw[1] * X[2] - dw[2] * X[1], dw[2] * X[0] - dw[0] * X[2], dw[0] * X[1] - dw[1] * X[0]};
      const double dd = dw[0] * X[0] + dw[1] * X[1] + dw[2] * X[2];
ORBX_PUNROLL
      for (int j = 0; j < 3; j++)
        dp[k][j] = (c * w[k] * wx[j] - s * w[k] * X[j]) + s * dx[j] + s * w[k] * wd * w[j] + k1 * (dd * w[j] + wd * dw[j]);
    }
  } else {  // p = X + omega x X + t
    dp[0][0] = 0.0, dp[0][1] = -X[2], dp[0][2] = X[1];
    dp[1][0] = X[2], dp[1][1] = 0.0, dp[1][2] = -X[0];
    dp[2][0] = -X[1], dp[2][1] = X[0], dp[2][2] = 0.0;
  }
  o->r[0] = wt * r0;
  o->r[1] = wt * r1;
ORBX_PUNROLL
  for (int k = 0; k < 3; k++) {
    o->Jc[k] = wt * (a0 * dp[k][0] + a2 * dp[k][2]);
    o->Jc[6 + k] = wt * (b1 * dp[k][1] + b2 * dp[k][2]);
    o->Jp[k] = wt * (a0 * P.R[k] + a2 * P.R[6 + k]);
    o->Jp[3 + k] = wt * (b1 * P.R[3 + k] + b2 * P.R[6 + k]);
  }
  o->Jc[3] = wt * a0, o->Jc[4] = 0.0, o->Jc[5] = wt * a2;
  o->Jc[9] = 0.0, o->Jc[10] = wt * b1, o->Jc[11] = wt * b2;
}

// ---- per-landmark pieces of the normal equations (rule 4) --------------------------------------------------------
// V (xx, xy, xz, yy, yz, zz) += Jp^T Jp, gp += Jp^T r
ORBX_PHD void ba_accum_point(const BaObs& o, double* V, double* gp) {
  ORBX_PNO_CONTRACT
  const double* a = o.Jp;
  const double* b = o.Jp + 3;
  V[0] = V[0] + (a[0] * a[0] + b[0] * b[0]);
  V[1] = V[1] + (a[0] * a[1] + b[0] * b[1]);
  V[2] = V[2] + (a[0] * a[2] + b[0] * b[2]);
  V[3] = V[3] + (a[1] * a[1] + b[1] * b[1]);
  V[4] = V[4] + (a[1] * a[2] + b[1] * b[2]);
  V[5] = V[5] + (a[2] * a[2] + b[2] * b[2]);
ORBX_PUNROLL
  for (int k = 0; k < 3; k++) gp[k] = gp[k] + (a[k] * o.r[0] + b[k] * o.r[1]);
}
// W (6 x 3) = Jc^T Jp of one observation
ORBX_PHD void ba_obs_W(const BaObs& o, double* W) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int a = 0; a < 6; a++)
ORBX_PUNROLL
    for (int b = 0; b < 3; b++) W[a * 3 + b] = o.Jc[a] * o.Jp[b] + o.Jc[6 + a] * o.Jp[3 + b];
}
// acc[0, 21) += lower triangle of Jc^T Jc (row-major: 00, 10, 11, 20, ...), acc[21, 27) += Jc^T r
ORBX_PHD void ba_accum_pose(const BaObs& o, double* acc) {
  ORBX_PNO_CONTRACT
  int k = 0;
ORBX_PUNROLL
  for (int a = 0; a < 6; a++)
ORBX_PUNROLL
    for (int b = 0; b <= a; b++, k++) acc[k] = acc[k] + (o.Jc[a] * o.Jc[b] + o.Jc[6 + a] * o.Jc[6 + b]);
ORBX_PUNROLL
  for (int a = 0; a < 6; a++) acc[21 + a] = acc[21 + a] + (o.Jc[a] * o.r[0] + o.Jc[6 + a] * o.r[1]);
}
// Jacobi scale of a column from the diagonal of J^T J at the start (rule 5)
ORBX_PHD double ba_jacobi_scale(double diag) {
  ORBX_PNO_CONTRACT
  return 1.0 / (1.0 + pose_sqrt(diag));
}
ORBX_PHD double ba_damping(double diag, double radius) {
  ORBX_PNO_CONTRACT
  const double d = diag < BA_DIAG_MIN ? BA_DIAG_MIN : (diag > BA_DIAG_MAX ? BA_DIAG_MAX : diag);
  return d / radius;
}
// The damped, scaled point block inverted by its symmetric adjugate (rule 6).  gs = scaled gradient, D2 = the
// damping.  A determinant that is not > 0: Vinv = 0, the landmark takes no step and enters no reduction.
ORBX_PHD bool ba_point_invert(const double* V, const double* gp, const double* sp, double radius, double* Vinv,
                              double* gs, double* D2) {
  ORBX_PNO_CONTRACT
  const double v00 = sp[0] * sp[0] * V[0], v01 = sp[0] * sp[1] * V[1], v02 = sp[0] * sp[2] * V[2];
  const double v11 = sp[1] * sp[1] * V[3], v12 = sp[1] * sp[2] * V[4], v22 = sp[2] * sp[2] * V[5];
  D2[0] = ba_damping(v00, radius), D2[1] = ba_damping(v11, radius), D2[2] = ba_damping(v22, radius);
  gs[0] = sp[0] * gp[0], gs[1] = sp[1] * gp[1], gs[2] = sp[2] * gp[2];
  const double m00 = v00 + D2[0], m11 = v11 + D2[1], m22 = v22 + D2[2];
  const double c00 = m11 * m22 - v12 * v12, c01 = v02 * v12 - v01 * m22, c02 = v01 * v12 - v02 * m11;
  const double det = m00 * c00 + v01 * c01 + v02 * c02;
  if (!(det > 0.0) || det > BA_DBL_MAX) {
ORBX_PUNROLL
    for (int k = 0; k < 6; k++) Vinv[k] = 0.0;
    return false;
  }
  Vinv[0] = c00 / det, Vinv[1] = c01 / det, Vinv[2] = c02 / det;
  Vinv[3] = (m00 * m22 - v02 * v02) / det, Vinv[4] = (v01 * v02 - m00 * v12) / det;
  Vinv[5] = (m00 * m11 - v01 * v01) / det;
  return true;
}
// one row of Ws = diag(sc) W diag(sp): out[b] = (sc_a W[a][b]) sp[b]
ORBX_PHD void ba_scale_W_row(const double* w3, double sc_a, const double* sp, double* out3) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int b = 0; b < 3; b++) out3[b] = (sc_a * w3[b]) * sp[b];
}
ORBX_PHD void ba_scale_W(const double* W, const double* sc, const double* sp, double* Ws) {
ORBX_PUNROLL
  for (int a = 0; a < 6; a++) ba_scale_W_row(W + a * 3, sc[a], sp, Ws + a * 3);
}
// Y (6 x 3) = Ws Vinv
ORBX_PHD void ba_W_Vinv(const double* Ws, const double* Vi, double* Y) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int a = 0; a < 6; a++) {
    const double x = Ws[a * 3], y = Ws[a * 3 + 1], z = Ws[a * 3 + 2];
    Y[a * 3 + 0] = x * Vi[0] + y * Vi[1] + z * Vi[2];
    Y[a * 3 + 1] = x * Vi[1] + y * Vi[3] + z * Vi[4];
    Y[a * 3 + 2] = x * Vi[2] + y * Vi[4] + z * Vi[5];
  }
}
// column b of a pose-pair block: acc[a * 6 + b] += (Y Wg^T)[a][b], wg3 = row b of Wg
ORBX_PHD void ba_accum_pair_col(const double* Y, const double* wg3, int b, double* acc) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int a = 0; a < 6; a++)
    acc[a * 6 + b] = acc[a * 6 + b] + (Y[a * 3] * wg3[0] + Y[a * 3 + 1] * wg3[1] + Y[a * 3 + 2] * wg3[2]);
}
// acc[0, 36) += Y Wg^T (row-major 6 x 6): the block of two different poses
ORBX_PHD void ba_accum_pair(const double* Y, const double* Wg, double* acc) {
ORBX_PUNROLL
  for (int b = 0; b < 6; b++) ba_accum_pair_col(Y, Wg + b * 3, b, acc);
}
// acc[0, 21) += the lower triangle of Y Wf^T (row-major: 00, 10, 11, 20, ...): a pose with itself; the block is
// symmetric in exact arithmetic and only its lower triangle is ever read
ORBX_PHD void ba_accum_diag(const double* Y, const double* Wf, double* acc) {
  ORBX_PNO_CONTRACT
  int k = 0;
ORBX_PUNROLL
  for (int a = 0; a < 6; a++)
ORBX_PUNROLL
    for (int b = 0; b <= a; b++, k++)
      acc[k] = acc[k] + (Y[a * 3] * Wf[b * 3] + Y[a * 3 + 1] * Wf[b * 3 + 1] + Y[a * 3 + 2] * Wf[b * 3 + 2]);
}
// acc[0, 6) += Y gs
ORBX_PHD void ba_accum_rhs(const double* Y, const double* gs, double* acc) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int a = 0; a < 6; a++) acc[a] = acc[a] + (Y[a * 3] * gs[0] + Y[a * 3 + 1] * gs[1] + Y[a * 3 + 2] * gs[2]);
}
// u (3) += Ws^T sc_step (the pose's scaled step)
ORBX_PHD void ba_accum_Wt_step(const double* Ws, const double* step, double* u) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int b = 0; b < 3; b++) {
    double v = u[b];
ORBX_PUNROLL
    for (int a = 0; a < 6; a++) v = v + Ws[a * 3 + b] * step[a];
    u[b] = v;
  }
}
// Back-substitution of one landmark: scaled step s = -Vinv (gs + u); candidate = X + diag(sp) s.
// acc[0] += s . (D2 s - gs)  (model decrease, rule 7), acc[1] += |diag(sp) s|^2, acc[2] += |X|^2
ORBX_PHD void ba_point_step(const double* Vi, const double* gs, const double* u, const double* D2, const double* sp,
                            const double* X, double* cand, double* acc) {
  ORBX_PNO_CONTRACT
  const double q0 = gs[0] + u[0], q1 = gs[1] + u[1], q2 = gs[2] + u[2];
  double s[3];
  s[0] = -(Vi[0] * q0 + Vi[1] * q1 + Vi[2] * q2);
  s[1] = -(Vi[1] * q0 + Vi[3] * q1 + Vi[4] * q2);
  s[2] = -(Vi[2] * q0 + Vi[4] * q1 + Vi[5] * q2);
  double m = 0.0, n2 = 0.0, x2 = 0.0;
ORBX_PUNROLL
  for (int k = 0; k < 3; k++) {
    const double d = sp[k] * s[k];
    cand[k] = X[k] + d;
    m = m + s[k] * (D2[k] * s[k] - gs[k]);
    n2 = n2 + d * d;
    x2 = x2 + X[k] * X[k];
  }
  acc[0] = acc[0] + m;
  acc[1] = acc[1] + n2;
  acc[2] = acc[2] + x2;
}

// ---- the serial part: one lane in the kernel (rules 6-8) ----------------------------------------------------------
// In-place Cholesky (no pivoting) of the lower triangle of A (n x n, row-major, leading dimension ld) and the solve
// A x = b, x over b.  A pivot that is not > 0: false.
ORBX_PHD bool ba_cholesky_solve(int n, int ld, double* A, double* b) {
  ORBX_PNO_CONTRACT
  for (int j = 0; j < n; j++) {
    double d = A[j * ld + j];
    for (int k = 0; k < j; k++) d = d - A[j * ld + k] * A[j * ld + k];
    if (!(d > 0.0) || d > BA_DBL_MAX) return false;
    const double l = pose_sqrt(d);
    A[j * ld + j] = l;
    for (int i = j + 1; i < n; i++) {
      double v = A[i * ld + j];
      for (int k = 0; k < j; k++) v = v - A[i * ld + k] * A[j * ld + k];
      A[i * ld + j] = v / l;
    }
  }
  for (int i = 0; i < n; i++) {
    double v = b[i];
    for (int k = 0; k < i; k++) v = v - A[i * ld + k] * b[k];
    b[i] = v / A[i * ld + i];
  }
  for (int i = n - 1; i >= 0; i--) {
    double v = b[i];
    for (int k = i + 1; k < n; k++) v = v - A[k * ld + i] * b[k];
    b[i] = v / A[i * ld + i];
  }
  return true;
}

// The reduced camera system (rule 6).  In: the lower blocks of A hold sum_j Wf Vinv Wg^T, b holds sum_j Wf Vinv gs,
// U holds 27 doubles per free pose (lower triangle of Jc^T Jc, then Jc^T r).  Out: A = diag(U' + Dc) - (...),
// b = (...) - gcs; Dc = the poses' damping, gcs = their scaled gradient.
ORBX_PHD void ba_assemble(int P, const double* U, const double* sc, double radius, double* A, int ld, double* b,
                          double* Dc, double* gcs) {
  ORBX_PNO_CONTRACT
  for (int f = 0; f < P; f++) {
    for (int a = 0; a < 6; a++) {
      const int r = 6 * f + a;
      for (int c = 0; c < 6 * f; c++) A[r * ld + c] = -A[r * ld + c];
      for (int c = 0; c <= a; c++) {
        const double u = (sc[r] * sc[6 * f + c]) * U[f * 27 + a * (a + 1) / 2 + c];
        if (c == a) {
          Dc[r] = ba_damping(u, radius);
          A[r * ld + r] = (u + Dc[r]) - A[r * ld + r];
        } else {
          A[r * ld + 6 * f + c] = u - A[r * ld + 6 * f + c];
        }
      }
      gcs[r] = sc[r] * U[f * 27 + 21 + a];
      b[r] = b[r] - gcs[r];
    }
  }
}
// candidate poses = x + diag(sc) step for poses 1 .. W-1 (pose 0 is constant); the poses' share of the model
// decrease, of |step|^2 and of |x|^2, summed in index order
ORBX_PHD void ba_pose_step(int W, const double* x, const double* sc, const double* step, const double* Dc,
                           const double* gcs, double* cand, double* model, double* step2, double* x2) {
  ORBX_PNO_CONTRACT
  double m = 0.0, n2 = 0.0, xx = 0.0;
  for (int k = 0; k < 6; k++) cand[k] = x[k];
  for (int r = 0; r < 6 * (W - 1); r++) {
    const double d = sc[r] * step[r];
    cand[6 + r] = x[6 + r] + d;
    m = m + step[r] * (Dc[r] * step[r] - gcs[r]);
    n2 = n2 + d * d;
    xx = xx + x[6 + r] * x[6 + r];
  }
  *model = m, *step2 = n2, *x2 = xx;
}

struct BaSummary {  // = orbx_ba_summary
  int32_t termination, iterations, successful_steps, pad;
  double initial_cost, final_cost;
};
struct BaTrust {
  double radius, decrease, cost;
};
enum { BA_STEP_REJECTED = 0, BA_STEP_ACCEPTED = 1, BA_STEP_CONVERGED = 2 };

ORBX_PHD void ba_trust_reject(BaTrust* T) {
  ORBX_PNO_CONTRACT
  T->radius = T->radius / T->decrease;
  T->decrease = T->decrease * 2.0;
}
// Ceres' order (rule 8): parameter tolerance, function tolerance, then the acceptance test.  cost terms are
// 1/2 sum rho; model = the model's decrease; step2 / x2 = squared norms of the step and of the accepted parameters.
ORBX_PHD int ba_trust_decide(BaTrust* T, bool solved, double model, double cand_cost, double step2, double x2) {
  ORBX_PNO_CONTRACT
  if (!solved || !(model > 0.0)) {
    ba_trust_reject(T);
    return BA_STEP_REJECTED;
  }
  if (pose_sqrt(step2) <= BA_PARAMETER_TOL * (pose_sqrt(x2) + BA_PARAMETER_TOL)) return BA_STEP_CONVERGED;
  if (!(cand_cost <= BA_DBL_MAX)) {  // a candidate that cannot be evaluated is a rejected step
    ba_trust_reject(T);
    return BA_STEP_REJECTED;
  }
  const double change = T->cost - cand_cost;
  if (pose_abs(change) <= BA_FUNCTION_TOL * T->cost) return BA_STEP_CONVERGED;
  const double rel = change / model;
  if (rel > BA_MIN_REL_DECREASE) {
    const double q = 2.0 * rel - 1.0;
    double f = 1.0 - q * q * q;
    if (f < 1.0 / 3.0) f = 1.0 / 3.0;
    T->radius = T->radius / f;
    if (T->radius > BA_RADIUS_MAX) T->radius = BA_RADIUS_MAX;
    T->decrease = 2.0;
    T->cost = cand_cost;
    return BA_STEP_ACCEPTED;
  }
  ba_trust_reject(T);
  return BA_STEP_REJECTED;
}

// ---- landmark priors (rules P1 and P2) --------------------------------------------------------
// The residual block sqrt(lam) (X - A) of one landmark, with no loss function and no square root taken:
// rho += lam |X - A|^2, the diagonal of V += lam, gp += lam (X - A).  Called after the landmark's last observation.
// lam = 0 (anything that is not > 0) is no operation at all: every accumulator keeps its bits.
ORBX_PHD void ba_prior_accum(const double* X, const double* A, double lam, double* V, double* gp, double* rho) {
  ORBX_PNO_CONTRACT
  if (!(lam > 0.0)) return;
  const double d0 = X[0] - A[0], d1 = X[1] - A[1], d2 = X[2] - A[2];
  *rho = *rho + lam * ((d0 * d0 + d1 * d1) + d2 * d2);
  V[0] = V[0] + lam, V[3] = V[3] + lam, V[5] = V[5] + lam;
  gp[0] = gp[0] + lam * d0, gp[1] = gp[1] + lam * d1, gp[2] = gp[2] + lam * d2;
}
// rho of the same block at X: the landmark's term of the candidate's cost, behind its observations' (rule P2)
ORBX_PHD double ba_prior_cost(const double* X, const double* A, double lam) {
  ORBX_PNO_CONTRACT
  const double d0 = X[0] - A[0], d1 = X[1] - A[1], d2 = X[2] - A[2];
  return lam * ((d0 * d0 + d1 * d1) + d2 * d2);
}
