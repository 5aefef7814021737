// orbx_tri_math.h -- the per-point arithmetic of the reference's get_scale
// (cv::triangulatePoints + the median of distance ratios, src/feature_matching.cpp:208-275,
// src/feature_tracking.cpp:244-310) and of the pose chaining (src/feature_matching.cpp:77-82),
// shared by the gfx950 kernels (orbx_scale.hip) and host code.  Like orbx_pose_math.h it is
// binary64 / binary32 built from IEEE + - * / only (sqrt is pose_sqrt), so the same source
// compiled with -ffp-contract=off for gfx950 and for x86-64 returns the same bits.  The rules
// are written out in DESIGN.md §9 (rank 6).
#pragma once
#include "orbx_pose_math.h"

#define TRI_JACOBI_SWEEPS 10
// clamp of the estimated scale, src/feature_matching.cpp:273
#define TRI_SCALE_MIN 0.1
#define TRI_SCALE_MAX 5.0

// rule 1: P1 = K [I | 0], P2 = K [R | t] (row-major 3x4; K, R row-major 3x3), sums left to right
ORBX_PHD void tri_projections(const double* K, const double* R, const double* t, double* P1, double* P2) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int r = 0; r < 3; r++) {
ORBX_PUNROLL
    for (int c = 0; c < 3; c++) {
      P1[r * 4 + c] = K[r * 3 + c];
      P2[r * 4 + c] = K[r * 3 + 0] * R[0 * 3 + c] + K[r * 3 + 1] * R[1 * 3 + c] + K[r * 3 + 2] * R[2 * 3 + c];
    }
    P1[r * 4 + 3] = 0.0;
    P2[r * 4 + 3] = K[r * 3 + 0] * t[0] + K[r * 3 + 1] * t[1] + K[r * 3 + 2] * t[2];
  }
}

ORBX_PHD bool tri_finite(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (u & 0x7f800000u) != 0x7f800000u;
}

// rule 1, second half: the eigenvector h of the smallest eigenvalue of the symmetric 4x4 matrix whose UPPER triangle
// `a` holds (the lower one is filled in here), by TRI_JACOBI_SWEEPS cyclic Jacobi sweeps over (0,1) (0,2) (0,3) (1,2)
// (1,3) (2,3); of equal smallest eigenvalues the lowest column wins.  Shared by the two-view DLT below and the
// N-view one of orbx_lm_math.h.
ORBX_PHD void tri_smallest_eigenvector(double (*a)[4], double* h) {
  ORBX_PNO_CONTRACT
  double v[4][4];
ORBX_PUNROLL
  for (int i = 0; i < 4; i++)
ORBX_PUNROLL
    for (int j = 0; j < 4; j++) {
      if (j < i) a[i][j] = a[j][i];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sw = 0; sw < TRI_JACOBI_SWEEPS; sw++) {
ORBX_PUNROLL
    for (int p = 0; p < 3; p++) {
ORBX_PUNROLL
      for (int q = p + 1; q < 4; q++) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double at = pose_abs(theta);
        double tt = at > 1e150 ? 0.5 / at : 1.0 / (at + pose_sqrt(theta * theta + 1.0));
        if (theta < 0) tt = -tt;
        const double c = 1.0 / pose_sqrt(tt * tt + 1.0), s = tt * c;
        a[p][p] = a[p][p] - tt * apq;
        a[q][q] = a[q][q] + tt * apq;
        a[p][q] = a[q][p] = 0.0;
ORBX_PUNROLL
        for (int r = 0; r < 4; r++) {
          if (r != p && r != q) {
            const double arp = c * a[r][p] - s * a[r][q], arq = s * a[r][p] + c * a[r][q];
            a[r][p] = a[p][r] = arp;
            a[r][q] = a[q][r] = arq;
          }
          const double vp = c * v[r][p] - s * v[r][q], vq = s * v[r][p] + c * v[r][q];
          v[r][p] = vp;
          v[r][q] = vq;
        }
      }
    }
  }
  double dmin = a[0][0], h0 = v[0][0], h1 = v[1][0], h2 = v[2][0], h3 = v[3][0];
ORBX_PUNROLL
  for (int k = 1; k < 4; k++)
    if (a[k][k] < dmin) {
      dmin = a[k][k];
      h0 = v[0][k], h1 = v[1][k], h2 = v[2][k], h3 = v[3][k];
    }
  h[0] = h0, h[1] = h1, h[2] = h2, h[3] = h3;
}

// rule 1: the DLT of one correspondence in pixel units.  The homogeneous point h is the eigenvector of the
// smallest eigenvalue of A^T A (tri_smallest_eigenvector).
ORBX_PHD void tri_homogeneous(const double* P1, const double* P2, double x1, double y1, double x2, double y2,
                              double* h) {
  ORBX_PNO_CONTRACT
  double A[4][4], a[4][4];
ORBX_PUNROLL
  for (int j = 0; j < 4; j++) {
    A[0][j] = x1 * P1[8 + j] - P1[j];
    A[1][j] = y1 * P1[8 + j] - P1[4 + j];
    A[2][j] = x2 * P2[8 + j] - P2[j];
    A[3][j] = y2 * P2[8 + j] - P2[4 + j];
  }
ORBX_PUNROLL
  for (int i = 0; i < 4; i++)
ORBX_PUNROLL
    for (int j = i; j < 4; j++)
      a[i][j] = A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j] + A[3][i] * A[3][j];
  tri_smallest_eigenvector(a, h);
}

// rule 2: X/w, Y/w, Z/w in double, each cast to float; returns whether the point is valid (w != 0 and three
// finite floats), an invalid one is (0, 0, 0).
ORBX_PHD bool tri_point(const double* P1, const double* P2, double x1, double y1, double x2, double y2, float* xyz) {
  ORBX_PNO_CONTRACT
  double h[4];
  tri_homogeneous(P1, P2, x1, y1, x2, y2, h);
  const float X = (float)(h[0] / h[3]), Y = (float)(h[1] / h[3]), Z = (float)(h[2] / h[3]);
  const bool ok = h[3] != 0.0 && tri_finite(X) && tri_finite(Y) && tri_finite(Z);
  xyz[0] = ok ? X : 0.f;
  xyz[1] = ok ? Y : 0.f;
  xyz[2] = ok ? Z : 0.f;
  return ok;
}

// rule 4: X' = R X + t in double from the float point, cast back to float
ORBX_PHD void tri_transform(const double* R, const double* t, const float* X, float* out) {
  ORBX_PNO_CONTRACT
  const double x = (double)X[0], y = (double)X[1], z = (double)X[2];
ORBX_PUNROLL
  for (int r = 0; r < 3; r++) out[r] = (float)(R[r * 3 + 0] * x + R[r * 3 + 1] * y + R[r * 3 + 2] * z + t[r]);
}

// rule 3: |a - b| in float, left to right, with a correctly rounded float sqrt: pose_sqrt is within 2 ulp in double,
// and the square root of a float is never that close to the midpoint of two floats (a 25-bit m has a 50-bit m^2,
// so m^2 differs from any float by at least 2^-49 relative), so rounding it to float rounds the exact root.
ORBX_PHD float tri_dist(const float* a, const float* b) {
  ORBX_PNO_CONTRACT
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const float s = dx * dx + dy * dy + dz * dz;
  return (float)pose_sqrt((double)s);
}
// prev_dist / (cur_dist + 1e-6) in double, src/feature_matching.cpp:268
ORBX_PHD double tri_ratio(const float* prev_a, const float* prev_b, const float* cur_a, const float* cur_b) {
  ORBX_PNO_CONTRACT
  const double pd = (double)tri_dist(prev_a, prev_b), cd = (double)tri_dist(cur_a, cur_b);
  return pd / (cd + 1e-6);
}
// Two finite points can be far enough apart for dx * dx to overflow a float: inf / (inf + 1e-6) is NaN, whose sign
// differs between x86-64 and gfx950 and which has no place in an order.  A ratio that is not finite is no ratio.
ORBX_PHD bool tri_ratio_ok(double ratio) { return (pose_d2u(ratio) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
// the element at sorted position r / 2 of the r ratios -> the scale
ORBX_PHD double tri_scale_clamp(double median) {
  return median < TRI_SCALE_MIN ? TRI_SCALE_MIN : (median > TRI_SCALE_MAX ? TRI_SCALE_MAX : median);
}

// rule 5: cur = prev * T^-1 with T = [R | s t], T^-1 = [R^T | -s R^T t]; row-major 4x4
ORBX_PHD void tri_chain(const double* prev, const double* R, const double* t, double s, double* cur) {
  ORBX_PNO_CONTRACT
  double Ti[16];
ORBX_PUNROLL
  for (int r = 0; r < 3; r++) {
ORBX_PUNROLL
    for (int c = 0; c < 3; c++) Ti[r * 4 + c] = R[c * 3 + r];
    Ti[r * 4 + 3] = -(s * (R[0 * 3 + r] * t[0] + R[1 * 3 + r] * t[1] + R[2 * 3 + r] * t[2]));
  }
  Ti[12] = Ti[13] = Ti[14] = 0.0;
  Ti[15] = 1.0;
  double out[16];
ORBX_PUNROLL
  for (int r = 0; r < 4; r++)
ORBX_PUNROLL
    for (int c = 0; c < 4; c++)
      out[r * 4 + c] = prev[r * 4 + 0] * Ti[0 * 4 + c] + prev[r * 4 + 1] * Ti[1 * 4 + c] + prev[r * 4 + 2] * Ti[2 * 4 + c] +
                       prev[r * 4 + 3] * Ti[3 * 4 + c];
ORBX_PUNROLL
  for (int i = 0; i < 16; i++) cur[i] = out[i];
}
