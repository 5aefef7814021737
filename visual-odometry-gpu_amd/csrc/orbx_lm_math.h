// orbx_lm_math.h -- the arithmetic of buildLandmarksFromFirstTwoFramesAndTracks
// (src/with_bundle_adjustment.cpp:502-575): the baseline gate, the two projection matrices, the linear triangulation
// of one track from its first two pixels and the depth check.  Shared by the gfx950 kernels (orbx_landmarks.hip) and
// the sequential restatement (tests/cpp/lm_sequential.cpp).  Binary64 built from IEEE + - * / and pose_sqrt only, on
// top of orbx_ba_math.h (the pose) and orbx_tri_math.h (projections, DLT), so the same source compiled with
// -ffp-contract=off for gfx950 and for x86-64 returns the same bits.  The rules are DESIGN.md §9 (rank 10).
// Below them: the pieces of the N-view build with its reprojection gate (rank 15), shared with
// tests/cpp/lm_views_sequential.cpp.
#pragma once
#include "orbx_ba_math.h"
#include "orbx_tri_math.h"

// = include/orbx.h: orbx_lm_status
enum { LM_OK = 0, LM_BASELINE = 1, LM_EMPTY = 2, LM_BAD_POSE = 3 };
// the reference's gate on the distance of the first two cameras (src/with_bundle_adjustment.cpp:515-516)
#define LM_BASELINE_MIN 0.1
#define LM_BASELINE_MAX 100.0

// rule 2: the distance of two camera translations against the gate
ORBX_PHD int lm_baseline(const double* t0, const double* t1) {
  ORBX_PNO_CONTRACT
  const double dx = t0[0] - t1[0], dy = t0[1] - t1[1], dz = t0[2] - t1[2];
  const double b = pose_sqrt((dx * dx + dy * dy) + dz * dz);
  return b < LM_BASELINE_MIN || b > LM_BASELINE_MAX ? LM_BASELINE : LM_OK;
}

// rules 1-3 of one window: the camera matrices of poses 0 and 1 (BA's own blocks: angle-axis, translation, world ->
// camera), the gate, and P0 = K [R0 | t0], P1 = K [R1 | t1] (row-major 3x4).  K: row-major 3x3.  Returns LM_OK,
// LM_BASELINE or LM_BAD_POSE; P0 / P1 are written only for LM_OK.
ORBX_PHD int lm_window_prepare(const double* K, const double* pose0, const double* pose1, double* P0, double* P1) {
  ORBX_PNO_CONTRACT
  BaPose A, B;
  ba_pose_prepare(pose0, &A);
  ba_pose_prepare(pose1, &B);
  if (!A.ok || !B.ok) return LM_BAD_POSE;
  if (lm_baseline(A.t, B.t) != LM_OK) return LM_BASELINE;
  double unused[12];
  tri_projections(K, A.R, A.t, unused, P0);
  tri_projections(K, B.R, B.t, unused, P1);
  return LM_OK;
}

ORBX_PHD bool lm_finite(double x) { return (pose_d2u(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// rules 3-4 of one track: the DLT in WORLD coordinates on the float pixels widened to double, X = h / h[3] kept in
// binary64; returns whether the landmark is kept (h[3] != 0, three finite quotients, world z > 0).  X always holds
// the three quotients.
ORBX_PHD bool lm_point(const double* P0, const double* P1, float x0, float y0, float x1, float y1, double* X) {
  ORBX_PNO_CONTRACT
  double h[4];
  tri_homogeneous(P0, P1, (double)x0, (double)y0, (double)x1, (double)y1, h);
  X[0] = h[0] / h[3], X[1] = h[1] / h[3], X[2] = h[2] / h[3];
  const bool valid = h[3] != 0.0 && lm_finite(X[0]) && lm_finite(X[1]) && lm_finite(X[2]);
  return valid && X[2] > 0.0;
}

// observations a slot contributes: `seen` clamped into [0, window_len] (a live slot of the tracker is inside already)
ORBX_PHD int lm_seen(int seen, int window_len) { return seen < 0 ? 0 : (seen > window_len ? window_len : seen); }

// ---- rank 15: a point from every view of its track, and the reprojection gate -------------------------------------
// = include/orbx_lm.h: orbx_lm_tri_mode, orbx_lm_reason
enum { LM_TRI_FIRST_TWO = 0, LM_TRI_WIDEST = 1, LM_TRI_ALL_VIEWS = 2 };
enum { LM_KEPT = 0, LM_SHORT = 1, LM_DEGENERATE = 2, LM_BEHIND = 3, LM_REPROJECTION = 4, LM_NO_WINDOW = 5 };
// one view's record: P_k = K [R_k | t_k] (row-major 3x4), then row 2 of [R_k | t_k] (the camera depth of a point)
#define LM_VIEW_DOUBLES 16

// rule 1: the views of a window that are prepared -- two for the first-two build without a gate (rank 10 exactly),
// every one otherwise.  Depth and reprojection look at the observed views among them.
ORBX_PHD int lm_views_prepared(int tri_mode, double max_reproj_px, int window_len) {
  return tri_mode == LM_TRI_FIRST_TWO && !(max_reproj_px > 0.0) ? 2 : window_len;
}

// rule 1 of one view: the record of its pose; returns whether ba_pose_prepare accepted the pose
ORBX_PHD int lm_view_prepare(const double* K, const double* pose6, double* rec) {
  ORBX_PNO_CONTRACT
  BaPose A;
  ba_pose_prepare(pose6, &A);
  double unused[12];
  tri_projections(K, A.R, A.t, unused, rec);
  rec[12] = A.R[6], rec[13] = A.R[7], rec[14] = A.R[8], rec[15] = A.t[2];
  return A.ok;
}

// rule 2: whether view k of a slot with sn observations enters the system (view 0 always does)
ORBX_PHD bool lm_view_used(int tri_mode, int k, int sn) {
  return tri_mode == LM_TRI_ALL_VIEWS ? k < sn : (tri_mode == LM_TRI_WIDEST ? k == 0 || k == sn - 1 : k < 2);
}

// rule 3: the x row and the y row of one view, as tri_homogeneous forms them
ORBX_PHD void lm_view_rows(const double* P, double x, double y, double* rx, double* ry) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int j = 0; j < 4; j++) {
    rx[j] = x * P[8 + j] - P[j];
    ry[j] = y * P[8 + j] - P[4 + j];
  }
}
// rule 3: the upper triangle of A^T A, summed row by row: the first row's products start the sums
ORBX_PHD void lm_normal_start(double (*a)[4], const double* r) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int i = 0; i < 4; i++)
ORBX_PUNROLL
    for (int j = i; j < 4; j++) a[i][j] = r[i] * r[j];
}
ORBX_PHD void lm_normal_add(double (*a)[4], const double* r) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int i = 0; i < 4; i++)
ORBX_PUNROLL
    for (int j = i; j < 4; j++) a[i][j] = a[i][j] + r[i] * r[j];
}

// rule 4: X = h / h[3]; returns whether the point is valid (h[3] != 0, three finite quotients)
ORBX_PHD bool lm_quotient(const double* h, double* X) {
  ORBX_PNO_CONTRACT
  X[0] = h[0] / h[3], X[1] = h[1] / h[3], X[2] = h[2] / h[3];
  return h[3] != 0.0 && lm_finite(X[0]) && lm_finite(X[1]) && lm_finite(X[2]);
}

// rule 5: the depth of X in the camera of a view's record
ORBX_PHD double lm_view_depth(const double* rec, const double* X) {
  ORBX_PNO_CONTRACT
  return (rec[12] * X[0] + rec[13] * X[1] + rec[14] * X[2]) + rec[15];
}

// rule 6: the squared reprojection error of X against the pixel (x, y) of a view
ORBX_PHD double lm_view_e2(const double* P, const double* X, double x, double y) {
  ORBX_PNO_CONTRACT
  const double q0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
  const double q1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
  const double q2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  const double ex = q0 / q2 - x, ey = q1 / q2 - y;
  return ex * ex + ey * ey;
}
// rule 6: reproj_px of a slot from its largest finite error; +inf when one was not finite
ORBX_PHD float lm_reproj_px(double max_e2, bool bad) {
  if (!bad) return (float)pose_sqrt(max_e2);
  const uint32_t inf = 0x7f800000u;
  float f;
  memcpy(&f, &inf, 4);
  return f;
}
