// orbx_lm_math.h -- the arithmetic of buildLandmarksFromFirstTwoFramesAndTracks
// (src/with_bundle_adjustment.cpp:502-575): the baseline gate, the two projection matrices, the linear triangulation
// of one track from its first two pixels and the depth check.  Shared by the gfx950 kernels (orbx_landmarks.hip) and
// the sequential restatement (tests/cpp/lm_sequential.cpp).  Binary64 built from IEEE + - * / and pose_sqrt only, on
// top of orbx_ba_math.h (the pose) and orbx_tri_math.h (projections, DLT), so the same source compiled with
// -ffp-contract=off for gfx950 and for x86-64 returns the same bits.  The rules are DESIGN.md §9 (rank 10).
#pragma once
#include "orbx_ba_math.h"
#include "orbx_tri_math.h"

// = include/orbx.h: orbx_lm_status
enum { LM_OK = 0, LM_BASELINE = 1, LM_EMPTY = 2, LM_BAD_POSE = 3 };
// the reference's gate on the distance of the first two cameras (src/with_bundle_adjustment.cpp:515-516)
#define LM_BASELINE_MIN 0.1
#define LM_BASELINE_MAX 100.0

// rules 1-3 of one window: the camera matrices of poses 0 and 1 (BA's own blocks: angle-axis, translation, world ->
// camera), the gate, and P0 = K [R0 | t0], P1 = K [R1 | t1] (row-major 3x4).  K: row-major 3x3.  Returns LM_OK,
// LM_BASELINE or LM_BAD_POSE; P0 / P1 are written only for LM_OK.
ORBX_PHD int lm_window_prepare(const double* K, const double* pose0, const double* pose1, double* P0, double* P1) {
  ORBX_PNO_CONTRACT
  BaPose A, B;
  ba_pose_prepare(pose0, &A);
  ba_pose_prepare(pose1, &B);
  if (!A.ok || !B.ok) return LM_BAD_POSE;
  const double dx = A.t[0] - B.t[0], dy = A.t[1] - B.t[1], dz = A.t[2] - B.t[2];
  const double b = pose_sqrt((dx * dx + dy * dy) + dz * dz);
  if (b < LM_BASELINE_MIN || b > LM_BASELINE_MAX) return LM_BASELINE;
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
