// orbx_search_math.h -- the arithmetic of the search by projection: a landmark projected into a
// predicted view (rules P2-P5) and the position gate of the re-association (rule L).  Shared by the gfx950 kernels
// (orbx_search.hip), the host layer and the sequential restatement (tests/cpp/search_sequential.cpp).  Binary64 built
// from IEEE + - * /, compares and what orbx_pnp_math.h is built from, so the same source compiled with
// -ffp-contract=off for gfx950 and for x86-64 returns the same bits.  The reference keeps no point across a solve
// (src/with_bundle_adjustment.cpp:586-593) and matches without geometry (src/feature_tracking.cpp:203-219).
#pragma once
#include "orbx_pnp_math.h"

// = include/orbx_search.h: orbx_proj_state
enum { SP_NONE = 0, SP_BEHIND = 1, SP_OUTSIDE = 2, SP_OK = 3 };

// rule P2: the model of a predicted pose (R row-major, then t); false when ba_pose_prepare does not accept the pose (a
// component that is not finite, or an angle beyond BA_MAX_THETA)
ORBX_PHD bool sp_pose_model(const double* pose6, double* M) {
  bool fin = true;
  for (int i = 0; i < 6; i++) fin = fin && wp_finite(pose6[i]);
  BaPose P;
  ba_pose_prepare(pose6, &P);
  pnp_pose_to_model(P, M);
  return fin && P.ok != 0;
}

// rules P3-P5 for one landmark X under the model M; K4 = fx, fy, cx, cy.  The three sums and the two quotients are
// pnp_inlier's, in its association order, so the pixel is bit for bit the one PnP scored.  out3 = u, v, depth; zeros
// unless the state is SP_OK.
ORBX_PHD int sp_project(const double* K4, const double* M, const double* X, int width, int height, double margin_px,
                        double* out3) {
  ORBX_PNO_CONTRACT
  out3[0] = 0.0, out3[1] = 0.0, out3[2] = 0.0;
  const double p0 = ((M[0] * X[0] + M[1] * X[1]) + M[2] * X[2]) + M[9];
  const double p1 = ((M[3] * X[0] + M[4] * X[1]) + M[5] * X[2]) + M[10];
  const double p2 = ((M[6] * X[0] + M[7] * X[1]) + M[8] * X[2]) + M[11];
  if (!(p2 > 0.0)) return SP_BEHIND;
  const double u = K4[0] * p0 / p2 + K4[2], v = K4[1] * p1 / p2 + K4[3];
  const double lo = -margin_px, hi_u = (double)(width - 1) + margin_px, hi_v = (double)(height - 1) + margin_px;
  if (!(wp_finite(u) && wp_finite(v) && u >= lo && u <= hi_u && v >= lo && v <= hi_v)) return SP_OUTSIDE;
  out3[0] = u, out3[1] = v, out3[2] = p2;
  return SP_OK;
}

// rule L: the query at (qx, qy), two floats, and the train slot at (tx, ty), two doubles, lie within the gate of
// squared radius r2 = radius_px * radius_px.  Every difference, product and sum is rounded once; a pair exactly on the
// circle is inside.
ORBX_PHD bool sp_in_gate(float qx, float qy, double tx, double ty, double r2) {
  ORBX_PNO_CONTRACT
  const double dx = (double)qx - tx, dy = (double)qy - ty;
  const double xx = dx * dx, yy = dy * dy;
  return xx + yy <= r2;
}
