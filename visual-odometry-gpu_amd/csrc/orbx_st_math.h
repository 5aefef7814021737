// orbx_st_math.h -- the arithmetic that joins overlapping tracked windows into one trajectory: what the reference does
// frame by frame with cur_pose = prev_pose * T.inv() and cur_pose = pose_window.back() after every solve
// (src/with_bundle_adjustment.cpp:203, :234-249), restated for windows that were chained, solved and gated each in a
// frame of its own.  Shared by the gfx950 kernels (orbx_stitch.hip), the host entry orbx_stitch_windows and the
// sequential restatement (tests/cpp/st_sequential.cpp).  Binary64 built from IEEE + - * /, pose_sqrt and integer
// operations only, so the same source compiled with -ffp-contract=off for gfx950 and for x86-64 returns the same
// bits.  The rules are DESIGN.md §9 (rank 16).
//
// A stream of W windows of L frames, window w starting at stream frame w * stride, 1 <= stride <= L - 1, has
// F = (W - 1) * stride + L frames.  P(w, k) is the camera -> world pose of frame k of window w in the window's own
// gauge (row-major 4x4), c(w, k) its camera centre.
#pragma once
#include "orbx_wp_math.h"

// = include/orbx_stream.h: the bits of orbx_stitch_view.status
enum { ST_OK = 0, ST_BROKEN = 1, ST_SCALE_UNALIGNED = 2 };

// what k_st_links leaves per window: R_rel(w, stride) | t_rel(w, stride) | b_first | b_link, and the broken flag
#define ST_LINK_DOUBLES 14

// ---- rule 1: the owner of stream frame f: the latest window that contains it ---------------------------------------
ORBX_PHD int st_owner(int f, int n_windows, int stride) {
  const int w = f / stride;
  return w < n_windows - 1 ? w : n_windows - 1;
}
// the frames of a stream; 0 when the sizes are no stream or the count leaves 31 bits
ORBX_PHD int st_frames(int n_windows, int window_len, int stride) {
  if (n_windows < 1 || window_len < 2 || stride < 1 || stride > window_len - 1) return 0;
  const long long f = (long long)(n_windows - 1) * stride + window_len;
  return f > 0x7fffffffll / 16 ? 0 : (int)f;
}
// the pair of the tracks-pose block whose scale is the scale of pair 0 of window w >= 1: pair `stride` of window
// w - 1, which covers the same two frames; -1 when stride == L - 1 (no such pair: the scale is 1)
ORBX_PHD long long st_scale0_pair(int w, int window_len, int stride) {
  return stride <= window_len - 2 ? (long long)(w - 1) * (window_len - 1) + stride : -1;
}

// ---- rule 2: rel = P0^-1 Pk as (R, t); the inverse in closed form, every dot product summed left to right ----------
ORBX_PHD void st_rel(const double* P0, const double* Pk, double* R, double* t) {
  ORBX_PNO_CONTRACT
  double Ri[9], ti[3];
  wp_invert_rigid(P0, Ri, ti);
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
ORBX_PUNROLL
    for (int j = 0; j < 3; j++)
      R[i * 3 + j] = (Ri[i * 3] * Pk[j] + Ri[i * 3 + 1] * Pk[4 + j]) + Ri[i * 3 + 2] * Pk[8 + j];
    t[i] = ((Ri[i * 3] * Pk[3] + Ri[i * 3 + 1] * Pk[7]) + Ri[i * 3 + 2] * Pk[11]) + ti[i];
  }
}
ORBX_PHD void st_identity(double* R, double* t) {
ORBX_PUNROLL
  for (int i = 0; i < 9; i++) R[i] = i % 4 == 0 ? 1.0 : 0.0;
  t[0] = 0.0, t[1] = 0.0, t[2] = 0.0;
}
// out = G [R | s t] for the rigid G (row-major 4x4; its bottom row is not read): the bottom row written is 0 0 0 1
ORBX_PHD void st_compose(const double* G, const double* R, const double* t, double s, double* out) {
  ORBX_PNO_CONTRACT
  double o[16];
  const double st[3] = {s * t[0], s * t[1], s * t[2]};
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
ORBX_PUNROLL
    for (int j = 0; j < 3; j++)
      o[i * 4 + j] = (G[i * 4] * R[j] + G[i * 4 + 1] * R[3 + j]) + G[i * 4 + 2] * R[6 + j];
    o[i * 4 + 3] = ((G[i * 4] * st[0] + G[i * 4 + 1] * st[1]) + G[i * 4 + 2] * st[2]) + G[i * 4 + 3];
  }
  o[12] = 0.0, o[13] = 0.0, o[14] = 0.0, o[15] = 1.0;
ORBX_PUNROLL
  for (int i = 0; i < 16; i++) out[i] = o[i];
}

// ---- rule 3: the distance of two camera centres ----------------------------------------------------------------
ORBX_PHD double st_baseline(const double* Pa, const double* Pb) {
  ORBX_PNO_CONTRACT
  const double dx = Pb[3] - Pa[3], dy = Pb[7] - Pa[7], dz = Pb[11] - Pa[11];
  return pose_sqrt((dx * dx + dy * dy) + dz * dz);
}
ORBX_PHD bool st_usable(double b) { return wp_finite(b) && b > 0.0; }

// ---- rules 2-4 of one window: P = its L poses.  link receives R_rel(stride) | t_rel(stride) | b_first | b_link
// (b_link is 0 when stride == L - 1: no frame stride + 1); a broken window has the identity and both baselines 0, so
// that the window behind it stays unaligned.  Returns 1 when the window is broken ------------------------------------
ORBX_PHD int st_link(const double* P, int L, int stride, double* link) {
  bool fin = true;
  for (int i = 0; i < 16 * L; i++) fin = fin && wp_finite(P[i]);
  if (!fin) {
    st_identity(link, link + 9);
    link[12] = 0.0, link[13] = 0.0;
    return 1;
  }
  st_rel(P, P + 16 * (size_t)stride, link, link + 9);
  link[12] = st_baseline(P, P + 16);
  link[13] = stride <= L - 2 ? st_baseline(P + 16 * (size_t)stride, P + 16 * (size_t)(stride + 1)) : 0.0;
  return 0;
}

// ---- rule 3: lambda(w) of window w >= 1 from b_link(w - 1) and b_first(w); *unaligned: the factor had to be 1 ------
ORBX_PHD double st_lambda(double b_link_prev, double b_first, int align_scale, int* unaligned) {
  ORBX_PNO_CONTRACT
  *unaligned = 0;
  if (!align_scale) return 1.0;
  if (st_usable(b_link_prev) && st_usable(b_first)) {
    const double q = b_link_prev / b_first;
    if (st_usable(q)) return q;
  }
  *unaligned = 1;
  return 1.0;
}

// ---- rule 5: the left fold, one window at a time and in window order.  G(0) = T_start (NULL: identity; its bottom
// row is written as 0 0 0 1), Lambda(0) = 1 ------------------------------------------------------------------------
ORBX_PHD void st_fold_begin(const double* T_start, double* G, double* Lam) {
ORBX_PUNROLL
  for (int i = 0; i < 12; i++) G[i] = T_start ? T_start[i] : (i % 5 == 0 ? 1.0 : 0.0);
  G[12] = 0.0, G[13] = 0.0, G[14] = 0.0, G[15] = 1.0;
  *Lam = 1.0;
}
// window w: (G, Lam) come in as G(w), Lambda(w - 1) and leave as G(w + 1), Lambda(w).  link / is_broken: the window's
// own; b_link_prev: b_link(w - 1), not read for w == 0.  Writes the window's anchor and Lambda; returns its status
ORBX_PHD int st_fold_step(int w, const double* link, int is_broken, double b_link_prev, int align_scale, double* G,
                          double* Lam, double* anchor4x4, double* lambda) {
  ORBX_PNO_CONTRACT
  int st = ST_OK;
  if (is_broken) {
    st = ST_BROKEN;  // lambda(w) = 1
  } else if (w > 0) {
    int un;
    *Lam = *Lam * st_lambda(b_link_prev, link[12], align_scale, &un);
    if (un) st = ST_SCALE_UNALIGNED;
  }
ORBX_PUNROLL
  for (int i = 0; i < 16; i++) anchor4x4[i] = G[i];
  *lambda = *Lam;
  st_compose(G, link, link + 9, *Lam, G);
  return st;
}

// ---- rule 6: stream frame f: trajectory[f] = G(w) [R_rel(w, k) | Lambda(w) t_rel(w, k)]; returns the owner ---------
ORBX_PHD int st_apply(int f, int n_windows, int window_len, int stride, const double* poses4x4,
                      const double* anchors4x4, const double* lambda, const int32_t* status, double* out) {
  const int w = st_owner(f, n_windows, stride), k = f - w * stride;
  const double* P = poses4x4 + 16 * (size_t)w * window_len;
  double R[9], t[3];
  if (status[w] & ST_BROKEN) st_identity(R, t);
  else st_rel(P, P + 16 * (size_t)k, R, t);
  st_compose(anchors4x4 + 16 * (size_t)w, R, t, lambda[w], out);
  return w;
}
