// orbx_wp_math.h -- the arithmetic between the pair motions of a tracked window and its bundle adjustment, and behind
// it: the window's camera -> world poses chained from (R, t, scale) per pair (src/with_bundle_adjustment.cpp:196-208),
// their world -> camera angle-axis blocks (:615-628, pose.inv() -> cv::Rodrigues) and the write-back gate of the solve
// (:683-718).  Shared by the gfx950 kernels (orbx_wposes.hip), the host entry orbx_chain_window_poses and the
// sequential restatement (tests/cpp/wp_sequential.cpp).  Binary64 built from IEEE + - * /, pose_sqrt and integer
// operations only (atan2 is restated below), so the same source compiled with -ffp-contract=off for gfx950 and for
// x86-64 returns the same bits.  The rules are DESIGN.md §9 (rank 14).
#pragma once
#include "orbx_ba_math.h"
#include "orbx_tri_math.h"

// = include/orbx_vo.h: orbx_wp_status
enum { WP_OK = 0, WP_NONFINITE = 1 };

// ---- atan2(y, x) for y >= 0: fdlibm's s_atan.c (argument reduction at 7/16, 11/16, 19/16, 39/16, the odd polynomial
// of degree 23 split into its even and odd halves) behind e_atan2.c's quadrant logic, cut down to the quadrants a
// non-negative y reaches.  Returns a value in [0, pi]; a NaN argument returns NaN ------------------------------------
ORBX_PHD double wp_atan(double x) {  // x >= 0
  ORBX_PNO_CONTRACT
  const double hi0 = 4.63647609000806093515e-01, hi1 = 7.85398163397448278999e-01, hi2 = 9.82793723247329054082e-01,
               hi3 = 1.57079632679489655800e+00;
  const double lo0 = 2.26987774529616870924e-17, lo1 = 3.06161699786838301793e-17, lo2 = 1.39033110312309984516e-17,
               lo3 = 6.12323399573676603587e-17;
  const double a0 = 3.33333333333329318027e-01, a1 = -1.99999999998764832476e-01, a2 = 1.42857142725034663711e-01,
               a3 = -1.11111104054623557880e-01, a4 = 9.09088713343650656196e-02, a5 = -7.69187620504482999495e-02,
               a6 = 6.66107313738753120669e-02, a7 = -5.83357013379057348645e-02, a8 = 4.97687799461593236017e-02,
               a9 = -3.65315727442169155270e-02, a10 = 1.62858201153657823623e-02;
  const uint32_t ix = (uint32_t)(pose_d2u(x) >> 32) & 0x7fffffffu;
  if (ix >= 0x44100000u) {  // x >= 2^66, or a NaN
    if (x != x) return x;
    return hi3 + lo3;
  }
  double hi = 0.0, lo = 0.0;
  bool reduced = true;
  if (ix < 0x3fdc0000u) {  // x < 7/16
    if (ix < 0x3e200000u) return x;  // x < 2^-29
    reduced = false;
  } else if (ix < 0x3ff30000u) {
    if (ix < 0x3fe60000u) {  // 7/16 <= x < 11/16
      hi = hi0, lo = lo0;
      x = (2.0 * x - 1.0) / (2.0 + x);
    } else {  // 11/16 <= x < 19/16
      hi = hi1, lo = lo1;
      x = (x - 1.0) / (x + 1.0);
    }
  } else if (ix < 0x40038000u) {  // 19/16 <= x < 39/16
    hi = hi2, lo = lo2;
    x = (x - 1.5) / (1.0 + 1.5 * x);
  } else {  // 39/16 <= x < 2^66
    hi = hi3, lo = lo3;
    x = -1.0 / x;
  }
  const double z = x * x;
  const double w = z * z;
  const double s1 = z * (a0 + w * (a2 + w * (a4 + w * (a6 + w * (a8 + w * a10)))));
  const double s2 = w * (a1 + w * (a3 + w * (a5 + w * (a7 + w * a9))));
  if (!reduced) return x - x * (s1 + s2);
  return hi - ((x * (s1 + s2) - lo) - x);
}
ORBX_PHD double wp_atan2(double y, double x) {  // y >= 0
  ORBX_PNO_CONTRACT
  const double pi = 3.1415926535897931160e+00, pi_lo = 1.2246467991473531772e-16, pi_o_2 = 1.5707963267948965580e+00;
  if (x != x || y != y) return x + y;
  if (x == 1.0) return wp_atan(y);
  const uint64_t ux = pose_d2u(x), uy = pose_d2u(y);
  const bool xneg = (ux >> 63) != 0;  // (the sign bit: x = -0 counts as negative, as in fdlibm)
  if (y == 0.0) return xneg ? pi : y;
  if (x == 0.0) return pi_o_2;
  const int k = ((int)((uy >> 32) & 0x7fffffffu) - (int)((ux >> 32) & 0x7fffffffu)) >> 20;
  double z;
  if (k > 60) {  // y / |x| > 2^60
    z = pi_o_2 + 0.5 * pi_lo;
  } else if (xneg && k < -60) {  // y / |x| < 2^-60 left of the origin
    z = 0.0;
  } else {
    z = wp_atan(pose_abs(y / x));
  }
  return xneg ? pi - (z - pi_lo) : z;
}

// ---- rigid motions: row-major 3x3 R, 3-vector t, row-major 4x4 T -----------------------------------------------
// world -> camera [R | t] of a camera -> world pose: the reference's pose.inv() in closed form
ORBX_PHD void wp_invert_rigid(const double* T, double* R, double* t) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
ORBX_PUNROLL
    for (int j = 0; j < 3; j++) R[i * 3 + j] = T[j * 4 + i];
  }
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) t[i] = -(R[i * 3] * T[3] + R[i * 3 + 1] * T[7] + R[i * 3 + 2] * T[11]);
}
// ([R | t])^-1 as a 4x4
ORBX_PHD void wp_compose_inverse(const double* R, const double* t, double* T) {
  ORBX_PNO_CONTRACT
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
ORBX_PUNROLL
    for (int j = 0; j < 3; j++) T[i * 4 + j] = R[j * 3 + i];
    T[i * 4 + 3] = -(R[0 * 3 + i] * t[0] + R[1 * 3 + i] * t[1] + R[2 * 3 + i] * t[2]);
  }
  T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
}
// the quaternion of the branch 1 + tr R < 1e-3, around the largest diagonal entry i (j, k follow it cyclically)
ORBX_PHD void wp_quat_near_pi(const double* R, int i, int j, int k, double* q) {
  ORBX_PNO_CONTRACT
  q[1 + i] = 1.0 + R[i * 4] - R[j * 4] - R[k * 4];
  q[1 + j] = R[i * 3 + j] + R[j * 3 + i];
  q[1 + k] = R[i * 3 + k] + R[k * 3 + i];
  q[0] = R[k * 3 + j] - R[j * 3 + k];
}
// cv::Rodrigues, matrix -> vector, angle in [0, pi] (through the unit quaternion: stable near pi)
ORBX_PHD void wp_rodrigues_inv(const double* R, double* w) {
  ORBX_PNO_CONTRACT
  double q[4] = {1.0 + R[0] + R[4] + R[8], R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  if (q[0] < 1e-3) {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > (i == 0 ? R[0] : R[4])) i = 2;
    if (i == 0) wp_quat_near_pi(R, 0, 1, 2, q);
    else if (i == 1) wp_quat_near_pi(R, 1, 2, 0, q);
    else wp_quat_near_pi(R, 2, 0, 1, q);
  }
  const double n = pose_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sg = q[0] < 0 ? -1.0 : 1.0;
ORBX_PUNROLL
  for (int i = 0; i < 4; i++) q[i] = sg * q[i] / n;
  const double s = pose_sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double f = s > 0 ? 2.0 * wp_atan2(s, q[0]) / s : 0.0;
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) w[i] = f * q[1 + i];
}

ORBX_PHD bool wp_finite(double x) { return (pose_d2u(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// one frame of a window: the camera -> world pose C as it is, and its block (angle-axis of R_wc, t_wc); returns
// whether all 22 numbers are finite
ORBX_PHD bool wp_emit(const double* C, double* pose4x4, double* pose6) {
  double R[9], t[3], w[3];
  wp_invert_rigid(C, R, t);
  wp_rodrigues_inv(R, w);
  bool fin = true;
ORBX_PUNROLL
  for (int i = 0; i < 16; i++) {
    pose4x4[i] = C[i];
    fin = fin && wp_finite(C[i]);
  }
ORBX_PUNROLL
  for (int i = 0; i < 3; i++) {
    pose6[i] = w[i], pose6[3 + i] = t[i];
    fin = fin && wp_finite(w[i]) && wp_finite(t[i]);
  }
  return fin;
}

// One window of L frames: C_0 = T0 (NULL: identity), C_{k+1} = C_k [R_k^T | -s_k R_k^T t_k] (tri_chain: the product
// orbx_chain_trajectory forms), s_0 = scale0 and s_k = scale[k * scale_stride] from pair 1 on; R, t, scale are read
// with strides in doubles, so that the kernel reads the tracks-pose block in place.  Writes 16 L and 6 L doubles;
// returns WP_OK or WP_NONFINITE.
ORBX_PHD int wp_chain_window(const double* T0, const double* R, int r_stride, const double* t, int t_stride,
                             const double* scale, int scale_stride, double scale0, int L, double* poses4x4,
                             double* poses6) {
  double C[16];
ORBX_PUNROLL
  for (int i = 0; i < 16; i++) C[i] = T0 ? T0[i] : (i % 5 == 0 ? 1.0 : 0.0);
  bool fin = wp_emit(C, poses4x4, poses6);
  for (int k = 0; k + 1 < L; k++) {
    const double s = k == 0 ? scale0 : scale[(size_t)k * scale_stride];
    tri_chain(C, R + (size_t)k * r_stride, t + (size_t)k * t_stride, s, C);
    const bool f = wp_emit(C, poses4x4 + 16 * (size_t)(k + 1), poses6 + 6 * (size_t)(k + 1));
    fin = fin && f;
  }
  return fin ? WP_OK : WP_NONFINITE;
}

// The write-back gate of one pose (src/with_bundle_adjustment.cpp:683-718): the block after the solve (pnew) against
// the block as built (pold).  angle = |log(R(new) R(old)^T)|, d = |t_new - t_old| on the world -> camera
// translations; the pose is updated iff the solve converged and angle < max_rot and d < max_trans (a NaN fails).
// T receives the camera -> world 4x4 of the block that holds afterwards.  Returns 1 when updated.
ORBX_PHD int wp_gate(const double* pnew, const double* pold, int termination, double max_rot, double max_trans,
                     double* T, double* angle, double* dist) {
  ORBX_PNO_CONTRACT
  BaPose A, B;
  ba_pose_prepare(pnew, &A);
  ba_pose_prepare(pold, &B);
  double Rd[9], wd[3];
ORBX_PUNROLL
  for (int a = 0; a < 3; a++) {
ORBX_PUNROLL
    for (int b = 0; b < 3; b++)
      Rd[a * 3 + b] = A.R[a * 3] * B.R[b * 3] + A.R[a * 3 + 1] * B.R[b * 3 + 1] + A.R[a * 3 + 2] * B.R[b * 3 + 2];
  }
  wp_rodrigues_inv(Rd, wd);
  *angle = pose_sqrt(wd[0] * wd[0] + wd[1] * wd[1] + wd[2] * wd[2]);
  double tn = 0.0;
ORBX_PUNROLL
  for (int k = 0; k < 3; k++) tn = tn + (A.t[k] - B.t[k]) * (A.t[k] - B.t[k]);
  *dist = pose_sqrt(tn);
  const int updated = termination == BA_CONVERGENCE && *angle < max_rot && *dist < max_trans ? 1 : 0;
  if (updated) wp_compose_inverse(A.R, A.t, T);
  else wp_compose_inverse(B.R, B.t, T);
  return updated;
}
