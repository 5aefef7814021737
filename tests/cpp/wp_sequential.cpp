// wp_sequential.cpp -- sequential restatement of the window-pose chain and of the write-back gate (DESIGN.md §9 rank
// 14; src/with_bundle_adjustment.cpp:196-208, :615-628, :683-718), the reference of tests/test_window_poses_ref.py and
// tests/test_window_poses.py.  One window after the other, one frame after the other.  It shares the arithmetic with
// the kernels through orbx_wp_math.h; the loops, the order and the layout are written here on their own.
//
// The rules, restated:
//   1  C_0 = T0 (identity without one); C_{k+1} = C_k [R_k^T | -s_k R_k^T t_k], s_0 = scale0, s_k = scale[k] after
//   2  (R_wc, t_wc) = C_k^-1 in closed form; poses6 = (log of R_wc through the unit quaternion, t_wc)
//   3  status NONFINITE iff any of the window's 22 L numbers is not finite
//   4  the gate per pose: updated iff termination == CONVERGENCE and |log(R(new) R(old)^T)| < max_rot and
//      |t_new - t_old| < max_trans; the 4x4 out is the inverse of the block that holds afterwards
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC wp_sequential.cpp
#include <cstdint>

#include "../../visual-odometry-gpu_amd/csrc/orbx_wp_math.h"

extern "C" {

// R (n, L - 1, 9), t (n, L - 1, 3), scale (n, L - 1); T0 (n, 16) or NULL; scale0 (n) or NULL
void seq_wp_chain(int n, int L, const double* T0, const double* scale0, const double* R, const double* t,
                  const double* scale, double* poses6, double* poses4x4, int32_t* status) {
  for (int w = 0; w < n; w++) {
    const size_t p = (size_t)w * (L - 1), f = (size_t)w * L;
    status[w] = wp_chain_window(T0 ? T0 + 16 * (size_t)w : nullptr, R + 9 * p, 9, t + 3 * p, 3, scale + p, 1,
                                scale0 ? scale0[w] : 1.0, L, poses4x4 + 16 * f, poses6 + 6 * f);
  }
}

// solved / built (n, L, 6), termination (n); out: poses4x4 (n, L, 16), updated (n, L) bytes, angle / dist (n, L)
void seq_wp_gate(int n, int L, const double* solved, const double* built, const int32_t* termination, double max_rot,
                 double max_trans, double* poses4x4, uint8_t* updated, double* angle, double* dist) {
  for (int w = 0; w < n; w++)
    for (int i = 0; i < L; i++) {
      const size_t k = (size_t)w * L + i;
      updated[k] = (uint8_t)wp_gate(solved + 6 * k, built + 6 * k, termination[w], max_rot, max_trans,
                                    poses4x4 + 16 * k, angle + k, dist + k);
    }
}

double seq_wp_atan2(double y, double x) { return wp_atan2(y, x); }
void seq_wp_atan2_many(int n, const double* y, const double* x, double* out) {
  for (int i = 0; i < n; i++) out[i] = wp_atan2(y[i], x[i]);
}
void seq_wp_rodrigues_inv(const double* R, double* w) { wp_rodrigues_inv(R, w); }

}  // extern "C"
