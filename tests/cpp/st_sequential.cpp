// st_sequential.cpp -- sequential restatement of the four kernels that join overlapping windows into one trajectory
// (src/with_bundle_adjustment.cpp:203, :234-249), the reference of tests/test_stitch_ref.py and
// tests/test_stitch.py.  One window after the other, one frame after the other.  It shares the arithmetic with the
// kernels through orbx_st_math.h; the loops, the order and the layout are written here on their own.
//
// The rules, restated (W windows of L frames, window w at stream frame w * stride, F = (W - 1) * stride + L):
//   1  frame f belongs to window w = min(W - 1, f / stride) at index k = f - w * stride
//   2  rel(w, k) = P(w, 0)^-1 P(w, k)
//   3  lambda(w + 1) = b_link(w) / b_first(w + 1) when asked for and usable, else 1 (and SCALE_UNALIGNED when asked for)
//   4  a window with an entry that is not finite: identity motions, lambda 1, baselines 0, BROKEN
//   5  G(0) = T_start, G(w + 1) = G(w) [R_rel(w, stride) | Lambda(w) t_rel(w, stride)], a left fold
//   6  trajectory[f] = G(w) [R_rel(w, k) | Lambda(w) t_rel(w, k)]
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC st_sequential.cpp
#include <cstdint>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_st_math.h"

extern "C" {

// k_st_scale0: scale (n * (L - 1)) the tracks-pose block's scales; scale0 (n) out
void seq_st_scale0(int n, int L, int stride, double scale0_first, const double* scale, double* scale0) {
  scale0[0] = scale0_first;
  for (int w = 1; w < n; w++) {
    const long long p = st_scale0_pair(w, L, stride);
    scale0[w] = p >= 0 ? scale[p] : 1.0;
  }
}

// k_st_links, k_st_fold, k_st_apply: poses (n, L, 16); T_start 16 doubles or NULL; out: trajectory (F, 16), owner (F),
// anchors (n, 16), lambda (n), status (n)
void seq_st_stitch(int n, int L, int stride, const double* poses, const double* T_start, int align_scale,
                   double* trajectory, int32_t* owner, double* anchors, double* lambda, int32_t* status) {
  std::vector<double> links((size_t)ST_LINK_DOUBLES * n);
  std::vector<int32_t> broken((size_t)n);
  for (int w = 0; w < n; w++)
    broken[(size_t)w] = st_link(poses + 16 * (size_t)w * L, L, stride, links.data() + (size_t)ST_LINK_DOUBLES * w);
  double G[16], Lam, b_link_prev = 0.0;
  st_fold_begin(T_start, G, &Lam);
  for (int w = 0; w < n; w++) {
    const double* lk = links.data() + (size_t)ST_LINK_DOUBLES * w;
    status[w] = st_fold_step(w, lk, broken[(size_t)w], b_link_prev, align_scale, G, &Lam, anchors + 16 * (size_t)w,
                             lambda + w);
    b_link_prev = lk[13];
  }
  const int F = (n - 1) * stride + L;
  for (int f = 0; f < F; f++)
    owner[f] = st_apply(f, n, L, stride, poses, anchors, lambda, status, trajectory + 16 * (size_t)f);
}

}  // extern "C"
