// lm_sequential.cpp -- sequential restatement of the landmark building of tracked windows (DESIGN.md §9 rank 10;
// the reference's buildLandmarksFromFirstTwoFramesAndTracks, src/with_bundle_adjustment.cpp:502-575), the reference
// of tests/test_landmarks_ref.py and tests/test_landmarks.py.  One window after the other, one slot after the other,
// std::vector storage, push_back compaction.  It shares rules 1-4 (gate, projections, DLT, depth check) with the
// kernels through orbx_lm_math.h; the loops, the order and the layout are written here on their own.
//
// The rules, restated:
//   1  poses 0 and 1 of a window through ba_pose_prepare; one that is not ok: status BAD_POSE
//   2  b = sqrt(|t0 - t1|^2), summed left to right; b < 0.1 or b > 100: status BASELINE, no landmarks
//   3  P0 = K [R0 | t0], P1 = K [R1 | t1]; every slot with seen >= 2: the DLT of its first two pixels (float widened
//      to double) in WORLD coordinates; X = h[0..2] / h[3] in binary64; valid iff h[3] != 0 and X is finite
//   4  kept iff valid and X[2] > 0
//   5  kept landmarks in ascending slot order, each with observations k = 0 .. seen - 1 in ascending k
//   6  the gate passed and nothing kept: EMPTY; a window that is not OK owns nothing
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC lm_sequential.cpp
#include <cstdint>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_lm_math.h"

namespace {

struct Window {
  int status = LM_OK;
  std::vector<double> points;  // 3 per landmark
  std::vector<int32_t> slot, obs_point, obs_pose;
  std::vector<double> obs_xy;
};

Window build(const double* K9, int window_len, int cap, const double* poses6, const float* tracks,
             const int32_t* seen) {
  Window w;
  double P0[12], P1[12];
  w.status = lm_window_prepare(K9, poses6, poses6 + 6, P0, P1);
  if (w.status != LM_OK) return w;
  for (int s = 0; s < cap; s++) {
    const int n = lm_seen(seen[s], window_len);
    if (n < 2) continue;
    const float* t = tracks + 2 * (size_t)window_len * s;
    double X[3];
    if (!lm_point(P0, P1, t[0], t[1], t[2], t[3], X)) continue;
    const int32_t j = (int32_t)w.slot.size();
    w.slot.push_back(s);
    for (int k = 0; k < 3; k++) w.points.push_back(X[k]);
    for (int k = 0; k < n; k++) {
      w.obs_point.push_back(j);
      w.obs_pose.push_back(k);
      w.obs_xy.push_back((double)t[2 * k]);
      w.obs_xy.push_back((double)t[2 * k + 1]);
    }
  }
  if (w.slot.empty()) w.status = LM_EMPTY;
  return w;
}

}  // namespace

extern "C" {

// n_windows windows in the layout of orbx_lk_windows_view; status [n], point_offset / obs_offset [n + 1]; the landmark
// arrays are sized by the caller for every slot kept (n * cap landmarks, n * cap * window_len observations)
void seq_lm_build(const double* K9, int n_windows, int cap, int window_len, const double* poses6, const float* tracks,
                  const int32_t* seen, int32_t* status, int32_t* point_offset, int32_t* obs_offset, double* points3,
                  int32_t* slot_of_point, int32_t* obs_point, int32_t* obs_pose, double* obs_xy) {
  size_t np = 0, no = 0;
  point_offset[0] = obs_offset[0] = 0;
  for (int w = 0; w < n_windows; w++) {
    const Window W = build(K9, window_len, cap, poses6 + 6 * (size_t)window_len * w,
                           tracks + 2 * (size_t)window_len * cap * w, seen + (size_t)cap * w);
    status[w] = W.status;
    for (size_t i = 0; i < W.slot.size(); i++) slot_of_point[np + i] = W.slot[i];
    for (size_t i = 0; i < W.points.size(); i++) points3[3 * np + i] = W.points[i];
    for (size_t i = 0; i < W.obs_point.size(); i++) {
      obs_point[no + i] = W.obs_point[i];
      obs_pose[no + i] = W.obs_pose[i];
      obs_xy[2 * (no + i)] = W.obs_xy[2 * i];
      obs_xy[2 * (no + i) + 1] = W.obs_xy[2 * i + 1];
    }
    np += W.slot.size();
    no += W.obs_point.size();
    point_offset[w + 1] = (int32_t)np;
    obs_offset[w + 1] = (int32_t)no;
  }
}

// rule 3 on one pixel pair with given projection matrices: the three quotients and the keep decision
int seq_lm_point(const double* P0, const double* P1, float x0, float y0, float x1, float y1, double* X) {
  return lm_point(P0, P1, x0, y0, x1, y1, X) ? 1 : 0;
}

// rules 1-2 and the projections of one window
int seq_lm_prepare(const double* K9, const double* pose0, const double* pose1, double* P0, double* P1) {
  return lm_window_prepare(K9, pose0, pose1, P0, P1);
}

}  // extern "C"
