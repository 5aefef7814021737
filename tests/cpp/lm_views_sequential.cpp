// lm_views_sequential.cpp -- sequential restatement of the landmarks build from every view of a track with its
// reprojection gate (include/orbx_lm.h), the reference of tests/test_landmarks_views_ref.py and
// tests/test_landmarks_views.py.  One window after the other, one slot after the other, std::vector storage, push_back
// compaction.  It shares the per-view and per-row arithmetic with the kernels through orbx_lm_math.h; the loops over
// views, the order of the checks and the layout are written here on their own.
//
// The rules, restated (sn = seen clamped into [0, window_len]):
//   1  the views prepared: 2 for FIRST_TWO without a gate, window_len otherwise; a prepared pose that is not ok: status
//      BAD_POSE; then the baseline gate of rank 10 on the translations of poses 0 and 1
//   2  FIRST_TWO uses views {0, 1}, WIDEST {0, sn - 1}, ALL_VIEWS {0 .. sn - 1}; sn < 2: SHORT
//   3  rows in ascending view order, x before y; the upper triangle of A^T A summed row by row starting from the first
//      row's products; the sweeps of tri_homogeneous
//   4  X = h / h[3]; h[3] == 0 or a quotient that is not finite: DEGENERATE
//   5  FIRST_TWO: world z > 0; else the camera depth > 0 in every observed view; a failure: BEHIND
//   6  reproj_px from the largest finite e2 over the observed views, +inf when one is not finite; with a gate, bad or
//      max_e2 > max_reproj_px^2: REPROJECTION.  Observed views: k < sn among the prepared ones
//   7  NO_WINDOW, SHORT, DEGENERATE, BEHIND, REPROJECTION, else KEPT
//   8  kept landmarks in ascending slot order with all sn observations; nothing kept behind a passed gate: EMPTY
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC lm_views_sequential.cpp
// With -DLM_VIEWS_MAIN it is a stand-alone program that builds one mixed window in every mode (for a sanitizer run).
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

struct Verdict {
  int reason;
  float reproj_px;
  double X[3];
};

Verdict judge(const std::vector<double>& table, int n_prep, int tri_mode, bool gated, double max_e2_kept,
              const float* t, int sn) {
  Verdict v{LM_SHORT, 0.f, {0.0, 0.0, 0.0}};
  if (sn < 2) return v;
  std::vector<int> used;
  if (tri_mode == LM_TRI_FIRST_TWO) used = {0, 1};
  if (tri_mode == LM_TRI_WIDEST) used = {0, sn - 1};
  if (tri_mode == LM_TRI_ALL_VIEWS)
    for (int k = 0; k < sn; k++) used.push_back(k);
  double a[4][4], h[4];
  bool first = true;
  for (int k : used) {
    double rows[2][4];
    lm_view_rows(&table[(size_t)LM_VIEW_DOUBLES * k], (double)t[2 * k], (double)t[2 * k + 1], rows[0], rows[1]);
    for (const double* r : {rows[0], rows[1]}) {
      if (first)
        lm_normal_start(a, r);
      else
        lm_normal_add(a, r);
      first = false;
    }
  }
  tri_smallest_eigenvector(a, h);
  v.reason = LM_DEGENERATE;
  if (!lm_quotient(h, v.X)) return v;
  const int observed = sn < n_prep ? sn : n_prep;
  bool behind = false, bad = false;
  double max_e2 = 0.0;
  if (tri_mode == LM_TRI_FIRST_TWO) behind = !(v.X[2] > 0.0);
  for (int k = 0; k < observed; k++) {
    const double* rec = &table[(size_t)LM_VIEW_DOUBLES * k];
    if (tri_mode != LM_TRI_FIRST_TWO && !(lm_view_depth(rec, v.X) > 0.0)) behind = true;
    const double e2 = lm_view_e2(rec, v.X, (double)t[2 * k], (double)t[2 * k + 1]);
    if (!lm_finite(e2))
      bad = true;
    else if (e2 > max_e2)
      max_e2 = e2;
  }
  v.reproj_px = lm_reproj_px(max_e2, bad);
  if (behind)
    v.reason = LM_BEHIND;
  else if (gated && (bad || max_e2 > max_e2_kept))
    v.reason = LM_REPROJECTION;
  else
    v.reason = LM_KEPT;
  return v;
}

Window build(const double* K9, int window_len, int cap, const double* poses6, const float* tracks,
             const int32_t* seen, int tri_mode, double max_reproj_px, int pose_status, uint8_t* reason,
             float* reproj_px) {
  Window w;
  const int n_prep = lm_views_prepared(tri_mode, max_reproj_px, window_len);
  std::vector<double> table((size_t)LM_VIEW_DOUBLES * window_len, 0.0);
  bool all_ok = true;
  for (int k = 0; k < n_prep; k++)
    if (!lm_view_prepare(K9, poses6 + 6 * k, &table[(size_t)LM_VIEW_DOUBLES * k])) all_ok = false;
  w.status = all_ok ? lm_baseline(poses6 + 3, poses6 + 9) : LM_BAD_POSE;
  if (pose_status != 0) w.status = LM_BAD_POSE;
  for (int s = 0; s < cap; s++) {
    reason[s] = LM_NO_WINDOW;
    reproj_px[s] = 0.f;
  }
  if (w.status != LM_OK) return w;
  const bool gated = max_reproj_px > 0.0;
  const double max_e2_kept = max_reproj_px * max_reproj_px;
  for (int s = 0; s < cap; s++) {
    const int sn = lm_seen(seen[s], window_len);
    const float* t = tracks + 2 * (size_t)window_len * s;
    const Verdict v = judge(table, n_prep, tri_mode, gated, max_e2_kept, t, sn);
    reason[s] = (uint8_t)v.reason;
    reproj_px[s] = v.reproj_px;
    if (v.reason != LM_KEPT) continue;
    const int32_t j = (int32_t)w.slot.size();
    w.slot.push_back(s);
    for (int k = 0; k < 3; k++) w.points.push_back(v.X[k]);
    for (int k = 0; k < sn; k++) {
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

// seq_lm_build's arguments (tests/cpp/lm_sequential.cpp), then the two options, pose_status (NULL, or one per window:
// not 0 is a chain that is not finite) and reason / reproj_px [n_windows][cap]
void seq_lm_views_build(const double* K9, int n_windows, int cap, int window_len, const double* poses6,
                        const float* tracks, const int32_t* seen, int32_t* status, int32_t* point_offset,
                        int32_t* obs_offset, double* points3, int32_t* slot_of_point, int32_t* obs_point,
                        int32_t* obs_pose, double* obs_xy, int tri_mode, double max_reproj_px,
                        const int32_t* pose_status, uint8_t* reason, float* reproj_px) {
  size_t np = 0, no = 0;
  point_offset[0] = obs_offset[0] = 0;
  for (int w = 0; w < n_windows; w++) {
    const Window W = build(K9, window_len, cap, poses6 + 6 * (size_t)window_len * w,
                           tracks + 2 * (size_t)window_len * cap * w, seen + (size_t)cap * w, tri_mode, max_reproj_px,
                           pose_status ? pose_status[w] : 0, reason + (size_t)cap * w, reproj_px + (size_t)cap * w);
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

}  // extern "C"

#ifdef LM_VIEWS_MAIN
#include <cstdio>
#include <limits>

// one mixed window of 64 slots and 5 views: a camera moving along z, points in front of it and behind it, ragged
// `seen`, one observation moved by 20 px, one observation that is not finite; every mode, without and with the gate
int main() {
  const int W = 5, cap = 64;
  const double K9[9] = {718.856, 0.0, 607.1928, 0.0, 718.856, 185.2157, 0.0, 0.0, 1.0};
  std::vector<double> poses(6 * W, 0.0);
  for (int k = 0; k < W; k++) poses[6 * k + 1] = 0.01 * k, poses[6 * k + 5] = -0.8 * k;
  std::vector<float> tracks(2 * W * cap, 0.f);
  std::vector<int32_t> seen(cap);
  for (int s = 0; s < cap; s++) {
    const double X[3] = {-8.0 + 0.25 * s, -1.0 + 0.03 * s, (s % 7 == 6 ? -1.0 : 1.0) * (6.0 + 0.5 * s)};
    seen[s] = s % (W + 2) - 1;  // -1 .. W: below and inside the clamp
    for (int k = 0; k < W; k++) {
      BaPose P;
      ba_pose_prepare(&poses[6 * k], &P);
      double p[3];
      ba_transform(P, X, p);
      tracks[2 * (W * s + k)] = (float)(K9[0] * p[0] / p[2] + K9[2]);
      tracks[2 * (W * s + k) + 1] = (float)(K9[4] * p[1] / p[2] + K9[5]);
    }
  }
  tracks[2 * (W * 12 + 3)] += 20.f;
  tracks[2 * (W * 19 + 2) + 1] = std::numeric_limits<float>::infinity();
  long long kept_total = 0;
  for (int mode = 0; mode < 3; mode++)
    for (double gate : {0.0, 3.0}) {
      std::vector<int32_t> status(1), po(2), oo(2), slot(cap), op(cap * W), oq(cap * W);
      std::vector<double> pts(3 * cap), oxy(2 * cap * W);
      std::vector<uint8_t> reason(cap);
      std::vector<float> px(cap);
      seq_lm_views_build(K9, 1, cap, W, poses.data(), tracks.data(), seen.data(), status.data(), po.data(), oo.data(),
                         pts.data(), slot.data(), op.data(), oq.data(), oxy.data(), mode, gate, nullptr, reason.data(),
                         px.data());
      int counts[6] = {};
      for (int s = 0; s < cap; s++) counts[reason[s]]++;
      std::printf("mode %d gate %.0f: status %d, kept %d short %d degenerate %d behind %d reprojection %d\n", mode, gate,
                  status[0], counts[0], counts[1], counts[2], counts[3], counts[4]);
      if (po[1] != counts[0]) return 1;
      kept_total += po[1];
    }
  return kept_total > 0 ? 0 : 1;
}
#endif
