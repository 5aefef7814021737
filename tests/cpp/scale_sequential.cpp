// Test infrastructure: a plain sequential restatement of the scale step (get_scale: triangulatePoints + the
// median of distance ratios, DESIGN.md §9 rank 6 rules 1-4), in the reference's loop order
// (src/feature_matching.cpp:208-275; the join of src/feature_tracking_scale.py:127-164): one loop over the
// points, std::map for the join of two match lists, std::nth_element for the median.  Only the per-point
// arithmetic comes from orbx_tri_math.h; the orchestration below is written independently of the kernels, so
// the GPU test that compares the two checks the kernels' compaction, LDS join and selection.
//
// Built by tests/test_scale.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_tri_math.h"

namespace {
struct P3 {
  float v[3];
  bool ok;
};

// the tail of get_scale (src/feature_matching.cpp:248-274) on two index-aligned lists
double scale_of(const std::vector<P3>& prev, const std::vector<P3>& cur, int* used) {
  *used = 0;
  if (prev.empty() || cur.empty()) return 1.0;
  const size_t min_idx = std::min(prev.size(), cur.size());
  std::vector<double> ratios;
  for (size_t i = 1; i < min_idx; ++i) {
    if (!(prev[i].ok && prev[i - 1].ok && cur[i].ok && cur[i - 1].ok)) continue;
    const double ratio = tri_ratio(prev[i].v, prev[i - 1].v, cur[i].v, cur[i - 1].v);
    if (tri_ratio_ok(ratio)) ratios.push_back(ratio);
  }
  *used = (int)ratios.size();
  if (ratios.empty()) return 1.0;
  std::nth_element(ratios.begin(), ratios.begin() + ratios.size() / 2, ratios.end());
  return tri_scale_clamp(ratios[ratios.size() / 2]);
}

std::vector<P3> list_of(const float* xyz, const uint8_t* valid, int n) {
  std::vector<P3> v((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) v[(size_t)i].v[k] = xyz[3 * i + k];
    v[(size_t)i].ok = valid ? valid[i] != 0 : true;
  }
  return v;
}
}  // namespace

extern "C" {

// rule 1 alone: the homogeneous points (4 n doubles), for the comparison against an SVD
void seq_triangulate_homogeneous(const float* pts1_xy, const float* pts2_xy, int n, const double* K, const double* R,
                                 const double* t, double* h) {
  double P1[12], P2[12];
  tri_projections(K, R, t, P1, P2);
  for (int i = 0; i < n; i++)
    tri_homogeneous(P1, P2, (double)pts1_xy[2 * i], (double)pts1_xy[2 * i + 1], (double)pts2_xy[2 * i],
                    (double)pts2_xy[2 * i + 1], h + 4 * i);
}

// rules 1-2 over n correspondences (pixels, float (x, y) pairs)
void seq_triangulate(const float* pts1_xy, const float* pts2_xy, int n, const double* K, const double* R,
                     const double* t, float* xyz, uint8_t* valid) {
  double P1[12], P2[12];
  tri_projections(K, R, t, P1, P2);
  for (int i = 0; i < n; i++)
    valid[i] = tri_point(P1, P2, (double)pts1_xy[2 * i], (double)pts1_xy[2 * i + 1], (double)pts2_xy[2 * i],
                         (double)pts2_xy[2 * i + 1], xyz + 3 * i)
                   ? 1
                   : 0;
}

// rule 3; the valid arrays may be NULL (all valid)
double seq_estimate_scale(const float* prev_xyz, const uint8_t* prev_valid, int n_prev, const float* cur_xyz,
                          const uint8_t* cur_valid, int n_cur, int* ratios_used) {
  return scale_of(list_of(prev_xyz, prev_valid, n_prev), list_of(cur_xyz, cur_valid, n_cur), ratios_used);
}

// rule 4: matches (., t12[i]) of frames 1 -> 2, in query order, with their points xyz12 (frame-1 coordinates) and the pose
// (R12, t12v); matches (q23[j], t23[j]) of frames 2 -> 3 with their points xyz23.  trip_i / trip_j (optional,
// capacity n23) receive the joined positions in ascending frame-2 index order.
double seq_join_scale(const int32_t* t12, int n12, const float* xyz12, const uint8_t* valid12,
                      const double* R12, const double* t12v, const int32_t* q23, int n23, const float* xyz23,
                      const uint8_t* valid23, int32_t* trip_i, int32_t* trip_j, int* triplets, int* ratios_used) {
  std::map<int32_t, int> to12;  // frame-2 keypoint index -> position in the 1 -> 2 list: the last write wins
  for (int i = 0; i < n12; i++) to12[t12[i]] = i;
  std::map<int32_t, int> to23;  // frame-2 keypoint index -> position in the 2 -> 3 list (query indices are unique)
  for (int j = 0; j < n23; j++) to23[q23[j]] = j;
  std::vector<P3> prev, cur;
  int nt = 0;
  for (const auto& kv : to23) {  // ascending frame-2 index
    const auto it = to12.find(kv.first);
    if (it == to12.end()) continue;
    const int i = it->second, j = kv.second;
    P3 a, b;
    tri_transform(R12, t12v, xyz12 + 3 * i, a.v);
    a.ok = valid12 ? valid12[i] != 0 : true;
    for (int k = 0; k < 3; k++) b.v[k] = xyz23[3 * j + k];
    b.ok = valid23 ? valid23[j] != 0 : true;
    prev.push_back(a);
    cur.push_back(b);
    if (trip_i) trip_i[nt] = i;
    if (trip_j) trip_j[nt] = j;
    nt++;
  }
  *triplets = nt;
  return scale_of(prev, cur, ratios_used);
}

}  // extern "C"
