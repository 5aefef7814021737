// search_sequential.cpp -- sequential restatement of the landmarks projected into a predicted view (DESIGN.md §9
// rank 21 rules P1-P5; csrc/orbx_search.hip), the reference of tests/test_cpp_search.py and tests/test_search.py.  One
// window after the other, one landmark after the other.  It shares the arithmetic (the pose's model, the three sums,
// the two quotients and the bounds) with the kernel through orbx_search_math.h; the join of landmarks to slots, the
// loops, the zeros and the count are written here on their own.
//
// The rules, restated:
//   P1  old slot t has a landmark iff the window is OK, a landmark j has slot_of_point == t (the first one, in a block
//       whose slots ascend) and its three source doubles are finite; otherwise NONE
//   P2  a pose that sp_pose_model does not accept leaves the whole window NONE, count 0
//   P3-P5  sp_project: BEHIND iff !(p2 > 0); OK iff u, v finite and inside [-margin, size - 1 + margin]; else OUTSIDE;
//       a slot that is not OK holds zeros; count = the OK slots
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC search_sequential.cpp
#include <cstdint>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_lm_math.h"
#include "../../visual-odometry-gpu_amd/csrc/orbx_search_math.h"

extern "C" {

// K9: row-major 3x3; poses6: pose_stride doubles per window; status / pt_off / slot_of_point / points3: the block as
// Context.landmarks_fetch returns it; xy (n x cap x 2), depth, state (n x cap), count (n)
void seq_sp_project(const double* K9, int n_windows, int cap, const double* poses6, int pose_stride,
                    const int32_t* status, const int32_t* pt_off, const int32_t* slot_of_point, const double* points3,
                    int width, int height, double margin_px, double* xy, double* depth, int32_t* state,
                    int32_t* count) {
  const double K4[4] = {K9[0], K9[4], K9[2], K9[5]};
  for (int w = 0; w < n_windows; w++) {
    double* XY = xy + 2 * (size_t)w * cap;
    double* Z = depth + (size_t)w * cap;
    int32_t* S = state + (size_t)w * cap;
    for (int s = 0; s < cap; s++) XY[2 * s] = 0.0, XY[2 * s + 1] = 0.0, Z[s] = 0.0, S[s] = SP_NONE;
    count[w] = 0;
    if (status[w] != LM_OK) continue;
    double M[PNP_MODEL_DOUBLES];
    if (!sp_pose_model(poses6 + (size_t)w * pose_stride, M)) continue;
    std::vector<char> taken(cap, 0);
    int ok = 0;
    for (int j = pt_off[w]; j < pt_off[w + 1]; j++) {
      const int s = slot_of_point[j];
      if (s < 0 || s >= cap || taken[s]) continue;
      taken[s] = 1;
      const double* X = points3 + 3 * (size_t)j;
      if (!(wp_finite(X[0]) && wp_finite(X[1]) && wp_finite(X[2]))) continue;
      double out[3];
      S[s] = sp_project(K4, M, X, width, height, margin_px, out);
      if (S[s] == SP_OK) XY[2 * s] = out[0], XY[2 * s + 1] = out[1], Z[s] = out[2], ok++;
    }
    count[w] = ok;
  }
}

// rule L for one pair, as the kernel and the host evaluate it
int seq_sp_in_gate(float qx, float qy, double tx, double ty, double radius_px) {
  return sp_in_gate(qx, qy, tx, ty, radius_px * radius_px) ? 1 : 0;
}

}  // extern "C"
