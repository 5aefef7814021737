// lm_views_mirror.cpp -- driver of the overload of orbx::run_bundle_adjustment_on_tracks that takes
// orbx::LandmarkOptions (host/orb.hpp), compiled and run by tests/test_cpp_landmarks_views.py.
//   lm_views_mirror <blob> <tri_mode> <max_reproj_px>:  the blob of tests/cpp/lm_mirror.cpp -- K (9 doubles), W (int32), W camera -> world poses (16 doubles each), the number of tracks n
//                      (int32), their points (n x W x 2 floats) and `seen` (n int32): what LKTracker::trackWindow
//                      returns.  Prints the world -> camera blocks handed to the library, the outcome, the poses
//                      after the write-back gate and the refined landmarks, every double as a hex float.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "orb.hpp"

namespace {
struct Reader {
  std::vector<char> buf;
  size_t pos = 0;
  explicit Reader(const char* path) {
    std::ifstream f(path, std::ios::binary);
    buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  }
  template <class T>
  T get() {
    T v;
    if (pos + sizeof(T) > buf.size()) throw std::runtime_error("blob too short");
    std::memcpy(&v, buf.data() + pos, sizeof(T));
    pos += sizeof(T);
    return v;
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  try {
    Reader in(argv[1]);
    double K[9];
    for (double& v : K) v = in.get<double>();
    const int W = in.get<int32_t>();
    std::vector<orbx::Pose4x4> poses((size_t)W);
    for (auto& T : poses)
      for (double& v : T) v = in.get<double>();
    const int n = in.get<int32_t>();
    std::vector<orbx::Point2f> xy((size_t)n * W);
    for (auto& p : xy) p.x = in.get<float>(), p.y = in.get<float>();
    std::vector<int32_t> seen((size_t)n);
    for (auto& s : seen) s = in.get<int32_t>();
    for (int i = 0; i < W; i++) {  // the blocks the mirror hands over (the same two calls, the same bits)
      double R[9], b[6];
      orbx::detail::invert_rigid(poses[(size_t)i], R, b + 3);
      orbx::detail::rodrigues_inv(R, b);
      std::printf("block %d", i);
      for (double v : b) std::printf(" %a", v);
      std::printf("\n");
    }
    orbx_ba_summary s{};
    std::vector<uint8_t> updated;
    int32_t status = -1;
    std::vector<orbx::Point3d> points;
    std::vector<int32_t> slots;
    orbx::LandmarkOptions options;
    options.tri_mode = std::atoi(argv[2]);
    options.max_reproj_px = std::atof(argv[3]);
    const bool ran =
        orbx::run_bundle_adjustment_on_tracks(poses, K, xy, seen, options, &s, &updated, &status, &points, &slots);
    std::printf("ran %d status %d landmarks %zu termination %d iterations %d steps %d initial %a final %a\n", ran ? 1 : 0,
                status, points.size(), s.termination, s.iterations, s.successful_steps, s.initial_cost, s.final_cost);
    for (int i = 0; i < W; i++) {
      std::printf("pose %d updated %d", i, (int)updated[(size_t)i]);
      for (double v : poses[(size_t)i]) std::printf(" %a", v);
      std::printf("\n");
    }
    for (size_t j = 0; j < points.size(); j++)
      std::printf("point %d %a %a %a\n", slots[j], points[j].x, points[j].y, points[j].z);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "lm_views_mirror: %s\n", e.what());
    return 1;
  }
}
