// wp_mirror.cpp -- driver of orbx::run_window_odometry_on_tracks and orbx::detail::ba_write_back (host/orb.hpp;
// DESIGN.md §9 rank 14), compiled and run by tests/test_cpp_window_poses.py and tests/test_window_poses.py.
//   wp_mirror window <blob>:  K (9 doubles), the first camera -> world pose (16 doubles), scale0 (double), W (int32),
//                             the number of tracks n (int32), their points (n x W x 2 floats) and `seen` (n int32).
//                             Prints the outcome and the gated poses, every double as a hex float.
//   wp_mirror gate <blob>:    n (int32) windows of W (int32) poses: the blocks after the solve and the blocks before
//                             (n x W x 6 doubles each).  Prints what ba_write_back decides for every pose, as if
//                             every window had converged (the caller knows which did).  Needs no GPU.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

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

int window(Reader& in) {
  double K[9];
  for (double& v : K) v = in.get<double>();
  orbx::Pose4x4 pose0;
  for (double& v : pose0) v = in.get<double>();
  const double scale0 = in.get<double>();
  const int W = in.get<int32_t>(), n = in.get<int32_t>();
  std::vector<orbx::Point2f> xy((size_t)n * W);
  for (auto& p : xy) p.x = in.get<float>(), p.y = in.get<float>();
  std::vector<int32_t> seen((size_t)n);
  for (auto& s : seen) s = in.get<int32_t>();
  const orbx::WindowOdometry r = orbx::run_window_odometry_on_tracks(pose0, K, xy, seen, W, scale0);
  std::printf("ran wp_status %d lm_status %d termination %d iterations %d steps %d initial %a final %a\n", r.wp_status,
              r.lm_status, r.summary.termination, r.summary.iterations, r.summary.successful_steps,
              r.summary.initial_cost, r.summary.final_cost);
  for (int i = 0; i < W; i++) {
    std::printf("pose %d updated %d", i, (int)r.updated[(size_t)i]);
    for (double v : r.pose_window[(size_t)i]) std::printf(" %a", v);
    std::printf("\n");
  }
  return 0;
}

int gate(Reader& in) {
  const int n = in.get<int32_t>(), W = in.get<int32_t>();
  std::vector<double> solved((size_t)n * W * 6), old(solved.size());
  for (double& v : solved) v = in.get<double>();
  for (double& v : old) v = in.get<double>();
  for (int w = 0; w < n; w++) {
    std::vector<orbx::Pose4x4> pose_window((size_t)W);
    std::vector<uint8_t> updated((size_t)W, 0);
    const std::vector<double> a(solved.begin() + (size_t)w * W * 6, solved.begin() + (size_t)(w + 1) * W * 6);
    const std::vector<double> b(old.begin() + (size_t)w * W * 6, old.begin() + (size_t)(w + 1) * W * 6);
    orbx::detail::ba_write_back(pose_window, a, b, &updated);
    std::printf("window %d", w);
    for (uint8_t u : updated) std::printf(" %d", (int)u);
    std::printf("\n");
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  try {
    Reader in(argv[2]);
    return std::string(argv[1]) == "gate" ? gate(in) : window(in);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "wp_mirror: %s\n", e.what());
    return 1;
  }
}
