// st_mirror.cpp -- driver of orbx::run_stream_odometry_on_tracks and orbx::stitch_windows (host/orb.hpp; DESIGN.md §9
// rank 16), compiled and run by tests/test_cpp_stitch.py.
//   st_mirror stream <blob>:  K (9 doubles), the pose of stream frame 0 (16 doubles), scale0 (double), the numbers of
//                             windows, frames per window, stride, tracks per window and align_scale (int32 each), the
//                             points (windows x tracks x frames x 2 floats) and `seen` (windows x tracks int32).
//                             Prints the statuses per window and the trajectory, every double as a hex float.
//   st_mirror stitch <blob>:  the pose of stream frame 0, the numbers of windows, frames per window, stride and
//                             align_scale, the window poses (windows x frames x 16 doubles).  Prints the same for
//                             orbx::stitch_windows.  Needs no GPU.
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

void print_trajectory(const std::vector<orbx::Pose4x4>& trajectory) {
  for (size_t f = 0; f < trajectory.size(); f++) {
    std::printf("frame %zu", f);
    for (double v : trajectory[f]) std::printf(" %a", v);
    std::printf("\n");
  }
}

int stream(Reader& in) {
  double K[9];
  for (double& v : K) v = in.get<double>();
  orbx::Pose4x4 pose0;
  for (double& v : pose0) v = in.get<double>();
  const double scale0 = in.get<double>();
  const int W = in.get<int32_t>(), L = in.get<int32_t>(), stride = in.get<int32_t>(), n = in.get<int32_t>();
  const bool align = in.get<int32_t>() != 0;
  std::vector<orbx::Point2f> xy((size_t)W * n * L);
  for (auto& p : xy) p.x = in.get<float>(), p.y = in.get<float>();
  std::vector<int32_t> seen((size_t)W * n);
  for (auto& s : seen) s = in.get<int32_t>();
  const orbx::StreamOdometry r =
      orbx::run_stream_odometry_on_tracks(pose0, K, xy, seen, W, L, stride, scale0, orbx::LandmarkOptions(), align);
  for (int w = 0; w < W; w++) {
    const orbx_ba_summary& s = r.summaries[(size_t)w];
    std::printf("window %d st_status %d wp_status %d lm_status %d termination %d iterations %d steps %d initial %a final %a\n",
                w, r.st_status[(size_t)w], r.wp_status[(size_t)w], r.lm_status[(size_t)w], s.termination, s.iterations,
                s.successful_steps, s.initial_cost, s.final_cost);
  }
  print_trajectory(r.trajectory);
  return 0;
}

int stitch(Reader& in) {
  orbx::Pose4x4 pose0;
  for (double& v : pose0) v = in.get<double>();
  const int W = in.get<int32_t>(), L = in.get<int32_t>(), stride = in.get<int32_t>();
  const bool align = in.get<int32_t>() != 0;
  std::vector<orbx::Pose4x4> poses((size_t)W * L);
  for (auto& p : poses)
    for (double& v : p) v = in.get<double>();
  const orbx::StitchedStream r = orbx::stitch_windows(poses, W, L, stride, pose0, align);
  for (int w = 0; w < W; w++) std::printf("window %d st_status %d lambda %a\n", w, r.status[(size_t)w], r.lambda[(size_t)w]);
  print_trajectory(r.trajectory);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  try {
    Reader in(argv[2]);
    return std::string(argv[1]) == "stitch" ? stitch(in) : stream(in);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "st_mirror: %s\n", e.what());
    return 1;
  }
}
