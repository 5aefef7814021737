// carry_mirror.cpp -- driver of orbx::localise_carried_window (host/orb.hpp), compiled and run by
// tests/test_cpp_carry.py.
//   carry_mirror <blob>:  K (9 doubles), n_old, n_slots, n_frames, iterationsCount, refine_iters and min_inliers (int32
//                         each), the seed (uint64), reprojectionError and confidence (double each), the old points
//                         (n_old x 3 doubles), old_slot_of_point (n_old int32), origin (n_slots int32), the tracks
//                         (n_slots x n_frames x 2 floats) and seen (n_slots int32).
// Prints the window's status, one line per record (every double as a hex float), the poses and the carried points.
#include <cstdio>
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
  if (argc != 2) return 2;
  try {
    Reader in(argv[1]);
    double K[9];
    for (double& v : K) v = in.get<double>();
    const int n_old = in.get<int32_t>(), n_slots = in.get<int32_t>(), n_frames = in.get<int32_t>();
    const int iterations = in.get<int32_t>(), refine = in.get<int32_t>(), min_inliers = in.get<int32_t>();
    const uint64_t seed = in.get<uint64_t>();
    const double error = in.get<double>(), confidence = in.get<double>();
    std::vector<orbx::Point3d> pts((size_t)n_old);
    for (auto& p : pts) p.x = in.get<double>(), p.y = in.get<double>(), p.z = in.get<double>();
    std::vector<int32_t> slot_of_point((size_t)n_old), origin((size_t)n_slots), seen((size_t)n_slots);
    for (auto& v : slot_of_point) v = in.get<int32_t>();
    for (auto& v : origin) v = in.get<int32_t>();
    std::vector<orbx::Point2f> tracks((size_t)n_slots * n_frames);
    for (auto& p : tracks) p.x = in.get<float>(), p.y = in.get<float>();
    for (auto& v : seen) v = in.get<int32_t>();
    const orbx::CarriedWindow w = orbx::localise_carried_window(pts, slot_of_point, origin, tracks, seen, n_frames, K,
                                                                iterations, error, confidence, seed, refine, min_inliers);
    std::printf("status %d ok %d\n", w.status, w.ok() ? 1 : 0);
    for (const orbx_pnp_record& r : w.records)
      std::printf("record %d %d %d %d %a %a %a %a %a %a %a\n", r.status, r.inliers, r.iters, r.n_corr, r.rms_px,
                  r.pose6[0], r.pose6[1], r.pose6[2], r.pose6[3], r.pose6[4], r.pose6[5]);
    std::printf("poses");
    for (double v : w.poses6) std::printf(" %a", v);
    std::printf("\npoints");
    for (int32_t v : w.carried_point) std::printf(" %d", v);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  return 0;
}
