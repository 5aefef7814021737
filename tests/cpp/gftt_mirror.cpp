// gftt_mirror.cpp -- driver of the C++ mirror of cv::goodFeaturesToTrack and of the initial-keypoint branch of
// src/with_bundle_adjustment.cpp:586-593 (host/orb.hpp), compiled and run by tests/test_cpp_gftt.py.
//   gftt_mirror gftt <blob>:  width, height (int32), the pixels, maxCorners (int32), qualityLevel, minDistance
//                             (double).  Runs orbx::goodFeaturesToTrack twice on one handle (the second call must
//                             ASSIGN, not append) and prints every corner.
//   gftt_mirror init <blob>:  width, height (int32), the pixels, the number of observations of frame 0 (int32),
//                             their (x, y) doubles.  Runs orbx::initial_keypoints and prints every keypoint.
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
  orbx::Image image() {
    const int w = get<int32_t>(), h = get<int32_t>();
    if (pos + (size_t)w * h > buf.size()) throw std::runtime_error("blob too short");
    orbx::Image img(reinterpret_cast<const uint8_t*>(buf.data() + pos), w, h, w);
    pos += (size_t)w * h;
    return img;
  }
};
void print(const std::vector<orbx::Point2f>& pts) {
  for (const auto& p : pts) std::printf("%a %a\n", (double)p.x, (double)p.y);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  try {
    Reader in(argv[2]);
    orbx::CornerDetector det;
    const orbx::Image img = in.image();
    if (std::string(argv[1]) == "gftt") {
      const int max_corners = in.get<int32_t>();
      const double quality = in.get<double>(), distance = in.get<double>();
      std::vector<orbx::Point2f> corners(7);  // stale content: the call assigns
      orbx::goodFeaturesToTrack(det, img, corners, max_corners, quality, distance);
      const std::vector<orbx::Point2f> first = corners;
      orbx::goodFeaturesToTrack(det, img, corners, max_corners, quality, distance);
      if (first.size() != corners.size() ||
          std::memcmp(first.data(), corners.data(), sizeof(orbx::Point2f) * first.size()))
        throw std::runtime_error("two calls differ");
      print(corners);
      return 0;
    }
    if (std::string(argv[1]) == "init") {
      std::vector<orbx::Point2d> obs((size_t)in.get<int32_t>());
      for (auto& p : obs) p.x = in.get<double>(), p.y = in.get<double>();
      print(orbx::initial_keypoints(det, obs, img));
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "gftt_mirror: %s\n", e.what());
    return 1;
  }
  return 2;
}
