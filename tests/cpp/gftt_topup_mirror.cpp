// gftt_topup_mirror.cpp -- driver of the C++ mirror of the masked cv::goodFeaturesToTrack and of the top-up of tracked
// points (host/orb.hpp), compiled and run by tests/test_cpp_gftt_topup.py.
//   gftt_topup_mirror mask <blob>:   width, height (int32), the pixels, the mask bytes (width x height), maxCorners
//                                    (int32), qualityLevel, minDistance (double).  Runs the mask overload of
//                                    orbx::goodFeaturesToTrack twice on one handle (the second call must ASSIGN) and
//                                    prints every corner.
//   gftt_topup_mirror topup <blob>:  width, height (int32), the pixels, the number of tracked points (int32), their
//                                    (x, y) floats, maxCorners (int32), qualityLevel, minDistance (double).  Runs
//                                    orbx::top_up_keypoints and prints `carried`, then every point with its origin.
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
  orbx::Image plane(int w, int h) {
    if (pos + (size_t)w * h > buf.size()) throw std::runtime_error("blob too short");
    orbx::Image img(reinterpret_cast<const uint8_t*>(buf.data() + pos), w, h, w);
    pos += (size_t)w * h;
    return img;
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  try {
    Reader in(argv[2]);
    orbx::CornerDetector det;
    const int w = in.get<int32_t>(), h = in.get<int32_t>();
    const orbx::Image img = in.plane(w, h);
    if (std::string(argv[1]) == "mask") {
      const orbx::Image mask = in.plane(w, h);
      const int max_corners = in.get<int32_t>();
      const double quality = in.get<double>(), distance = in.get<double>();
      std::vector<orbx::Point2f> corners(7);  // stale content: the call assigns
      orbx::goodFeaturesToTrack(det, img, corners, max_corners, quality, distance, mask);
      const std::vector<orbx::Point2f> first = corners;
      orbx::goodFeaturesToTrack(det, img, corners, max_corners, quality, distance, mask);
      if (first.size() != corners.size() ||
          std::memcmp(first.data(), corners.data(), sizeof(orbx::Point2f) * first.size()))
        throw std::runtime_error("two calls differ");
      for (const auto& p : corners) std::printf("%a %a\n", (double)p.x, (double)p.y);
      return 0;
    }
    if (std::string(argv[1]) == "topup") {
      std::vector<orbx::Point2f> tracked((size_t)in.get<int32_t>());
      for (auto& p : tracked) p.x = in.get<float>(), p.y = in.get<float>();
      const int max_corners = in.get<int32_t>();
      const double quality = in.get<double>(), distance = in.get<double>();
      const orbx::ToppedUp out = orbx::top_up_keypoints(det, img, tracked, max_corners, quality, distance);
      if (out.points.size() != out.origin.size()) throw std::runtime_error("points and origin differ in length");
      std::printf("%d\n", out.carried);
      for (size_t i = 0; i < out.points.size(); i++)
        std::printf("%a %a %d\n", (double)out.points[i].x, (double)out.points[i].y, (int)out.origin[i]);
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "gftt_topup_mirror: %s\n", e.what());
    return 1;
  }
  return 2;
}
