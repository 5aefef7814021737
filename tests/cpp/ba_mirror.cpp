// ba_mirror.cpp -- driver of the C++ mirror of src/with_bundle_adjustment.cpp's host glue (host/orb.hpp), compiled
// and run by tests/test_ba.py.
//   ba_mirror ba <blob>:  K (9 doubles), W (int32), W camera -> world poses (16 doubles each), the number of tracks
//                         (int32), then per track its length (int32) and (frame int32, x float, y float) entries.
//                         Runs build_landmarks + run_bundle_adjustment and prints the outcome.
//   ba_mirror lk <blob>:  frames, width, height (int32), the frames' pixels, the number of points (int32), their
//                         (x, y) floats.  Runs track_points_across_window and prints every track.
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
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  try {
    Reader in(argv[2]);
    if (std::string(argv[1]) == "ba") {
      double K[9];
      for (double& v : K) v = in.get<double>();
      const int W = in.get<int32_t>();
      std::vector<orbx::Pose4x4> poses((size_t)W);
      for (auto& T : poses)
        for (double& v : T) v = in.get<double>();
      std::vector<orbx::Track> tracks((size_t)in.get<int32_t>());
      for (auto& tr : tracks) {
        const int len = in.get<int32_t>();
        for (int k = 0; k < len; k++) {
          const int frame = in.get<int32_t>();
          orbx::Point2f p;
          p.x = in.get<float>(), p.y = in.get<float>();
          tr.emplace_back(frame, p);
        }
      }
      std::vector<orbx::Landmark> landmarks;
      const bool built = orbx::build_landmarks(poses, K, tracks, landmarks);
      orbx_ba_summary s{};
      std::vector<uint8_t> updated;
      const bool ran = built && orbx::run_bundle_adjustment(poses, K, landmarks, &s, &updated);
      std::printf("built %d landmarks %zu ran %d termination %d iterations %d initial %a final %a\n", built ? 1 : 0,
                  landmarks.size(), ran ? 1 : 0, s.termination, s.iterations, s.initial_cost, s.final_cost);
      for (int i = 0; i < W; i++) {
        std::printf("pose %d updated %d", i, ran ? (int)updated[(size_t)i] : 0);
        for (double v : poses[(size_t)i]) std::printf(" %a", v);
        std::printf("\n");
      }
      return 0;
    }
    if (std::string(argv[1]) == "lk") {
      const int n = in.get<int32_t>(), w = in.get<int32_t>(), h = in.get<int32_t>();
      std::vector<orbx::Image> imgs;
      for (int i = 0; i < n; i++) {
        imgs.emplace_back(reinterpret_cast<const uint8_t*>(in.buf.data() + in.pos), w, h, w);
        in.pos += (size_t)w * h;
      }
      std::vector<orbx::Point2f> pts((size_t)in.get<int32_t>());
      for (auto& p : pts) p.x = in.get<float>(), p.y = in.get<float>();
      orbx::LKTracker lk;
      const auto tracks = orbx::track_points_across_window(lk, imgs, pts);
      for (size_t i = 0; i < tracks.size(); i++)
        for (const auto& obs : tracks[i]) std::printf("%zu %d %a %a\n", i, obs.first, (double)obs.second.x, (double)obs.second.y);
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ba_mirror: %s\n", e.what());
    return 1;
  }
  return 2;
}
