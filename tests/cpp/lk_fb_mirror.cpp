// lk_fb_mirror.cpp -- driver of the C++ mirror of trackPointsAcrossWindow with the forward-backward check
// (host/orb.hpp), compiled and run by tests/test_cpp_lk_fb.py.
//   lk_fb_mirror <mode> <blob> <threshold>:  the blob of lk_window_mirror.cpp -- frames, width, height (int32), the
//                                            pixels of every frame, the number of points (int32), their (x, y) floats
//   mode "pairs":  orbx::track_points_across_window_fb (two orbx_lk_track calls per pair, survivors compacted on the
//                  host, the distance rule on the host)
//   mode "launch": orbx::track_points_across_window_fb_one_launch (one tracking launch for the window)
// Prints one line per track: its length, why it ended, then "frame x y" for every observation, the floats in hex.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

#include "orb.hpp"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  try {
    std::ifstream f(argv[2], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    auto take = [&](void* dst, size_t bytes) {
      if (pos + bytes > buf.size()) throw std::runtime_error("blob too short");
      if (dst) std::memcpy(dst, buf.data() + pos, bytes);
      pos += bytes;
    };
    int32_t dims[3];
    take(dims, sizeof(dims));
    const int n_frames = dims[0], w = dims[1], h = dims[2];
    std::vector<orbx::Image> imgs;
    for (int i = 0; i < n_frames; i++) {
      imgs.emplace_back(reinterpret_cast<const uint8_t*>(buf.data() + pos), w, h, w);
      take(nullptr, (size_t)w * h);
    }
    int32_t n = 0;
    take(&n, sizeof(n));
    std::vector<orbx::Point2f> pts((size_t)n);
    take(pts.data(), sizeof(orbx::Point2f) * pts.size());
    const float thr = std::strtof(argv[3], nullptr);
    orbx::LKTracker lk;
    const std::string mode = argv[1];
    std::vector<orbx::Track> tracks;
    std::vector<int32_t> lost;
    if (mode == "pairs")
      tracks = orbx::track_points_across_window_fb(lk, imgs, pts, thr, &lost);
    else if (mode == "launch")
      tracks = orbx::track_points_across_window_fb_one_launch(lk, imgs, pts, thr, &lost);
    else
      return 2;
    for (size_t i = 0; i < tracks.size(); i++) {
      std::printf("%zu %d", tracks[i].size(), (int)lost[i]);
      for (const auto& o : tracks[i]) std::printf(" %d %a %a", o.first, (double)o.second.x, (double)o.second.y);
      std::printf("\n");
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "lk_fb_mirror: %s\n", e.what());
    return 1;
  }
}
