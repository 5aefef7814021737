// reloc_mirror.cpp -- driver of orbx::Feature2D::compute, orbx::describe_points and orbx::reassociate (host/orb.hpp;
// DESIGN.md §9 rank 19), compiled and run by tests/test_cpp_reloc.py.
//   reloc_mirror pins    prints the layout of the two views of include/orbx_reloc.h (no GPU needed)
//   reloc_mirror <blob>  width, height, n (int32 each), the image (width x height bytes) and n points (two floats each).
// Prints one `compute` line per keypoint that Feature2D::compute kept (its index before the call, the angle in degrees
// as a hex float, the 32 descriptor bytes), one `describe` line per point of orbx::describe_points (state, the angle in
// radians as a hex float, the bytes) and the re-association of that set with itself.
#include <cstddef>
#include <cstdio>
#include <fstream>
#include <iterator>

#include "orb.hpp"

static_assert(offsetof(orbx_point_descriptors_view, desc) == 0 && offsetof(orbx_point_descriptors_view, angle) == 8 &&
                  offsetof(orbx_point_descriptors_view, state) == 16 && offsetof(orbx_point_descriptors_view, n_ok) == 24 &&
                  offsetof(orbx_point_descriptors_view, slot_capacity) == 32 &&
                  offsetof(orbx_point_descriptors_view, n) == 36 && sizeof(orbx_point_descriptors_view) == 40,
              "orbx_point_descriptors_view");
static_assert(offsetof(orbx_reassociate_view, origin) == 0 && offsetof(orbx_reassociate_view, dist) == 8 &&
                  offsetof(orbx_reassociate_view, count) == 16 && offsetof(orbx_reassociate_view, q_capacity) == 24 &&
                  offsetof(orbx_reassociate_view, t_capacity) == 28 && offsetof(orbx_reassociate_view, n_windows) == 32 &&
                  sizeof(orbx_reassociate_view) == 40,
              "orbx_reassociate_view");
static_assert(ORBX_PD_NONE == 0 && ORBX_PD_BORDER == 1 && ORBX_PD_OK == 2 && ORBX_PD_BANKS == 2, "orbx_pd_state");

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
void print_bytes(const ORBDescriptor& d) {
  std::printf(" ");
  for (uint8_t b : d.data) std::printf("%02x", b);
  std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (std::string(argv[1]) == "pins") {
    std::printf("orbx_point_descriptors_view %zu %zu %zu\n", sizeof(orbx_point_descriptors_view),
                offsetof(orbx_point_descriptors_view, slot_capacity), offsetof(orbx_point_descriptors_view, n));
    std::printf("orbx_reassociate_view %zu %zu %zu %zu\n", sizeof(orbx_reassociate_view),
                offsetof(orbx_reassociate_view, q_capacity), offsetof(orbx_reassociate_view, t_capacity),
                offsetof(orbx_reassociate_view, n_windows));
    return 0;
  }
  try {
    Reader in(argv[1]);
    const int w = in.get<int32_t>(), h = in.get<int32_t>(), n = in.get<int32_t>();
    std::vector<uint8_t> pixels((size_t)w * h);
    for (auto& v : pixels) v = in.get<uint8_t>();
    std::vector<orbx::Point2f> pts((size_t)n);
    for (auto& p : pts) p.x = in.get<float>(), p.y = in.get<float>();
    const orbx::Image image(pixels.data(), w, h);
    std::vector<orbx::KeyPoint> kps((size_t)n);
    for (int i = 0; i < n; i++) {
      kps[(size_t)i].pt = pts[(size_t)i];
      kps[(size_t)i].octave = i % 3;  // ignored: everything is described at level 0
      kps[(size_t)i].class_id = i;
    }
    auto orb = orbx::Feature2D::create(500, 1.2f, 4);
    orbx::DescriptorMat des;
    orb->compute(image, kps, des);
    if (des.rows != (int)kps.size() || des.d.size() != kps.size()) throw std::runtime_error("rows differ from keypoints");
    for (size_t i = 0; i < kps.size(); i++) {
      std::printf("compute %d %a %d", kps[i].class_id, kps[i].angle, kps[i].octave);
      print_bytes(des.d[i]);
    }
    const orbx::PointDescriptors pd = orbx::describe_points(image, pts);
    for (int i = 0; i < n; i++) {
      std::printf("describe %d %a", pd.state[(size_t)i], pd.angle[(size_t)i]);
      print_bytes(pd.desc[(size_t)i]);
    }
    const orbx::Reassociation r = orbx::reassociate(pd, pd, 0.8, 256, true);
    std::printf("origin %d", r.count);
    for (int32_t v : r.origin) std::printf(" %d", v);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  return 0;
}
