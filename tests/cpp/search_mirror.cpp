// search_mirror.cpp -- the C++ mirror of the search by projection (host/orb.hpp: orbx::project_landmarks and
// orbx::reassociate_gated) on the arrays tests/test_cpp_search.py writes: the projection of one
// old window and the gated re-association of one window, every double printed as a hex float.
//   search_mirror.bin <file>
//   file: int32 n_old, cap, width, height, nq, nt, max_distance, accept_lone, unique | double margin, radius, ratio |
//         K (9) | pose6 (6) | points3 (n_old x 3) | slot_of_point (n_old) | qdesc (nq x 32) | qstate (nq) | qxy (nq x 2
//         floats) | tdesc (nt x 32) | tstate (nt) | txy (nt x 2 doubles) | tpstate (nt)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "orb.hpp"

namespace {

struct Reader {
  std::vector<char> bytes;
  size_t at = 0;
  template <class T>
  std::vector<T> take(size_t n) {
    std::vector<T> out(n);
    if (at + n * sizeof(T) > bytes.size()) throw std::runtime_error("the file is too short");
    if (n) std::memcpy(out.data(), bytes.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return out;
  }
};

template <class T>
void print_ints(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (const T& x : v) std::printf(" %d", (int)x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  using namespace orbx;
  if (argc != 2) return 2;
  try {
    std::ifstream f(argv[1], std::ios::binary);
    Reader r;
    r.bytes.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    const std::vector<int32_t> n = r.take<int32_t>(9);
    const std::vector<double> d = r.take<double>(3), K = r.take<double>(9), pose6 = r.take<double>(6);
    const std::vector<Point3d> pts = r.take<Point3d>((size_t)n[0]);
    const std::vector<int32_t> slot = r.take<int32_t>((size_t)n[0]);
    const std::vector<ORBDescriptor> qdesc = r.take<ORBDescriptor>((size_t)n[4]);
    const std::vector<int32_t> qstate = r.take<int32_t>((size_t)n[4]);
    const std::vector<Point2f> qxy = r.take<Point2f>((size_t)n[4]);
    const std::vector<ORBDescriptor> tdesc = r.take<ORBDescriptor>((size_t)n[5]);
    const std::vector<int32_t> tstate = r.take<int32_t>((size_t)n[5]);
    const std::vector<Point2d> txy = r.take<Point2d>((size_t)n[5]);
    const std::vector<int32_t> tpstate = r.take<int32_t>((size_t)n[5]);

    const ProjectedLandmarks p = project_landmarks(pts, slot, n[1], K.data(), pose6.data(), n[2], n[3], d[0]);
    std::printf("xy");
    for (const Point2d& q : p.xy) std::printf(" %a %a", q.x, q.y);
    std::printf("\ndepth");
    for (double z : p.depth) std::printf(" %a", z);
    std::printf("\n");
    print_ints("state", p.state);
    std::printf("pcount %d\n", (int)p.count);

    const GatedMatches g = reassociate_gated(qdesc, qstate, qxy, tdesc, tstate, txy, tpstate, d[1], d[2], n[6],
                                             n[7] != 0, n[8] != 0);
    print_ints("origin", g.origin);
    print_ints("dist", g.dist);
    print_ints("candidates", g.candidates);
    std::printf("count %d\n", (int)g.count);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "search_mirror: %s\n", e.what());
    return 1;
  }
  return 0;
}
