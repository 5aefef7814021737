// pnp_mirror.cpp -- driver of orbx::solvePnPRansac (host/orb.hpp), compiled and run by
// tests/test_cpp_pnp.py.
//   pnp_mirror <blob>:  K (9 doubles), the number of points, iterationsCount, refine_iters and min_inliers (int32 each),
//                       the seed (uint64), reprojectionError and confidence (double each), the object points (n x 3
//                       doubles) and the image points (n x 2 doubles).
// Prints whether a pose was found, status, inliers, iters, rms, rvec and tvec (every double as a hex float), then the
// inlier indices.  rvec and tvec are preset to 7.5: a call that finds no pose must leave them alone.
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
    const int n = in.get<int32_t>(), iterations = in.get<int32_t>(), refine = in.get<int32_t>();
    const int min_inliers = in.get<int32_t>();
    const uint64_t seed = in.get<uint64_t>();
    const double error = in.get<double>(), confidence = in.get<double>();
    std::vector<orbx::Point3d> obj((size_t)n);
    for (auto& p : obj) p.x = in.get<double>(), p.y = in.get<double>(), p.z = in.get<double>();
    std::vector<orbx::Point2d> img((size_t)n);
    for (auto& p : img) p.x = in.get<double>(), p.y = in.get<double>();
    double rvec[3] = {7.5, 7.5, 7.5}, tvec[3] = {7.5, 7.5, 7.5};
    std::vector<int> inliers;
    orbx::PnPInfo info;
    const bool found = orbx::solvePnPRansac(obj, img, K, rvec, tvec, iterations, error, confidence, &inliers, seed,
                                            refine, min_inliers, &info);
    std::printf("found %d status %d inliers %d iters %d rms %a rvec %a %a %a tvec %a %a %a\n", found ? 1 : 0,
                info.status, info.inliers, info.iters, info.rms_px, rvec[0], rvec[1], rvec[2], tvec[0], tvec[1],
                tvec[2]);
    std::printf("indices");
    for (int i : inliers) std::printf(" %d", i);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  return 0;
}
