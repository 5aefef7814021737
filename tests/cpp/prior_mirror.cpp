// prior_mirror.cpp -- driver of orbx::bundle_adjust_with_priors (host/orb.hpp), compiled and run
// by tests/test_cpp_prior.py.
//   prior_mirror <blob>:  K (9 doubles), n_poses, n_points, n_obs, n_priors (0 or n_points), start and max_iters (int32
//                         each), huber_delta (double), the poses (n_poses x 6 doubles), the points (n_points x 3),
//                         obs_point and obs_pose (n_obs int32 each), obs_xy (n_obs x 2 doubles), the anchors
//                         (n_priors x 3 doubles) and the weights (n_priors doubles).
// Prints the summary, then the poses and the points, every double as a hex float.
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
    const int n_poses = in.get<int32_t>(), n_points = in.get<int32_t>(), n_obs = in.get<int32_t>();
    const int n_priors = in.get<int32_t>(), start = in.get<int32_t>(), max_iters = in.get<int32_t>();
    const double delta = in.get<double>();
    std::vector<double> poses((size_t)6 * n_poses), weights((size_t)n_priors);
    for (double& v : poses) v = in.get<double>();
    std::vector<orbx::Point3d> points((size_t)n_points), anchors((size_t)n_priors);
    for (auto& p : points) p.x = in.get<double>(), p.y = in.get<double>(), p.z = in.get<double>();
    std::vector<int32_t> op((size_t)n_obs), oq((size_t)n_obs);
    for (auto& v : op) v = in.get<int32_t>();
    for (auto& v : oq) v = in.get<int32_t>();
    std::vector<orbx::Point2d> xy((size_t)n_obs);
    for (auto& p : xy) p.x = in.get<double>(), p.y = in.get<double>();
    for (auto& p : anchors) p.x = in.get<double>(), p.y = in.get<double>(), p.z = in.get<double>();
    for (double& v : weights) v = in.get<double>();
    const orbx::PriorSolve r =
        orbx::bundle_adjust_with_priors(K, poses, points, op, oq, xy, anchors, weights, start, delta, max_iters);
    std::printf("summary %d %d %d %a %a converged %d\n", r.summary.termination, r.summary.iterations,
                r.summary.successful_steps, r.summary.initial_cost, r.summary.final_cost, r.converged() ? 1 : 0);
    std::printf("poses");
    for (double v : r.poses6) std::printf(" %a", v);
    std::printf("\npoints");
    for (const orbx::Point3d& p : r.points) std::printf(" %a %a %a", p.x, p.y, p.z);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  return 0;
}
