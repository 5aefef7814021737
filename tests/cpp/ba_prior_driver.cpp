// ba_prior_driver.cpp -- a main for tests/cpp/ba_prior_sequential.cpp: the stand-alone program of the host-side
// sanitizer run, and of tests/test_ba_prior.py, which compares its output with the shared
// library's.  Reads the windows tests/test_ba_prior.py::write_driver_input writes, solves each from its anchors
// (ORBX_PRIOR_START_ANCHOR) and prints the summary and every double of the result as a hex float.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fno-fast-math -fsanitize=address,undefined -fno-sanitize-recover=all
//       ba_prior_sequential.cpp ba_prior_driver.cpp -o ba_prior_driver.bin && ./ba_prior_driver.bin windows.bin
#include <cstdint>
#include <cstdio>
#include <vector>

struct Summary {
  int32_t termination, iterations, successful_steps, pad;
  double initial_cost, final_cost;
};

extern "C" void seq_ba_prior(const double* K9, int W, double* poses6, int N, double* points3, int n_obs,
                             const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                             const double* prior_xyz, const double* prior_weight, int start, double delta,
                             int max_iters, Summary* out);

template <class T>
static bool take(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_windows = 0;
  double K[9];
  if (std::fread(&n_windows, sizeof n_windows, 1, f) != 1 || std::fread(K, sizeof(double), 9, f) != 9) return 3;
  for (int w = 0; w < n_windows; w++) {
    int32_t dims[3];
    if (std::fread(dims, sizeof(int32_t), 3, f) != 3 || dims[0] < 2 || dims[1] < 1 || dims[2] < 1) return 3;
    const size_t W = (size_t)dims[0], N = (size_t)dims[1], M = (size_t)dims[2];
    std::vector<double> poses, pts, xy, anchors, weights;
    std::vector<int32_t> op, oq;
    if (!take(f, poses, 6 * W) || !take(f, pts, 3 * N) || !take(f, op, M) || !take(f, oq, M) || !take(f, xy, 2 * M) ||
        !take(f, anchors, 3 * N) || !take(f, weights, N))
      return 3;
    Summary s{};
    seq_ba_prior(K, (int)W, poses.data(), (int)N, pts.data(), (int)M, op.data(), oq.data(), xy.data(), anchors.data(),
                 weights.data(), 1, 1.0, 200, &s);
    std::printf("%d %d %d %a %a\n", s.termination, s.iterations, s.successful_steps, s.initial_cost, s.final_cost);
    for (double v : poses) std::printf("%a ", v);
    for (double v : pts) std::printf("%a ", v);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
