// ba_sequential.cpp -- sequential restatement of the bundle-adjustment solve, the reference of
// tests/test_ba.py.  One window at a time, in the order of Ceres' trust-region loop: evaluate, linearise, solve the
// damped normal equations through the Schur complement, evaluate the candidate, accept or reject.  Plain loops over
// residual blocks, dense std::vector storage.  It shares the per-observation and per-block functions and the serial
// rules (Cholesky, trust region) with the kernel through orbx_ba_math.h; the loops, the storage and the summation
// rule (rule 9: 256 lane-strided partial sums, xor butterfly, four waves in order) are written here on their own.
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC ba_sequential.cpp
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_ba_math.h"

namespace {

// rule 9: partial[l] was summed over landmarks l, l + 256, ... in ascending order
double tree(const double* partial, bool is_max = false) {
  double v[BA_LANES], n[BA_LANES];
  for (int l = 0; l < BA_LANES; l++) v[l] = partial[l];
  for (int d = 1; d < 64; d <<= 1) {
    for (int l = 0; l < BA_LANES; l++) n[l] = is_max ? (v[l] > v[l ^ d] ? v[l] : v[l ^ d]) : v[l] + v[l ^ d];
    for (int l = 0; l < BA_LANES; l++) v[l] = n[l];
  }
  if (is_max) {
    double m = v[0] > v[64] ? v[0] : v[64];
    m = m > v[128] ? m : v[128];
    return m > v[192] ? m : v[192];
  }
  return ((v[0] + v[64]) + v[128]) + v[192];
}

struct Solver {
  int W = 0, N = 0, P = 0;
  double K4[4] = {0, 0, 0, 0}, delta = 1.0;
  std::vector<int> row, opose;  // CSR by landmark
  std::vector<double> oxy;
  std::vector<double> x, cand, X, Xc;  // poses (6 W), points (3 N)
  std::vector<BaPose> Px, Pc;
  std::vector<double> V, gp, sp, Vinv, gs, D2, Wo;  // per landmark (6 / 3 N), per observation (18)
  std::vector<double> U, sc, Dc, gcs, A, b;
  BaTrust T{};
  BaSummary sum{};
  double gmax = 0.0;
  bool bad = false;

  int find(int j, int pose) const {
    for (int o = row[j]; o < row[j + 1]; o++)
      if (opose[o] == pose) return o;
    return -1;
  }

  double linearize(bool first) {
    std::vector<double> part(BA_LANES, 0.0), gpart(BA_LANES, 0.0);
    for (int j = 0; j < N; j++) {
      const int l = j % BA_LANES;
      double Vj[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
      for (int o = row[j]; o < row[j + 1]; o++) {
        BaObs ob;
        ba_obs_eval(K4, Px[opose[o]], &X[3 * j], oxy[2 * o], oxy[2 * o + 1], delta, true, &ob);
        part[l] = part[l] + ob.rho;
        if (first && ob.z == 0.0) bad = true;
        ba_accum_point(ob, Vj, g);
        if (opose[o] > 0) ba_obs_W(ob, &Wo[18 * o]);
      }
      for (int k = 0; k < 6; k++) V[6 * j + k] = Vj[k];
      for (int k = 0; k < 3; k++) {
        gp[3 * j + k] = g[k];
        const double a = pose_abs(g[k]);
        gpart[l] = a > gpart[l] ? a : gpart[l];
      }
      if (first) {
        sp[3 * j + 0] = ba_jacobi_scale(Vj[0]);
        sp[3 * j + 1] = ba_jacobi_scale(Vj[3]);
        sp[3 * j + 2] = ba_jacobi_scale(Vj[5]);
      }
    }
    const double sum_rho = tree(part.data());
    gmax = tree(gpart.data(), true);
    for (int f = 0; f < P; f++) {
      std::vector<double> acc(BA_LANES * 27, 0.0);
      for (int j = 0; j < N; j++) {
        const int o = find(j, f + 1);
        if (o < 0) continue;
        BaObs ob;
        ba_obs_eval(K4, Px[f + 1], &X[3 * j], oxy[2 * o], oxy[2 * o + 1], delta, true, &ob);
        ba_accum_pose(ob, &acc[(j % BA_LANES) * 27]);
      }
      for (int k = 0; k < 27; k++) {
        double p[BA_LANES];
        for (int l = 0; l < BA_LANES; l++) p[l] = acc[l * 27 + k];
        U[f * 27 + k] = tree(p);
      }
      for (int k = 21; k < 27; k++) {
        const double a = pose_abs(U[f * 27 + k]);
        gmax = a > gmax ? a : gmax;
      }
    }
    if (first)
      for (int r = 0; r < 6 * P; r++) sc[r] = ba_jacobi_scale(U[(r / 6) * 27 + (r % 6) * ((r % 6) + 1) / 2 + (r % 6)]);
    return sum_rho;
  }

  // one trust-region step at T.radius: the candidate, and what the decision needs
  bool step(double* model, double* cand_cost, double* step2, double* x2) {
    const double radius = T.radius;
    const int ld = 6 * P;
    for (int j = 0; j < N; j++)
      ba_point_invert(&V[6 * j], &gp[3 * j], &sp[3 * j], radius, &Vinv[6 * j], &gs[3 * j], &D2[3 * j]);
    std::fill(A.begin(), A.end(), 0.0);
    std::fill(b.begin(), b.end(), 0.0);
    for (int f = 0; f < P; f++) {
      for (int g = 0; g < f; g++) {  // two different poses: a full 6x6 block
        std::vector<double> acc(BA_LANES * 36, 0.0);
        for (int j = 0; j < N; j++) {
          const int of = find(j, f + 1), og = find(j, g + 1);
          if (of < 0 || og < 0) continue;
          double Wf[18], Wg[18], Y[18];
          ba_scale_W(&Wo[18 * of], &sc[6 * f], &sp[3 * j], Wf);
          ba_W_Vinv(Wf, &Vinv[6 * j], Y);
          ba_scale_W(&Wo[18 * og], &sc[6 * g], &sp[3 * j], Wg);
          ba_accum_pair(Y, Wg, &acc[(j % BA_LANES) * 36]);
        }
        for (int k = 0; k < 36; k++) {
          double p[BA_LANES];
          for (int l = 0; l < BA_LANES; l++) p[l] = acc[l * 36 + k];
          A[(6 * f + k / 6) * ld + 6 * g + k % 6] = tree(p);
        }
      }
      std::vector<double> acc(BA_LANES * 27, 0.0);  // the pose with itself: lower triangle, then the right side
      for (int j = 0; j < N; j++) {
        const int of = find(j, f + 1);
        if (of < 0) continue;
        double Wf[18], Y[18];
        double* a = &acc[(j % BA_LANES) * 27];
        ba_scale_W(&Wo[18 * of], &sc[6 * f], &sp[3 * j], Wf);
        ba_W_Vinv(Wf, &Vinv[6 * j], Y);
        ba_accum_diag(Y, Wf, a);
        ba_accum_rhs(Y, &gs[3 * j], a + 21);
      }
      int k = 0;
      for (int r = 0; r < 6; r++)
        for (int c = 0; c <= r; c++, k++) {
          double p[BA_LANES];
          for (int l = 0; l < BA_LANES; l++) p[l] = acc[l * 27 + k];
          A[(6 * f + r) * ld + 6 * f + c] = tree(p);
        }
      for (int r = 0; r < 6; r++) {
        double p[BA_LANES];
        for (int l = 0; l < BA_LANES; l++) p[l] = acc[l * 27 + 21 + r];
        b[6 * f + r] = tree(p);
      }
    }
    ba_assemble(P, U.data(), sc.data(), radius, A.data(), ld, b.data(), Dc.data(), gcs.data());
    if (!ba_cholesky_solve(6 * P, ld, A.data(), b.data())) return false;
    double pm, ps2, px2;
    ba_pose_step(W, x.data(), sc.data(), b.data(), Dc.data(), gcs.data(), cand.data(), &pm, &ps2, &px2);
    bool pose_ok = true;
    for (int i = 0; i < W; i++) {
      ba_pose_prepare(&cand[6 * i], &Pc[i]);
      pose_ok = pose_ok && Pc[i].ok;
    }
    std::vector<double> acc(BA_LANES * 4, 0.0);
    for (int j = 0; j < N; j++) {
      double* a = &acc[(j % BA_LANES) * 4];
      double u[3] = {0, 0, 0};
      for (int o = row[j]; o < row[j + 1]; o++) {
        const int i = opose[o];
        if (i == 0) continue;
        double Ws[18];
        ba_scale_W(&Wo[18 * o], &sc[6 * (i - 1)], &sp[3 * j], Ws);
        ba_accum_Wt_step(Ws, &b[6 * (i - 1)], u);
      }
      ba_point_step(&Vinv[6 * j], &gs[3 * j], u, &D2[3 * j], &sp[3 * j], &X[3 * j], &Xc[3 * j], a);
      for (int o = row[j]; o < row[j + 1]; o++) {
        double z;
        a[3] = a[3] + ba_obs_cost(K4, Pc[opose[o]], &Xc[3 * j], oxy[2 * o], oxy[2 * o + 1], delta, &z);
      }
    }
    double tot[4];
    for (int k = 0; k < 4; k++) {
      double p[BA_LANES];
      for (int l = 0; l < BA_LANES; l++) p[l] = acc[l * 4 + k];
      tot[k] = tree(p);
    }
    *model = 0.5 * (tot[0] + pm);
    *step2 = tot[1] + ps2;
    *x2 = tot[2] + px2;
    *cand_cost = pose_ok ? 0.5 * tot[3] : BA_DBL_MAX * 2.0;
    return true;
  }

  void init(const double* K9, int W_, const double* poses6, int N_, const double* points3, int n_obs,
            const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy, double delta_) {
    W = W_, N = N_, P = W - 1, delta = delta_;
    K4[0] = K9[0], K4[1] = K9[4], K4[2] = K9[2], K4[3] = K9[5];
    std::vector<int> order(n_obs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) {
      return obs_point[a] != obs_point[c] ? obs_point[a] < obs_point[c] : obs_pose[a] < obs_pose[c];
    });
    row.assign(N + 1, 0);
    opose.resize(n_obs), oxy.resize(2 * (size_t)n_obs);
    for (int k = 0; k < n_obs; k++) {
      const int o = order[k];
      row[obs_point[o] + 1]++;
      opose[k] = obs_pose[o];
      oxy[2 * k] = obs_xy[2 * o], oxy[2 * k + 1] = obs_xy[2 * o + 1];
    }
    for (int j = 0; j < N; j++) row[j + 1] += row[j];
    x.assign(poses6, poses6 + 6 * W), cand = x;
    X.assign(points3, points3 + 3 * (size_t)N), Xc = X;
    Px.resize(W), Pc.resize(W);
    V.assign(6 * (size_t)N, 0.0), Vinv = V;
    gp.assign(3 * (size_t)N, 0.0), sp = gp, gs = gp, D2 = gp;
    Wo.assign(18 * (size_t)n_obs, 0.0);
    U.assign(27 * P, 0.0), sc.assign(6 * P, 0.0), Dc = sc, gcs = sc, b = sc;
    A.assign(36 * (size_t)P * P, 0.0);
    bad = false;
    for (int i = 0; i < W; i++) {
      ba_pose_prepare(&x[6 * i], &Px[i]);
      if (!Px[i].ok) bad = true;
    }
    const double cost = 0.5 * linearize(true);
    T.radius = BA_RADIUS0, T.decrease = 2.0, T.cost = cost;
    sum = BaSummary{BA_NO_CONVERGENCE, 0, 0, 0, cost, cost};
  }

  void solve(int max_iters) {
    bool done = false;
    if (bad || !(T.cost <= BA_DBL_MAX)) {
      sum.termination = BA_FAILURE;
      done = true;
    } else if (gmax <= BA_GRADIENT_TOL) {
      sum.termination = BA_CONVERGENCE;
      done = true;
    }
    for (int it = 1; it <= max_iters && !done; it++) {
      double model = 0.0, cand_cost = 0.0, step2 = 0.0, x2 = 0.0;
      const bool solved = step(&model, &cand_cost, &step2, &x2);
      const int act = ba_trust_decide(&T, solved, model, cand_cost, step2, x2);
      sum.iterations = it;
      if (act == BA_STEP_CONVERGED) sum.termination = BA_CONVERGENCE, done = true;
      if (act == BA_STEP_ACCEPTED) {
        sum.successful_steps++;
        x = cand, X = Xc, Px = Pc;
        linearize(false);
        if (gmax <= BA_GRADIENT_TOL) sum.termination = BA_CONVERGENCE, done = true;
      }
      if (!done && T.radius <= BA_RADIUS_MIN) sum.termination = BA_CONVERGENCE, done = true;
    }
    sum.final_cost = T.cost;
  }
};

}  // namespace

extern "C" {

void seq_sincos(double x, double* s, double* c) { ba_sincos(x, s, c); }

// residual (2), Jc (12), Jp (6), rho of one observation
void seq_obs_eval(const double* K9, const double* pose6, const double* X, const double* xy, double delta, int weighted,
                  double* r, double* Jc, double* Jp, double* rho) {
  const double K4[4] = {K9[0], K9[4], K9[2], K9[5]};
  BaPose P;
  ba_pose_prepare(pose6, &P);
  BaObs o;
  ba_obs_eval(K4, P, X, xy[0], xy[1], delta, weighted != 0, &o);
  for (int k = 0; k < 2; k++) r[k] = o.r[k];
  for (int k = 0; k < 12; k++) Jc[k] = o.Jc[k];
  for (int k = 0; k < 6; k++) Jp[k] = o.Jp[k];
  *rho = o.rho;
}

// the whole solve of one window; poses6 / points3 are rewritten only on convergence
void seq_ba(const double* K9, int W, double* poses6, int N, double* points3, int n_obs, const int32_t* obs_point,
            const int32_t* obs_pose, const double* obs_xy, double delta, int max_iters, BaSummary* out) {
  Solver s;
  s.init(K9, W, poses6, N, points3, n_obs, obs_point, obs_pose, obs_xy, delta);
  s.solve(max_iters);
  if (s.sum.termination == BA_CONVERGENCE) {
    std::copy(s.x.begin(), s.x.end(), poses6);
    std::copy(s.X.begin(), s.X.end(), points3);
  }
  *out = s.sum;
}

// the first step at trust-region radius `radius`: candidate - start for poses (6 W) and points (3 N); 0 if the
// reduced system could not be factored
int seq_ba_first_step(const double* K9, int W, const double* poses6, int N, const double* points3, int n_obs,
                      const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy, double delta,
                      double radius, double* dposes, double* dpoints) {
  Solver s;
  s.init(K9, W, poses6, N, points3, n_obs, obs_point, obs_pose, obs_xy, delta);
  s.T.radius = radius;
  double m, c, s2, x2;
  if (!s.step(&m, &c, &s2, &x2)) return 0;
  for (int k = 0; k < 6 * W; k++) dposes[k] = s.cand[k] - s.x[k];
  for (int k = 0; k < 3 * N; k++) dpoints[k] = s.Xc[k] - s.X[k];
  return 1;
}

}  // extern "C"
