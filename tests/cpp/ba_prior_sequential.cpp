// ba_prior_sequential.cpp -- sequential restatement of the bundle-adjustment solve with landmark priors (DESIGN.md §9
// rank 7, rules 1-9, plus rank 20, rules P1-P5), the reference of tests/test_ba_prior.py and tests/test_prior_gpu.py.
// One window at a time; every landmark is a record of its own with its observations inside it, and every sum over
// landmarks goes through 256 lane accumulators that are folded by a recursive halving tree (rule 9: what the xor
// butterfly leaves in a wave's first lane, then the four waves in order).  It shares the per-observation and per-block
// functions and the serial rules with the kernel through orbx_ba_math.h, and nothing with tests/cpp/ba_sequential.cpp:
// with every weight 0 the two must agree byte for byte, which ties them together.
//   g++ -O2 -std=c++17 -ffp-contract=off -fno-fast-math -shared -fPIC ba_prior_sequential.cpp
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../visual-odometry-gpu_amd/csrc/orbx_ba_math.h"

namespace {

struct View {  // one observation of a landmark
  int pose;
  double x, y;
  double W[18];  // Jc^T Jp at the accepted point (poses > 0)
};

struct Landmark {
  double X[3], cand[3];
  double A[3], lam;  // the prior: anchor and weight (rule P1); lam = 0: none
  double V[6], g[3], sp[3], Vinv[6], gs[3], D2[3];
  std::vector<View> views;  // ascending pose
  const View* seen_by(int pose) const {
    for (const View& v : views)
      if (v.pose == pose) return &v;
    return nullptr;
  }
};

// rule 9 for K sums at once: lane l of 256 takes landmarks l, l + 256, ... in ascending order
template <int K>
struct Lanes {
  double v[BA_LANES][K];
  Lanes() {
    for (auto& row : v)
      for (double& x : row) x = 0.0;
  }
  double* of(size_t landmark) { return v[landmark % BA_LANES]; }
  // a block of n lanes from lo: the lower half's fold combined with the upper half's -- the value the butterfly
  // leaves in the block's first lane
  double fold(int k, int lo, int n, bool is_max) const {
    if (n == 1) return v[lo][k];
    const double a = fold(k, lo, n / 2, is_max), b = fold(k, lo + n / 2, n / 2, is_max);
    return is_max ? (a > b ? a : b) : a + b;
  }
  double total(int k, bool is_max = false) const {
    const double a = fold(k, 0, 64, is_max), b = fold(k, 64, 64, is_max), c = fold(k, 128, 64, is_max),
                 d = fold(k, 192, 64, is_max);
    if (is_max) {
      double m = a > b ? a : b;
      m = m > c ? m : c;
      return m > d ? m : d;
    }
    return ((a + b) + c) + d;
  }
};

struct Window {
  int n_poses = 0, n_free = 0;
  double K4[4], delta = 1.0;
  std::vector<Landmark> lms;
  std::vector<double> x, xc;   // accepted and candidate poses
  std::vector<BaPose> Px, Pc;
  std::vector<double> U, sc, Dc, gcs, A, b;
  BaTrust T{};
  BaSummary sum{};
  double gmax = 0.0;
  bool bad = false;

  Window(const double* K9, int W, const double* poses6, int N, const double* points3, int n_obs,
         const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy, const double* prior_xyz,
         const double* prior_weight, int start, double delta_)
      : n_poses(W), n_free(W - 1), delta(delta_), lms((size_t)N), x(poses6, poses6 + 6 * W), xc(x), Px(W), Pc(W),
        U(27 * (W - 1)), sc(6 * (W - 1)), Dc(sc), gcs(sc), A(36 * (size_t)(W - 1) * (W - 1)), b(sc) {
    K4[0] = K9[0], K4[1] = K9[4], K4[2] = K9[2], K4[3] = K9[5];
    for (int j = 0; j < N; j++) {
      Landmark& L = lms[j];
      std::memset(&L.cand, 0, sizeof L.cand);
      for (int k = 0; k < 3; k++) L.X[k] = points3[3 * j + k], L.A[k] = prior_xyz ? prior_xyz[3 * j + k] : 0.0;
      L.lam = prior_weight ? prior_weight[j] : 0.0;
      if (start == 1 && L.lam > 0.0)  // rule P5
        for (int k = 0; k < 3; k++) L.X[k] = L.A[k];
    }
    for (int pose = 0; pose < W; pose++)  // pose by pose, so that every landmark's views ascend
      for (int o = 0; o < n_obs; o++)
        if (obs_pose[o] == pose) {
          View v{};
          v.pose = pose, v.x = obs_xy[2 * o], v.y = obs_xy[2 * o + 1];
          lms[obs_point[o]].views.push_back(v);
        }
    for (int i = 0; i < W; i++) {
      ba_pose_prepare(&x[6 * i], &Px[i]);
      if (!Px[i].ok) bad = true;
    }
    const double cost = 0.5 * linearize(true);
    T.radius = BA_RADIUS0, T.decrease = 2.0, T.cost = cost;
    sum = BaSummary{BA_NO_CONVERGENCE, 0, 0, 0, cost, cost};
  }

  // rules 1-4 at the accepted point, and P1-P3; returns sum rho
  double linearize(bool first) {
    Lanes<1> rho, gm;
    for (size_t j = 0; j < lms.size(); j++) {
      Landmark& L = lms[j];
      for (double& v : L.V) v = 0.0;
      for (double& v : L.g) v = 0.0;
      for (View& v : L.views) {
        BaObs ob;
        ba_obs_eval(K4, Px[v.pose], L.X, v.x, v.y, delta, true, &ob);
        rho.of(j)[0] = rho.of(j)[0] + ob.rho;
        if (first && ob.z == 0.0) bad = true;
        ba_accum_point(ob, L.V, L.g);
        if (v.pose > 0) ba_obs_W(ob, v.W);
      }
      ba_prior_accum(L.X, L.A, L.lam, L.V, L.g, rho.of(j));  // behind the last observation
      for (int k = 0; k < 3; k++) {
        const double a = pose_abs(L.g[k]);
        if (a > gm.of(j)[0]) gm.of(j)[0] = a;
      }
      if (first) L.sp[0] = ba_jacobi_scale(L.V[0]), L.sp[1] = ba_jacobi_scale(L.V[3]), L.sp[2] = ba_jacobi_scale(L.V[5]);
    }
    gmax = gm.total(0, true);
    for (int f = 0; f < n_free; f++) {
      Lanes<27> acc;
      for (size_t j = 0; j < lms.size(); j++) {
        const View* v = lms[j].seen_by(f + 1);
        if (!v) continue;
        BaObs ob;
        ba_obs_eval(K4, Px[f + 1], lms[j].X, v->x, v->y, delta, true, &ob);
        ba_accum_pose(ob, acc.of(j));
      }
      for (int k = 0; k < 27; k++) U[27 * f + k] = acc.total(k);
      for (int k = 21; k < 27; k++) {
        const double a = pose_abs(U[27 * f + k]);
        if (a > gmax) gmax = a;
      }
    }
    if (first)
      for (int f = 0; f < n_free; f++)
        for (int a = 0; a < 6; a++) sc[6 * f + a] = ba_jacobi_scale(U[27 * f + a * (a + 1) / 2 + a]);
    return rho.total(0);
  }

  // rules 5-7 at T.radius: the candidate and what rule 8 needs; false when the reduced system cannot be factored
  bool candidate(double* model, double* cost, double* step2, double* x2) {
    const int ld = 6 * n_free;
    for (Landmark& L : lms) ba_point_invert(L.V, L.g, L.sp, T.radius, L.Vinv, L.gs, L.D2);
    for (int f = 0; f < n_free; f++) {
      for (int g = 0; g < f; g++) {
        Lanes<36> acc;
        for (size_t j = 0; j < lms.size(); j++) {
          const Landmark& L = lms[j];
          const View *vf = L.seen_by(f + 1), *vg = L.seen_by(g + 1);
          if (!vf || !vg) continue;
          double Wf[18], Wg[18], Y[18];
          ba_scale_W(vf->W, &sc[6 * f], L.sp, Wf);
          ba_W_Vinv(Wf, L.Vinv, Y);
          ba_scale_W(vg->W, &sc[6 * g], L.sp, Wg);
          ba_accum_pair(Y, Wg, acc.of(j));
        }
        for (int r = 0; r < 6; r++)
          for (int c = 0; c < 6; c++) A[(6 * f + r) * ld + 6 * g + c] = acc.total(6 * r + c);
      }
      Lanes<27> acc;
      for (size_t j = 0; j < lms.size(); j++) {
        const Landmark& L = lms[j];
        const View* vf = L.seen_by(f + 1);
        if (!vf) continue;
        double Wf[18], Y[18];
        ba_scale_W(vf->W, &sc[6 * f], L.sp, Wf);
        ba_W_Vinv(Wf, L.Vinv, Y);
        ba_accum_diag(Y, Wf, acc.of(j));
        ba_accum_rhs(Y, L.gs, acc.of(j) + 21);
      }
      for (int r = 0, k = 0; r < 6; r++)
        for (int c = 0; c <= r; c++, k++) A[(6 * f + r) * ld + 6 * f + c] = acc.total(k);
      for (int r = 0; r < 6; r++) b[6 * f + r] = acc.total(21 + r);
    }
    ba_assemble(n_free, U.data(), sc.data(), T.radius, A.data(), ld, b.data(), Dc.data(), gcs.data());
    if (!ba_cholesky_solve(ld, ld, A.data(), b.data())) return false;
    double pm, ps2, px2;
    ba_pose_step(n_poses, x.data(), sc.data(), b.data(), Dc.data(), gcs.data(), xc.data(), &pm, &ps2, &px2);
    bool evaluable = true;
    for (int i = 0; i < n_poses; i++) {
      ba_pose_prepare(&xc[6 * i], &Pc[i]);
      if (!Pc[i].ok) evaluable = false;
    }
    Lanes<4> acc;
    for (size_t j = 0; j < lms.size(); j++) {
      Landmark& L = lms[j];
      double u[3] = {0.0, 0.0, 0.0};
      for (const View& v : L.views) {
        if (v.pose == 0) continue;
        double Ws[18];
        ba_scale_W(v.W, &sc[6 * (v.pose - 1)], L.sp, Ws);
        ba_accum_Wt_step(Ws, &b[6 * (v.pose - 1)], u);
      }
      double* a = acc.of(j);
      ba_point_step(L.Vinv, L.gs, u, L.D2, L.sp, L.X, L.cand, a);
      for (const View& v : L.views) {
        double z;
        a[3] = a[3] + ba_obs_cost(K4, Pc[v.pose], L.cand, v.x, v.y, delta, &z);
      }
      if (L.lam > 0.0) a[3] = a[3] + ba_prior_cost(L.cand, L.A, L.lam);  // rule P2
    }
    *model = 0.5 * (acc.total(0) + pm);
    *step2 = acc.total(1) + ps2;
    *x2 = acc.total(2) + px2;
    *cost = evaluable ? 0.5 * acc.total(3) : BA_DBL_MAX * 2.0;
    return true;
  }

  void solve(int max_iters) {
    bool done = true;
    if (bad || !(T.cost <= BA_DBL_MAX)) sum.termination = BA_FAILURE;
    else if (gmax <= BA_GRADIENT_TOL) sum.termination = BA_CONVERGENCE;
    else done = false;
    for (int it = 1; it <= max_iters && !done; it++) {
      double model = 0.0, cost = 0.0, step2 = 0.0, x2 = 0.0;
      const bool solved = candidate(&model, &cost, &step2, &x2);
      const int act = ba_trust_decide(&T, solved, model, cost, step2, x2);
      sum.iterations = it;
      if (act == BA_STEP_CONVERGED) sum.termination = BA_CONVERGENCE, done = true;
      if (act == BA_STEP_ACCEPTED) {
        sum.successful_steps++;
        x = xc, Px = Pc;
        for (Landmark& L : lms)
          for (int k = 0; k < 3; k++) L.X[k] = L.cand[k];
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

// the whole solve of one window; prior_xyz (3 N) and prior_weight (N) may both be NULL: no priors; start: 0 given,
// 1 anchor.  poses6 / points3 are rewritten only on convergence (rule P5)
void seq_ba_prior(const double* K9, int W, double* poses6, int N, double* points3, int n_obs, const int32_t* obs_point,
                  const int32_t* obs_pose, const double* obs_xy, const double* prior_xyz, const double* prior_weight,
                  int start, double delta, int max_iters, BaSummary* out) {
  Window w(K9, W, poses6, N, points3, n_obs, obs_point, obs_pose, obs_xy, prior_xyz, prior_weight, start, delta);
  w.solve(max_iters);
  if (w.sum.termination == BA_CONVERGENCE) {
    for (int k = 0; k < 6 * W; k++) poses6[k] = w.x[k];
    for (int j = 0; j < N; j++)
      for (int k = 0; k < 3; k++) points3[3 * j + k] = w.lms[j].X[k];
  }
  *out = w.sum;
}

// the two prior functions of orbx_ba_math.h on caller-held accumulators: V (6), gp (3), rho (1) are updated in place
void seq_prior_accum(const double* X, const double* A, double lam, double* V, double* gp, double* rho) {
  ba_prior_accum(X, A, lam, V, gp, rho);
}
double seq_prior_cost(const double* X, const double* A, double lam) { return ba_prior_cost(X, A, lam); }

}  // extern "C"
