// orbx_api_prior.cpp -- host layer of liborbx.so (orbx_host.h) behind include/orbx_prior.h: landmark priors in the
// window solve.  The two host entries are orbx_bundle_adjust / _batch with two more arrays
// (ba_batch, orbx_api_geom.cpp); the device entries gather the priors of a carried window from the carry block
// (rule P6) and solve the landmarks block with them (lm_solve, orbx_api_landmarks.cpp).  The reference's problem has
// reprojection residuals only (src/with_bundle_adjustment.cpp:612-679) and keeps no point across a solve
// (src/with_bundle_adjustment.cpp:586-593).
#include <cmath>
#include <vector>

#include "../../include/orbx_prior.h"
#include "orbx_host.h"

using namespace orbx_host;

namespace {

bool start_ok(int start) { return start == ORBX_PRIOR_START_GIVEN || start == ORBX_PRIOR_START_ANCHOR; }

int priors_range(orbx_ctx* c, int first, int n) {
  if (c->prior.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no priors have been gathered");
  if (!range_ok(first, n, c->prior.n)) return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the priors block");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_bundle_adjust_prior_batch(orbx_ctx* c, const double* K, int n_windows, const int32_t* pose_offset,
                                   double* poses6, const int32_t* point_offset, double* points3,
                                   const int32_t* obs_offset, const int32_t* obs_point, const int32_t* obs_pose,
                                   const double* obs_xy, const double* prior_xyz, const double* prior_weight, int start,
                                   double huber_delta, int max_iters, orbx_ba_summary* summaries) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!start_ok(start)) return fail(c, ORBX_ERR_INVALID_ARG, "start is neither ORBX_PRIOR_START_GIVEN nor _ANCHOR");
  if ((prior_xyz == nullptr) != (prior_weight == nullptr))
    return fail(c, ORBX_ERR_INVALID_ARG, "prior_xyz and prior_weight are NULL together or not at all");
  const BaPriorArgs prior{prior_xyz, prior_weight, start};
  return ba_batch(c, K, n_windows, pose_offset, poses6, point_offset, points3, obs_offset, obs_point, obs_pose, obs_xy,
                  huber_delta, max_iters, summaries, &prior);
}

int orbx_bundle_adjust_prior(orbx_ctx* c, const double* K, int n_poses, double* poses6, int n_points, double* points3,
                             int n_obs, const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                             const double* prior_xyz, const double* prior_weight, int start, double huber_delta,
                             int max_iters, orbx_ba_summary* summary) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n_poses < 0 || n_points < 0 || n_obs < 0) return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  const int32_t po[2] = {0, n_poses}, pt[2] = {0, n_points}, ob[2] = {0, n_obs};
  return orbx_bundle_adjust_prior_batch(c, K, 1, po, poses6, pt, points3, ob, obs_point, obs_pose, obs_xy, prior_xyz,
                                        prior_weight, start, huber_delta, max_iters, summary);
}

int orbx_landmarks_priors_carried_device(orbx_ctx* c, double weight, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!(weight >= 0.0) || !std::isfinite(weight)) return fail(c, ORBX_ERR_INVALID_ARG, "weight is negative or not finite");
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  if (c->carry.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks have been carried");
  if (c->carry.n != c->lm.n || c->carry.cap != c->lm.cap)
    return fail(c, ORBX_ERR_INVALID_ARG, "the carry block's n_windows or slot_capacity differs from the landmarks block's");
  hipStream_t s = stream_of(c, stream);
  int st = c->lm.side.enter(c, s);  // (the priors run under the landmarks' event: they belong to that block)
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->lm.side, s};
  if ((st = c->lm.side.after(c, c->carry.side, s)) != ORBX_OK) return st;
  const int n = c->lm.n, cap = c->lm.cap;
  const LmBlock L((size_t)n, (size_t)cap, (size_t)c->lm.len);
  const CarryBlock CB((size_t)n, (size_t)cap);
  const PriorBlock B((size_t)n, (size_t)cap);
  if ((st = c->lm.side.grow(c, c->prior.blk, B.bytes)) != ORBX_OK) return st;
  c->prior.n = 0;  // from here on the previous block is being replaced
  HIPCHK(c, hipMemcpyAsync(at<int32_t>(c->prior.blk, B.pt_off), at<const int32_t>(c->lm.blk, L.pt_off),
                           sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
  HIPCHK(c, orbx_launch_prior_gather(s, at<const int32_t>(c->lm.blk, L.status), at<const int32_t>(c->lm.blk, L.pt_off),
                                     at<const int32_t>(c->lm.blk, L.slot), at<const double>(c->carry.blk, CB.xyz),
                                     at<const int32_t>(c->carry.blk, CB.point), n, cap, weight,
                                     at<double>(c->prior.blk, B.prior), at<int32_t>(c->prior.blk, B.count)));
  c->prior.n = n;
  c->prior.cap = cap;
  c->prior.lm_gen = c->lm.gen;
  return ORBX_OK;
}

int orbx_landmarks_priors_results_device(orbx_ctx* c, orbx_landmarks_priors_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->prior.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no priors have been gathered");
  const PriorBlock B((size_t)c->prior.n, (size_t)c->prior.cap);
  v->prior = at<const double>(c->prior.blk, B.prior);
  v->count = at<const int32_t>(c->prior.blk, B.count);
  v->n_windows = c->prior.n;
  return ORBX_OK;
}

int orbx_landmarks_priors_fetch(orbx_ctx* c, int first, int n, double* prior_xyz, double* prior_weight, int32_t* count,
                                int capacity, int* n_points) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = priors_range(c, first, n);
  if (st != ORBX_OK) return st;
  if (capacity < 0) return fail(c, ORBX_ERR_INVALID_ARG, "a capacity is negative");
  if ((st = c->lm.side.wait(c)) != ORBX_OK) return st;
  const PriorBlock B((size_t)c->prior.n, (size_t)c->prior.cap);
  int32_t p0 = 0, p1 = 0;
  HIPCHK(c, hipMemcpy(&p0, at<const int32_t>(c->prior.blk, B.pt_off) + first, sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(&p1, at<const int32_t>(c->prior.blk, B.pt_off) + first + n, sizeof(int32_t), hipMemcpyDeviceToHost));
  const size_t np = (size_t)(p1 - p0);
  if (n_points) *n_points = (int)np;
  if ((prior_xyz || prior_weight) && np > (size_t)capacity)
    return fail(c, ORBX_ERR_CAPACITY, "priors fetch: capacity is too small");
  if ((prior_xyz || prior_weight) && np) {
    std::vector<double> p4(4 * np);
    HIPCHK(c, hipMemcpy(p4.data(), at<const double>(c->prior.blk, B.prior) + 4 * (size_t)p0, sizeof(double) * 4 * np,
                        hipMemcpyDeviceToHost));
    for (size_t j = 0; j < np; j++) {
      if (prior_xyz) prior_xyz[3 * j] = p4[4 * j], prior_xyz[3 * j + 1] = p4[4 * j + 1], prior_xyz[3 * j + 2] = p4[4 * j + 2];
      if (prior_weight) prior_weight[j] = p4[4 * j + 3];
    }
  }
  if (count)
    HIPCHK(c, hipMemcpy(count, at<const int32_t>(c->prior.blk, B.count) + first, sizeof(int32_t) * n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_bundle_adjust_landmarks_prior_device(orbx_ctx* c, double huber_delta, int max_iters, int start, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!start_ok(start)) return fail(c, ORBX_ERR_INVALID_ARG, "start is neither ORBX_PRIOR_START_GIVEN nor _ANCHOR");
  if (c->prior.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no priors have been gathered");
  if (c->prior.lm_gen != c->lm.gen || c->prior.n != c->lm.n || c->prior.cap != c->lm.cap)
    return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has been rebuilt since the priors were gathered");
  const PriorBlock B((size_t)c->prior.n, (size_t)c->prior.cap);
  // (the gather ran under the landmarks' event, which lm_solve enters: on another stream it has finished by then)
  return lm_solve(c, huber_delta, max_iters, stream_of(c, stream), nullptr, nullptr, at<const double>(c->prior.blk, B.prior),
                  start);
}

}  // extern "C"
