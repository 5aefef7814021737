// orbx_api_pnp.cpp -- host layer of liborbx.so (orbx_host.h) behind include/orbx_pnp.h: perspective-n-point with RANSAC
// over the landmarks block, one problem per (window, frame >= 2), its result block, the one problem of host arrays and
// the solve seeded with the PnP poses.  The reference has no such step: its window poses come
// from the chain of src/with_bundle_adjustment.cpp:196-208 alone.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbx_pnp.h"
#include "orbx_host.h"
#include "orbx_pnp_math.h"

using namespace orbx_host;

static_assert((int)ORBX_PNP_OK == (int)PNP_OK && (int)ORBX_PNP_NO_MODEL == (int)PNP_NO_MODEL, "orbx_pnp_status");
static_assert(ORBX_PNP_MAX_REFINE_ITERS == PNP_MAX_REFINE, "refine_iters");
static_assert(sizeof(orbx_pnp_record) == sizeof(OrbxPnpRecord) && sizeof(orbx_pnp_record) == 72, "orbx_pnp_record");

namespace {

// the argument rules both entries share; nothing is launched
int pnp_check(orbx_ctx* c, const double* K, double prob, double threshold_px, int max_iters, int refine_iters,
              int min_inliers) {
  if (!pose_args_ok(K, prob, threshold_px, max_iters)) return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  if (refine_iters < 0 || refine_iters > ORBX_PNP_MAX_REFINE_ITERS)
    return fail(c, ORBX_ERR_INVALID_ARG, "refine_iters outside [0, 20]");
  if (min_inliers < 4) return fail(c, ORBX_ERR_INVALID_ARG, "min_inliers < 4");
  return ORBX_OK;
}

double clamp01(double p) { return p < 0 ? 0.0 : (p > 1 ? 1.0 : p); }

int pnp_check_range(orbx_ctx* c, int first, int n) {
  if (c->pnp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no PnP batch has run");
  if (!range_ok(first, n, c->pnp.n)) return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the PnP block");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_pnp_ransac(orbx_ctx* c, const double* points3, const double* pixels_xy, int n, const double* K, double prob,
                    double threshold_px, int max_iters, uint64_t seed, int refine_iters, int min_inliers,
                    double* pose6, uint8_t* mask, int32_t* inliers, int32_t* iters, double* rms_px, int32_t* status) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = pnp_check(c, K, prob, threshold_px, max_iters, refine_iters, min_inliers);
  if (st != ORBX_OK) return st;
  if (n < 0 || (n > 0 && (!points3 || !pixels_xy))) return fail(c, ORBX_ERR_INVALID_ARG, "n < 0, or a NULL array");
  hipStream_t s = c->stream;
  if ((st = c->pnp.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->pnp.side, s};
  const size_t cap = (size_t)(n > 0 ? n : 1);
  const PnpBlock B(1, cap, 3);
  const PnpScratch S(1, cap, 3);
  if ((st = c->pnp.side.grow(c, c->pnp.hscr, S.bytes)) != ORBX_OK) return st;
  if ((st = c->pnp.side.grow(c, c->pnp.hblk, B.bytes)) != ORBX_OK) return st;
  std::vector<OrbxPnpCorr> up((size_t)n);
  for (int i = 0; i < n; i++) {
    for (int e = 0; e < 3; e++) up[i].X[e] = points3[3 * (size_t)i + e];
    up[i].x = pixels_xy[2 * (size_t)i], up[i].y = pixels_xy[2 * (size_t)i + 1];
  }
  if (n > 0)
    HIPCHK(c, hipMemcpyAsync(at<OrbxPnpCorr>(c->pnp.hscr, S.corr), up.data(), sizeof(OrbxPnpCorr) * (size_t)n,
                             hipMemcpyHostToDevice, s));
  const double K4[4] = {K[0], K[4], K[2], K[5]};
  const OrbxPnpIn none{};
  HIPCHK(c, orbx_launch_pnp(s, 1, 3, (int)cap, none, n, K4, clamp01(prob), threshold_px, max_iters, seed, refine_iters,
                            min_inliers, at<OrbxPnpCorr>(c->pnp.hscr, S.corr), at<int32_t>(c->pnp.hscr, S.cidx),
                            at<OrbxPnpRecord>(c->pnp.hblk, B.records), nullptr, at<uint8_t>(c->pnp.hblk, B.mask)));
  HIPCHK(c, hipStreamSynchronize(s));  // (also: `up` has been read)
  OrbxPnpRecord r;
  HIPCHK(c, hipMemcpy(&r, at<const OrbxPnpRecord>(c->pnp.hblk, B.records), sizeof r, hipMemcpyDeviceToHost));
  if (mask && n > 0) HIPCHK(c, hipMemcpy(mask, at<const uint8_t>(c->pnp.hblk, B.mask), (size_t)n, hipMemcpyDeviceToHost));
  if (pose6) std::memcpy(pose6, r.pose6, sizeof r.pose6);
  if (inliers) *inliers = r.inliers;
  if (iters) *iters = r.iters;
  if (rms_px) *rms_px = r.rms_px;
  if (status) *status = r.status;
  return ORBX_OK;
}

int orbx_window_poses_pnp_device(orbx_ctx* c, double prob, double threshold_px, int max_iters, uint64_t seed,
                                 int refine_iters, int min_inliers, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  if (c->lm.len < 3) return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has windows of 2 frames");
  int st = pnp_check(c, c->lm.K, prob, threshold_px, max_iters, refine_iters, min_inliers);
  if (st != ORBX_OK) return st;
  hipStream_t s = stream_of(c, stream);
  if ((st = c->pnp.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->pnp.side, s};
  // the landmarks block may have been built on another stream; a seeded solve may still be reading the last seeds
  if ((st = c->pnp.side.after(c, c->lm.side, s)) != ORBX_OK) return st;
  const int n = c->lm.n, cap = c->lm.cap, len = c->lm.len;
  const PnpBlock B((size_t)n, (size_t)cap, (size_t)len);
  const PnpScratch S((size_t)n, (size_t)cap, (size_t)len);
  if ((st = c->pnp.side.grow(c, c->pnp.scr, S.bytes)) != ORBX_OK) return st;
  if ((st = c->pnp.side.grow(c, c->pnp.blk, B.bytes)) != ORBX_OK) return st;
  // from here on the previous block is being replaced
  c->pnp.n = 0;
  const LmBlock L((size_t)n, (size_t)cap, (size_t)len);
  const LmScratch LS((size_t)n, cap, (size_t)len);
  OrbxPnpIn in;
  in.status = at<const int32_t>(c->lm.blk, L.status);
  in.pt_off = at<const int32_t>(c->lm.blk, L.pt_off);
  in.obs_off = at<const int32_t>(c->lm.blk, L.obs_off);
  in.rows = at<const int32_t>(c->lm.blk, L.rows);
  in.points3 = at<const double>(c->lm.blk, L.points);
  in.oxy = at<const double>(c->lm.blk, L.oxy);
  in.built6 = at<const double>(c->lm.scr, LS.poses);
  const double K4[4] = {c->lm.K[0], c->lm.K[4], c->lm.K[2], c->lm.K[5]};
  HIPCHK(c, orbx_launch_pnp(s, n, len, cap, in, 0, K4, clamp01(prob), threshold_px, max_iters, seed, refine_iters,
                            min_inliers, at<OrbxPnpCorr>(c->pnp.scr, S.corr), at<int32_t>(c->pnp.scr, S.cidx),
                            at<OrbxPnpRecord>(c->pnp.blk, B.records), at<double>(c->pnp.blk, B.poses6),
                            at<uint8_t>(c->pnp.blk, B.mask)));
  c->pnp.n = n;
  c->pnp.cap = cap;
  c->pnp.len = len;
  c->pnp.lm_gen = c->lm.gen;
  return ORBX_OK;
}

int orbx_window_poses_pnp_results_device(orbx_ctx* c, orbx_window_poses_pnp_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->pnp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no PnP batch has run");
  const PnpBlock B((size_t)c->pnp.n, (size_t)c->pnp.cap, (size_t)c->pnp.len);
  v->records = at<const orbx_pnp_record>(c->pnp.blk, B.records);
  v->poses6 = at<const double>(c->pnp.blk, B.poses6);
  v->mask = at<const uint8_t>(c->pnp.blk, B.mask);
  v->slot_capacity = c->pnp.cap;
  v->window_len = c->pnp.len;
  v->n_windows = c->pnp.n;
  return ORBX_OK;
}

int orbx_window_poses_pnp_fetch(orbx_ctx* c, int first, int n, orbx_pnp_record* records, double* poses6) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = pnp_check_range(c, first, n);
  if (st != ORBX_OK) return st;
  if ((st = c->pnp.side.wait(c)) != ORBX_OK) return st;
  const PnpBlock B((size_t)c->pnp.n, (size_t)c->pnp.cap, (size_t)c->pnp.len);
  const size_t per = (size_t)c->pnp.len - 2, len = (size_t)c->pnp.len;
  if (records)
    HIPCHK(c, hipMemcpy(records, at<const OrbxPnpRecord>(c->pnp.blk, B.records) + per * first,
                        sizeof(OrbxPnpRecord) * per * n, hipMemcpyDeviceToHost));
  if (poses6)
    HIPCHK(c, hipMemcpy(poses6, at<const double>(c->pnp.blk, B.poses6) + 6 * len * first, sizeof(double) * 6 * len * n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_window_poses_pnp_mask_fetch(orbx_ctx* c, int window, int k, uint8_t* mask, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = pnp_check_range(c, window, 1);
  if (st != ORBX_OK) return st;
  if (k < 2 || k >= c->pnp.len) return fail(c, ORBX_ERR_INVALID_ARG, "k outside [2, window_len)");
  if (capacity < 0) return fail(c, ORBX_ERR_INVALID_ARG, "a capacity is negative");
  if (c->pnp.lm_gen != c->lm.gen)
    return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has been rebuilt since the PnP batch");
  if ((st = c->pnp.side.wait(c)) != ORBX_OK) return st;
  const LmBlock L((size_t)c->lm.n, (size_t)c->lm.cap, (size_t)c->lm.len);
  int32_t po[2] = {0, 0};
  HIPCHK(c, hipMemcpy(po, at<const int32_t>(c->lm.blk, L.pt_off) + window, sizeof po, hipMemcpyDeviceToHost));
  const int np = po[1] - po[0];
  if (count) *count = np;
  if (mask && np > capacity) return fail(c, ORBX_ERR_CAPACITY, "PnP mask fetch: capacity is too small");
  const PnpBlock B((size_t)c->pnp.n, (size_t)c->pnp.cap, (size_t)c->pnp.len);
  const size_t row = ((size_t)window * (c->pnp.len - 2) + (k - 2)) * c->pnp.cap;
  if (mask && np > 0)
    HIPCHK(c, hipMemcpy(mask, at<const uint8_t>(c->pnp.blk, B.mask) + row, (size_t)np, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_bundle_adjust_landmarks_pnp_device(orbx_ctx* c, double huber_delta, int max_iters, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->pnp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no PnP batch has run");
  if (c->lm.n < 1 || c->pnp.lm_gen != c->lm.gen)
    return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has been rebuilt since the PnP batch");
  const PnpBlock B((size_t)c->pnp.n, (size_t)c->pnp.cap, (size_t)c->pnp.len);
  return lm_solve(c, huber_delta, max_iters, stream_of(c, stream), at<const double>(c->pnp.blk, B.poses6),
                  &c->pnp.side);
}

}  // extern "C"
