// orbx_api_tracks.cpp -- host layer of liborbx.so (orbx_host.h): pose, triangulated points and relative scale of
// every consecutive frame pair of tracked windows, from the tracks block on the device.
// The point lists of src/feature_tracking.cpp:166-193 handed to get_pose (:222-242) and get_scale (:244-310), and
// src/with_bundle_adjustment.cpp:180-203, for many windows per call.
#include <algorithm>
#include <cstring>

#include "orbx_host.h"

using namespace orbx_host;

static_assert(sizeof(orbx_tracks_pose_result) == sizeof(OrbxPoseOut), "orbx_tracks_pose_result is OrbxPoseOut");
static_assert(sizeof(orbx_tracks_scale_result) == sizeof(OrbxScaleOut), "orbx_tracks_scale_result is OrbxScaleOut");

namespace {

int tp_pairs(const orbx_ctx* c) { return c->tp.n * (c->tp.len - 1); }

// enqueues the four kernels on s; arguments are checked
int tp_run(orbx_ctx* c, const double* K, const float* d_tracks, const int32_t* d_seen, int n, int cap, int len,
           double prob, double threshold, int max_iters, uint64_t seed, hipStream_t s) {
  int st = c->tp.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->tp.side, s};
  // the tracks may be the windows tracker's block, written on another stream
  if ((st = c->tp.side.after(c, c->lkw.side, s)) != ORBX_OK) return st;
  const TpBlock B(n, cap, len);
  const int pairs = n * (len - 1);
  if ((st = c->tp.side.grow(c, c->tp.scr, tp_scratch_bytes(n, cap, len))) != ORBX_OK) return st;
  if ((st = c->tp.side.grow(c, c->tp.blk, B.bytes)) != ORBX_OK) return st;
  // from here on the previous block is being replaced (a larger one has already taken its place)
  c->tp.n = 0;
  uint8_t* b = (uint8_t*)c->tp.blk.p;
  OrbxPosePt* pts = (OrbxPosePt*)c->tp.scr.p;
  OrbxPoseOut* pose = (OrbxPoseOut*)(b + B.pose);
  int32_t* npts = (int32_t*)(b + B.n);
  int32_t* slot_of = (int32_t*)(b + B.slot_of);
  float* xyz = (float*)(b + B.xyz);
  HIPCHK(c, orbx_launch_tracks_prep(s, n, cap, len, d_tracks, d_seen, K, pts, npts, slot_of, b + B.mask, xyz,
                                    b + B.valid));
  HIPCHK(c, orbx_launch_pose_ransac(s, pairs, cap, pts, npts, K, prob, threshold, max_iters, seed, pose, b + B.mask));
  HIPCHK(c, orbx_launch_tracks_triangulate(s, n, cap, len, d_tracks, npts, slot_of, pose, K, xyz, b + B.valid));
  // the join on the slot: the slot lists are both index arrays, one chain per window
  HIPCHK(c, orbx_launch_scale_join(s, pairs, len - 1, cap, npts, slot_of, slot_of, xyz, b + B.valid, pose,
                                   (OrbxScaleOut*)(b + B.scale)));
  c->tp.n = n;
  c->tp.cap = cap;
  c->tp.len = len;
  return ORBX_OK;
}

}  // namespace

namespace orbx_host {

int tp_check(orbx_ctx* c, const double* K, const void* tracks, const void* seen, int n, int cap, int len, double prob,
             double threshold, int max_iters) {
  if (!pose_args_ok(K, prob, threshold, max_iters) || !finite_all(K, 9))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  if (!tracks || !seen) return fail(c, ORBX_ERR_INVALID_ARG, "tracks or seen is NULL");
  if (n < 1 || cap < 1 || len < 2)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1, slot_capacity < 1 or window_len < 2");
  if ((size_t)cap * 16 > ORBX_SCALE_LDS_MAX)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more slots per window than the join holds in LDS");
  if ((unsigned long long)n * (unsigned long long)(len - 1) * (unsigned long long)cap > 0x7fffffffull)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more list positions in a batch than 32-bit offsets hold");
  return ORBX_OK;
}

}  // namespace orbx_host

extern "C" {

int orbx_tracks_pose_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                            int n_windows, int slot_capacity, int window_len, double prob, double threshold,
                            int max_iters, uint64_t seed, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = tp_check(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, prob, threshold, max_iters);
  if (st != ORBX_OK) return st;
  return tp_run(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, prob, threshold, max_iters, seed,
                stream_of(c, stream));
}

int orbx_tracks_pose_results_device(orbx_ctx* c, orbx_tracks_pose_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->tp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no tracks have been posed");
  const TpBlock B(c->tp.n, c->tp.cap, c->tp.len);
  const uint8_t* b = (const uint8_t*)c->tp.blk.p;
  v->pose = (const orbx_tracks_pose_result*)(b + B.pose);
  v->n = (const int32_t*)(b + B.n);
  v->scale = (const orbx_tracks_scale_result*)(b + B.scale);
  v->slot_of = (const int32_t*)(b + B.slot_of);
  v->mask = b + B.mask;
  v->xyz = (const float*)(b + B.xyz);
  v->valid = b + B.valid;
  v->slot_capacity = c->tp.cap;
  v->window_len = c->tp.len;
  v->n_windows = c->tp.n;
  v->n_pairs = tp_pairs(c);
  return ORBX_OK;
}

int orbx_tracks_pose_fetch(orbx_ctx* c, int first, int n, double* E, double* R, double* t, int32_t* inliers,
                           int32_t* good, int32_t* iters, int32_t* counts, double* scale, int32_t* triplets,
                           int32_t* ratios_used) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->tp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no tracks have been posed");
  if (!range_ok(first, n, tp_pairs(c), 0))
    return fail(c, ORBX_ERR_INVALID_ARG, "pairs outside the last tracks-pose block");
  if (n == 0) return ORBX_OK;
  const int st = c->tp.side.wait(c);
  if (st != ORBX_OK) return st;
  const TpBlock B(c->tp.n, c->tp.cap, c->tp.len);
  const uint8_t* b = (const uint8_t*)c->tp.blk.p;
  if (E || R || t || inliers || good || iters) {
    std::vector<OrbxPoseOut> r((size_t)n);
    HIPCHK(c, hipMemcpy(r.data(), (const OrbxPoseOut*)(b + B.pose) + first, sizeof(OrbxPoseOut) * (size_t)n,
                        hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++)
      pose_unpack(r[(size_t)i], E ? E + 9 * i : nullptr, R ? R + 9 * i : nullptr, t ? t + 3 * i : nullptr,
                  inliers ? inliers + i : nullptr, good ? good + i : nullptr, iters ? iters + i : nullptr);
  }
  if (counts)
    HIPCHK(c, hipMemcpy(counts, (const int32_t*)(b + B.n) + first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (scale || triplets || ratios_used) {
    std::vector<OrbxScaleOut> r((size_t)n);
    HIPCHK(c, hipMemcpy(r.data(), (const OrbxScaleOut*)(b + B.scale) + first, sizeof(OrbxScaleOut) * (size_t)n,
                        hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
      if (scale) scale[i] = r[(size_t)i].scale;
      if (triplets) triplets[i] = r[(size_t)i].triplets;
      if (ratios_used) ratios_used[i] = r[(size_t)i].ratios_used;
    }
  }
  return ORBX_OK;
}

int orbx_tracks_pose_pair_fetch(orbx_ctx* c, int pair, int32_t* slot_of, uint8_t* mask, float* xyz, uint8_t* valid,
                                int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count || capacity < 0) return fail(c, ORBX_ERR_INVALID_ARG, "bad pair output arguments");
  if (c->tp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no tracks have been posed");
  if (pair < 0 || pair >= tp_pairs(c)) return fail(c, ORBX_ERR_INVALID_ARG, "pair outside the last tracks-pose block");
  const int st = c->tp.side.wait(c);
  if (st != ORBX_OK) return st;
  const TpBlock B(c->tp.n, c->tp.cap, c->tp.len);
  const uint8_t* b = (const uint8_t*)c->tp.blk.p;
  int32_t np = 0;
  HIPCHK(c, hipMemcpy(&np, (const int32_t*)(b + B.n) + pair, sizeof np, hipMemcpyDeviceToHost));
  *count = np;
  if (np > capacity) return fail(c, ORBX_ERR_CAPACITY, "capacity smaller than the pair's list");
  if (np == 0) return ORBX_OK;
  const size_t row = (size_t)pair * c->tp.cap;
  if (slot_of)
    HIPCHK(c, hipMemcpy(slot_of, (const int32_t*)(b + B.slot_of) + row, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost));
  if (mask) HIPCHK(c, hipMemcpy(mask, b + B.mask + row, (size_t)np, hipMemcpyDeviceToHost));
  if (xyz) HIPCHK(c, hipMemcpy(xyz, (const float*)(b + B.xyz) + 3 * row, sizeof(float) * 3 * (size_t)np, hipMemcpyDeviceToHost));
  if (valid) HIPCHK(c, hipMemcpy(valid, b + B.valid + row, (size_t)np, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_tracks_pose(orbx_ctx* c, const double* K, const float* tracks_xy, const int32_t* seen, int n_slots,
                     int window_len, double prob, double threshold, int max_iters, uint64_t seed, double* E, double* R,
                     double* t, int32_t* inliers, int32_t* good, int32_t* iters, int32_t* counts, double* scale,
                     int32_t* triplets, int32_t* ratios_used) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = tp_check(c, K, tracks_xy, seen, 1, n_slots, window_len, prob, threshold, max_iters);
  if (st != ORBX_OK) return st;
  const float* d_tracks;
  const int32_t* d_seen;
  if ((st = stage_tracks(c, c->tp.side, c->tp.stage, tracks_xy, seen, n_slots, window_len, &d_tracks, &d_seen)) != ORBX_OK)
    return st;
  if ((st = tp_run(c, K, d_tracks, d_seen, 1, n_slots, window_len, prob, threshold, max_iters, seed, c->stream)) !=
      ORBX_OK)
    return st;
  return orbx_tracks_pose_fetch(c, 0, window_len - 1, E, R, t, inliers, good, iters, counts, scale, triplets,
                                ratios_used);
}

}  // extern "C"
