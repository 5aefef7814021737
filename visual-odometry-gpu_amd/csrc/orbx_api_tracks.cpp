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

// a buffer of the tracks-pose path of at least `bytes`: the new allocation is made BEFORE the old one is released, so
// that a failed call keeps what it had
int tp_grow(orbx_ctx* c, DevBuf& b, size_t bytes) {
  if (b.p && b.bytes >= bytes) return ORBX_OK;
  const int st = c->tp.side.wait(c);  // (the old allocation may still be read or written)
  if (st != ORBX_OK) return st;
  bytes = align_up_sz(std::max<size_t>(bytes, 256), 256);
  void* p = nullptr;
  HIPCHK(c, hipMalloc(&p, bytes));
  if (b.p) (void)hipFree(b.p);
  b.p = p;
  b.bytes = bytes;
  return ORBX_OK;
}

// the result block: one row of `cap` per pair in every per-position array
struct TpBlock {
  size_t pose, n, scale, slot_of, mask, xyz, valid, bytes;
};
TpBlock tp_block(int n_windows, int cap, int len) {
  TpBlock L;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t r = off;
    off = align_up_sz(off + bytes, 256);
    return r;
  };
  const size_t pairs = (size_t)n_windows * (len - 1), e = pairs * cap;
  L.pose = take(sizeof(OrbxPoseOut) * pairs);
  L.n = take(sizeof(int32_t) * pairs);
  L.scale = take(sizeof(OrbxScaleOut) * pairs);
  L.slot_of = take(sizeof(int32_t) * e);
  L.mask = take(e);
  L.xyz = take(sizeof(float) * 3 * e);
  L.valid = take(e);
  L.bytes = off;
  return L;
}

int tp_pairs(const orbx_ctx* c) { return c->tp.n * (c->tp.len - 1); }

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

// enqueues the four kernels on s; arguments are checked
int tp_run(orbx_ctx* c, const double* K, const float* d_tracks, const int32_t* d_seen, int n, int cap, int len,
           double prob, double threshold, int max_iters, uint64_t seed, hipStream_t s) {
  int st = c->tp.side.enter(c, s);
  if (st != ORBX_OK) return st;
  const SideWork::Mark mark{c->tp.side, s};
  // the tracks may be the windows tracker's block, written on another stream
  if (c->lkw.side.ev && c->lkw.side.stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->lkw.side.ev, 0));
  const TpBlock B = tp_block(n, cap, len);
  const int pairs = n * (len - 1);
  if ((st = tp_grow(c, c->tp.scr, sizeof(OrbxPosePt) * (size_t)pairs * cap)) != ORBX_OK) return st;
  if ((st = tp_grow(c, c->tp.blk, B.bytes)) != ORBX_OK) return st;
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

extern "C" {

int orbx_tracks_pose_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                            int n_windows, int slot_capacity, int window_len, double prob, double threshold,
                            int max_iters, uint64_t seed, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = tp_check(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, prob, threshold, max_iters);
  if (st != ORBX_OK) return st;
  return tp_run(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, prob, threshold, max_iters, seed,
                stream ? (hipStream_t)stream : c->stream);
}

int orbx_tracks_pose_results_device(orbx_ctx* c, orbx_tracks_pose_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->tp.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no tracks have been posed");
  const TpBlock B = tp_block(c->tp.n, c->tp.cap, c->tp.len);
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
  if (first < 0 || n < 0 || first > tp_pairs(c) || n > tp_pairs(c) - first)
    return fail(c, ORBX_ERR_INVALID_ARG, "pairs outside the last tracks-pose block");
  if (n == 0) return ORBX_OK;
  const int st = c->tp.side.wait(c);
  if (st != ORBX_OK) return st;
  const TpBlock B = tp_block(c->tp.n, c->tp.cap, c->tp.len);
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
  const TpBlock B = tp_block(c->tp.n, c->tp.cap, c->tp.len);
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
  hipStream_t s = c->stream;
  if ((st = c->tp.side.enter(c, s)) != ORBX_OK) return st;
  const size_t tb = sizeof(float) * 2 * (size_t)n_slots * window_len;
  const size_t o_seen = align_up_sz(tb, 256);
  {
    const SideWork::Mark mark{c->tp.side, s};
    if ((st = tp_grow(c, c->tp.stage, o_seen + sizeof(int32_t) * (size_t)n_slots)) != ORBX_OK) return st;
    HIPCHK(c, hipMemcpyAsync(c->tp.stage.p, tracks_xy, tb, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((uint8_t*)c->tp.stage.p + o_seen, seen, sizeof(int32_t) * (size_t)n_slots,
                             hipMemcpyHostToDevice, s));
  }
  const uint8_t* stage = (const uint8_t*)c->tp.stage.p;
  if ((st = tp_run(c, K, (const float*)stage, (const int32_t*)(stage + o_seen), 1, n_slots, window_len, prob,
                   threshold, max_iters, seed, s)) != ORBX_OK)
    return st;
  return orbx_tracks_pose_fetch(c, 0, window_len - 1, E, R, t, inliers, good, iters, counts, scale, triplets,
                                ratios_used);
}

}  // extern "C"
