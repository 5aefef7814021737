// orbx_api_carry.cpp -- host layer of liborbx.so (orbx_host.h) behind include/orbx_carry.h: landmarks carried from the
// current landmarks block into the next generation of windows, the PnP of every frame of those windows against them,
// the landmarks build from those poses and the one window of host arrays.  The reference
// re-detects at every solve (src/with_bundle_adjustment.cpp:586-593) and chains its poses
// (src/with_bundle_adjustment.cpp:196-208).
#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/orbx_carry.h"
#include "orbx_host.h"
#include "orbx_lm_math.h"
#include "orbx_pnp_math.h"

using namespace orbx_host;

static_assert((int)ORBX_CARRY_OK == (int)CARRY_OK && (int)ORBX_CARRY_LOST == (int)CARRY_LOST, "orbx_carry_status");
static_assert((int)ORBX_LM_OK == (int)LM_OK, "orbx_landmarks_status");

namespace {

struct PnpParams {
  double prob, threshold_px;
  int max_iters;
  uint64_t seed;
  int refine_iters, min_inliers;
};

// the argument rules of orbx_pnp_ransac; nothing is launched
int pnp_check(orbx_ctx* c, const double* K, const PnpParams& p) {
  if (!pose_args_ok(K, p.prob, p.threshold_px, p.max_iters)) return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  if (p.refine_iters < 0 || p.refine_iters > ORBX_PNP_MAX_REFINE_ITERS)
    return fail(c, ORBX_ERR_INVALID_ARG, "refine_iters outside [0, 20]");
  if (p.min_inliers < 4) return fail(c, ORBX_ERR_INVALID_ARG, "min_inliers < 4");
  return ORBX_OK;
}

int sizes_check(orbx_ctx* c, int n, int cap) {
  if (n < 1 || cap < 1) return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1 or slot_capacity < 1");
  if (cap > ORBX_BA_MAX_POINTS) return fail(c, ORBX_ERR_UNSUPPORTED, "more slots in a window than 65536");
  if ((unsigned long long)n * ((unsigned long long)cap + 1) > 0x7fffffffull)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more slots in a batch than 32-bit offsets hold");
  return ORBX_OK;
}

// the join of d_origin to the old block `in` on s, which c->carry.side has entered; arguments are checked
int carry_run(orbx_ctx* c, const OrbxCarryIn& in, const int32_t* d_origin, int n, int cap, hipStream_t s) {
  const CarryBlock B((size_t)n, (size_t)cap);
  const int st = c->carry.side.grow(c, c->carry.blk, B.bytes);
  if (st != ORBX_OK) return st;
  c->carry.n = 0;  // from here on the previous block is being replaced
  HIPCHK(c, orbx_launch_carry_join(s, in, d_origin, n, cap, at<double>(c->carry.blk, B.xyz),
                                   at<int32_t>(c->carry.blk, B.point), at<int32_t>(c->carry.blk, B.count)));
  c->carry.n = n;
  c->carry.cap = cap;
  return ORBX_OK;
}

// gather, RANSAC and fill against the carry block on s, which c->carry.side has entered; arguments are checked
int carried_pnp_run(orbx_ctx* c, const double* K, const float* d_tracks, const int32_t* d_seen, int len,
                    const PnpParams& p, hipStream_t s) {
  const int n = c->carry.n, cap = c->carry.cap;
  const CarryBlock CB((size_t)n, (size_t)cap);
  const CarryPnpBlock B((size_t)n, (size_t)cap, (size_t)len);
  const CarryPnpScratch S((size_t)n, (size_t)cap, (size_t)len);
  int st;
  if ((st = c->carry.side.grow(c, c->carry.pscr, S.bytes)) != ORBX_OK) return st;
  if ((st = c->carry.side.grow(c, c->carry.pblk, B.bytes)) != ORBX_OK) return st;
  c->carry.pn = 0;  // from here on the previous block is being replaced
  OrbxPnpCorr* corr = at<OrbxPnpCorr>(c->carry.pscr, S.corr);
  int32_t* cidx = at<int32_t>(c->carry.pscr, S.cidx);
  int32_t* ncorr = at<int32_t>(c->carry.pscr, S.ncorr);
  OrbxPnpRecord* rec = at<OrbxPnpRecord>(c->carry.pblk, B.records);
  HIPCHK(c, orbx_launch_carry_gather(s, at<const double>(c->carry.blk, CB.xyz), at<const int32_t>(c->carry.blk, CB.point),
                                     at<const int32_t>(c->carry.blk, CB.count), d_tracks, d_seen, n, cap, len, corr,
                                     cidx, ncorr));
  const double K4[4] = {K[0], K[4], K[2], K[5]};
  const OrbxPnpIn none{};
  const double prob = p.prob < 0 ? 0.0 : (p.prob > 1 ? 1.0 : p.prob);
  HIPCHK(c, orbx_launch_pnp(s, n, len, cap, none, 0, K4, prob, p.threshold_px, p.max_iters, p.seed, p.refine_iters,
                            p.min_inliers, corr, cidx, rec, nullptr, at<uint8_t>(c->carry.pblk, B.mask), ncorr));
  HIPCHK(c, orbx_launch_carry_fill(s, rec, n, len, at<double>(c->carry.pblk, B.poses6),
                                   at<int32_t>(c->carry.pblk, B.status)));
  c->carry.pn = n;
  c->carry.pcap = cap;
  c->carry.plen = len;
  return ORBX_OK;
}

int carried_check(orbx_ctx* c, const double* K, const void* tracks, const void* seen, int n, int cap, int len,
                  const PnpParams& p) {
  const int st = pnp_check(c, K, p);
  if (st != ORBX_OK) return st;
  if (!tracks || !seen) return fail(c, ORBX_ERR_INVALID_ARG, "tracks or seen is NULL");
  if (len < 2 || len > ORBX_BA_MAX_POSES) return fail(c, ORBX_ERR_INVALID_ARG, "window_len outside [2, 8]");
  if (c->carry.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks have been carried");
  if (n != c->carry.n || cap != c->carry.cap)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows or slot_capacity differs from the carry block");
  if ((unsigned long long)n * cap * len > 0x7fffffffull)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more observations in a batch than 32-bit offsets hold");
  return ORBX_OK;
}

int carry_range(orbx_ctx* c, int first, int n) {
  if (c->carry.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks have been carried");
  if (!range_ok(first, n, c->carry.n)) return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the carry block");
  return ORBX_OK;
}

int carried_range(orbx_ctx* c, int first, int n) {
  if (c->carry.pn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no carried PnP batch has run");
  if (!range_ok(first, n, c->carry.pn))
    return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the carried PnP block");
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_landmarks_carry_device(orbx_ctx* c, const int32_t* d_origin, int n_windows, int slot_capacity, int source,
                                void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!d_origin) return fail(c, ORBX_ERR_INVALID_ARG, "origin is NULL");
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  if (n_windows != c->lm.n) return fail(c, ORBX_ERR_INVALID_ARG, "n_windows differs from the landmarks block");
  int st = sizes_check(c, n_windows, slot_capacity);
  if (st != ORBX_OK) return st;
  if (source != ORBX_CARRY_BUILT && source != ORBX_CARRY_SOLVED)
    return fail(c, ORBX_ERR_INVALID_ARG, "source is neither ORBX_CARRY_BUILT nor ORBX_CARRY_SOLVED");
  if (source == ORBX_CARRY_SOLVED && !c->lm.solved)
    return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has not been solved");
  hipStream_t s = stream_of(c, stream);
  if ((st = c->carry.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->carry.side, s};
  // the block and its solve may have been written on another stream; so may the top-up's origin
  if ((st = c->carry.side.after(c, c->lm.side, s)) != ORBX_OK) return st;
  if ((st = c->carry.side.after(c, c->gf.side, s)) != ORBX_OK) return st;
  if ((st = c->carry.side.after(c, c->reloc.side, s)) != ORBX_OK) return st;  // (or the re-association's, rank 19)
  const LmBlock L((size_t)c->lm.n, (size_t)c->lm.cap, (size_t)c->lm.len);
  const LmSolve V((size_t)c->lm.n, (size_t)c->lm.cap, (size_t)c->lm.len);
  OrbxCarryIn in;
  in.status = at<const int32_t>(c->lm.blk, L.status);
  in.pt_off = at<const int32_t>(c->lm.blk, L.pt_off);
  in.slot = at<const int32_t>(c->lm.blk, L.slot);
  in.src = source == ORBX_CARRY_SOLVED ? at<const double>(c->lm.sol, V.points) : at<const double>(c->lm.blk, L.points);
  in.old_cap = c->lm.cap;
  return carry_run(c, in, d_origin, n_windows, slot_capacity, s);
}

int orbx_landmarks_carry_results_device(orbx_ctx* c, orbx_landmarks_carry_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->carry.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks have been carried");
  const CarryBlock B((size_t)c->carry.n, (size_t)c->carry.cap);
  v->xyz = at<const double>(c->carry.blk, B.xyz);
  v->point = at<const int32_t>(c->carry.blk, B.point);
  v->count = at<const int32_t>(c->carry.blk, B.count);
  v->slot_capacity = c->carry.cap;
  v->n_windows = c->carry.n;
  return ORBX_OK;
}

int orbx_landmarks_carry_fetch(orbx_ctx* c, int first, int n, double* xyz, int32_t* point, int32_t* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = carry_range(c, first, n);
  if (st != ORBX_OK) return st;
  if ((st = c->carry.side.wait(c)) != ORBX_OK) return st;
  const CarryBlock B((size_t)c->carry.n, (size_t)c->carry.cap);
  const size_t s0 = (size_t)first * c->carry.cap, ns = (size_t)n * c->carry.cap;
  if (xyz)
    HIPCHK(c, hipMemcpy(xyz, at<const double>(c->carry.blk, B.xyz) + 3 * s0, sizeof(double) * 3 * ns,
                        hipMemcpyDeviceToHost));
  if (point)
    HIPCHK(c, hipMemcpy(point, at<const int32_t>(c->carry.blk, B.point) + s0, sizeof(int32_t) * ns,
                        hipMemcpyDeviceToHost));
  if (count)
    HIPCHK(c, hipMemcpy(count, at<const int32_t>(c->carry.blk, B.count) + first, sizeof(int32_t) * n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_window_poses_pnp_carried_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                         int n_windows, int slot_capacity, int window_len, double prob,
                                         double threshold_px, int max_iters, uint64_t seed, int refine_iters,
                                         int min_inliers, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const PnpParams p{prob, threshold_px, max_iters, seed, refine_iters, min_inliers};
  int st = carried_check(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, p);
  if (st != ORBX_OK) return st;
  hipStream_t s = stream_of(c, stream);
  // (the carry ran under the same event: on another stream it has finished once enter() returns)
  if ((st = c->carry.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->carry.side, s};
  // the tracks may be the windows tracker's block, written on another stream; a carried build may still be reading
  // the last poses
  if ((st = c->carry.side.after(c, c->lkw.side, s)) != ORBX_OK) return st;
  if ((st = c->carry.side.after(c, c->lm.side, s)) != ORBX_OK) return st;
  return carried_pnp_run(c, K, d_tracks_xy, d_seen, window_len, p, s);
}

int orbx_window_poses_pnp_carried_results_device(orbx_ctx* c, orbx_window_poses_carried_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  if (c->carry.pn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no carried PnP batch has run");
  const CarryPnpBlock B((size_t)c->carry.pn, (size_t)c->carry.pcap, (size_t)c->carry.plen);
  v->records = at<const orbx_pnp_record>(c->carry.pblk, B.records);
  v->poses6 = at<const double>(c->carry.pblk, B.poses6);
  v->mask = at<const uint8_t>(c->carry.pblk, B.mask);
  v->window_status = at<const int32_t>(c->carry.pblk, B.status);
  v->slot_capacity = c->carry.pcap;
  v->window_len = c->carry.plen;
  v->n_windows = c->carry.pn;
  return ORBX_OK;
}

int orbx_window_poses_pnp_carried_fetch(orbx_ctx* c, int first, int n, orbx_pnp_record* records, double* poses6,
                                        int32_t* window_status) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = carried_range(c, first, n);
  if (st != ORBX_OK) return st;
  if ((st = c->carry.side.wait(c)) != ORBX_OK) return st;
  const CarryPnpBlock B((size_t)c->carry.pn, (size_t)c->carry.pcap, (size_t)c->carry.plen);
  const size_t len = (size_t)c->carry.plen;
  if (records)
    HIPCHK(c, hipMemcpy(records, at<const OrbxPnpRecord>(c->carry.pblk, B.records) + len * first,
                        sizeof(OrbxPnpRecord) * len * n, hipMemcpyDeviceToHost));
  if (poses6)
    HIPCHK(c, hipMemcpy(poses6, at<const double>(c->carry.pblk, B.poses6) + 6 * len * first,
                        sizeof(double) * 6 * len * n, hipMemcpyDeviceToHost));
  if (window_status)
    HIPCHK(c, hipMemcpy(window_status, at<const int32_t>(c->carry.pblk, B.status) + first, sizeof(int32_t) * n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_window_poses_pnp_carried_mask_fetch(orbx_ctx* c, int window, int k, uint8_t* mask, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = carried_range(c, window, 1);
  if (st != ORBX_OK) return st;
  if (k < 0 || k >= c->carry.plen) return fail(c, ORBX_ERR_INVALID_ARG, "k outside [0, window_len)");
  if (capacity < 0) return fail(c, ORBX_ERR_INVALID_ARG, "a capacity is negative");
  if (count) *count = c->carry.pcap;
  if (mask && c->carry.pcap > capacity) return fail(c, ORBX_ERR_CAPACITY, "carried PnP mask fetch: capacity is too small");
  if ((st = c->carry.side.wait(c)) != ORBX_OK) return st;
  const CarryPnpBlock B((size_t)c->carry.pn, (size_t)c->carry.pcap, (size_t)c->carry.plen);
  const size_t row = ((size_t)window * c->carry.plen + k) * c->carry.pcap;
  if (mask)
    HIPCHK(c, hipMemcpy(mask, at<const uint8_t>(c->carry.pblk, B.mask) + row, (size_t)c->carry.pcap,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_landmarks_build_carried_device(orbx_ctx* c, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                        int n_windows, int slot_capacity, int window_len, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const int st = lm_check_build(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, nullptr);
  if (st != ORBX_OK) return st;
  if (c->carry.pn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no carried PnP batch has run");
  if (n_windows != c->carry.pn || window_len != c->carry.plen)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_windows or window_len differs from the carried PnP block");
  const CarryPnpBlock B((size_t)c->carry.pn, (size_t)c->carry.pcap, (size_t)c->carry.plen);
  return lm_run(c, K, d_tracks_xy, d_seen, n_windows, slot_capacity, window_len, nullptr,
                at<const double>(c->carry.pblk, B.poses6), at<const int32_t>(c->carry.pblk, B.status),
                stream_of(c, stream), nullptr, &c->carry.side);
}

int orbx_localise_carried_window(orbx_ctx* c, const double* old_points3, const int32_t* old_slot_of_point, int n_old,
                                 const int32_t* origin, const float* tracks_xy, const int32_t* seen, int n_slots,
                                 int window_len, const double* K, double prob, double threshold_px, int max_iters,
                                 uint64_t seed, int refine_iters, int min_inliers, orbx_pnp_record* records,
                                 double* poses6, int32_t* window_status, int32_t* carried_point) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const PnpParams p{prob, threshold_px, max_iters, seed, refine_iters, min_inliers};
  int st = pnp_check(c, K, p);
  if (st != ORBX_OK) return st;
  if (n_old < 0 || (n_old > 0 && (!old_points3 || !old_slot_of_point)) || !origin || !tracks_xy || !seen)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_old < 0, or a NULL array");
  if (window_len < 2 || window_len > ORBX_BA_MAX_POSES)
    return fail(c, ORBX_ERR_INVALID_ARG, "window_len outside [2, 8]");
  if ((st = sizes_check(c, 1, n_slots)) != ORBX_OK) return st;
  if (n_old > ORBX_BA_MAX_POINTS) return fail(c, ORBX_ERR_UNSUPPORTED, "more landmarks in a window than 65536");
  hipStream_t s = c->stream;
  if ((st = c->carry.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->carry.side, s};
  if ((st = c->carry.side.after(c, c->lm.side, s)) != ORBX_OK) return st;  // (a carried build may read the last poses)
  const CarryStage G((size_t)n_old, (size_t)n_slots, (size_t)window_len);
  if ((st = c->carry.side.grow(c, c->carry.stage, G.bytes)) != ORBX_OK) return st;
  const int32_t head[3] = {LM_OK, 0, n_old};
  uint8_t* g = (uint8_t*)c->carry.stage.p;
  HIPCHK(c, hipMemcpyAsync(g + G.status, &head[0], sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(g + G.pt_off, &head[1], sizeof(int32_t) * 2, hipMemcpyHostToDevice, s));
  if (n_old > 0) {
    HIPCHK(c, hipMemcpyAsync(g + G.slot, old_slot_of_point, sizeof(int32_t) * (size_t)n_old, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(g + G.points, old_points3, sizeof(double) * 3 * (size_t)n_old, hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, hipMemcpyAsync(g + G.origin, origin, sizeof(int32_t) * (size_t)n_slots, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(g + G.seen, seen, sizeof(int32_t) * (size_t)n_slots, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(g + G.tracks, tracks_xy, sizeof(float) * 2 * (size_t)n_slots * window_len,
                           hipMemcpyHostToDevice, s));
  OrbxCarryIn in;
  in.status = (const int32_t*)(g + G.status);
  in.pt_off = (const int32_t*)(g + G.pt_off);
  in.slot = (const int32_t*)(g + G.slot);
  in.src = (const double*)(g + G.points);
  in.old_cap = INT_MAX;
  if ((st = carry_run(c, in, (const int32_t*)(g + G.origin), 1, n_slots, s)) != ORBX_OK) return st;
  if ((st = carried_pnp_run(c, K, (const float*)(g + G.tracks), (const int32_t*)(g + G.seen), window_len, p, s)) !=
      ORBX_OK)
    return st;
  HIPCHK(c, hipStreamSynchronize(s));  // (also: the host arrays have been read)
  const CarryBlock CB(1, (size_t)n_slots);
  const CarryPnpBlock B(1, (size_t)n_slots, (size_t)window_len);
  if (records)
    HIPCHK(c, hipMemcpy(records, at<const OrbxPnpRecord>(c->carry.pblk, B.records),
                        sizeof(OrbxPnpRecord) * (size_t)window_len, hipMemcpyDeviceToHost));
  if (poses6)
    HIPCHK(c, hipMemcpy(poses6, at<const double>(c->carry.pblk, B.poses6), sizeof(double) * 6 * (size_t)window_len,
                        hipMemcpyDeviceToHost));
  if (window_status)
    HIPCHK(c, hipMemcpy(window_status, at<const int32_t>(c->carry.pblk, B.status), sizeof(int32_t),
                        hipMemcpyDeviceToHost));
  if (carried_point)
    HIPCHK(c, hipMemcpy(carried_point, at<const int32_t>(c->carry.blk, CB.point), sizeof(int32_t) * (size_t)n_slots,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

}  // extern "C"
