// orbx_api_geom.cpp -- host layer of liborbx.so (orbx_host.h): relative pose, triangulation / scale / trajectory
// chaining, and bundle adjustment.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "orbx_host.h"
#include "orbx_tri_math.h"

using namespace orbx_host;

// ---- relative pose (next row) ---------------------------

extern "C" {

int orbx_estimate_pose(orbx_ctx* c, const float* pts1_xy, const float* pts2_xy, int n, const double* K, double prob,
                       double threshold, int max_iters, uint64_t seed, double* E, double* R, double* t, uint8_t* mask,
                       int32_t* inliers, int32_t* good, int32_t* iters) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!pts1_xy || !pts2_xy)) || !E || !R || !t || !inliers || !good || !iters ||
      !pose_args_ok(K, prob, threshold, max_iters))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  const int cap = n > 0 ? n : 1;
  const PoseBlock L(1, cap);
  DevBuf& b = c->pose.hblk;
  ENSURE(c, c->pose.hin, sizeof(float) * 4 * (size_t)cap);
  ENSURE(c, b, L.bytes);
  hipStream_t s = c->stream;
  float* d_p1 = (float*)c->pose.hin.p;
  float* d_p2 = d_p1 + 2 * (size_t)cap;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(d_p1, pts1_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_p2, pts2_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, orbx_launch_pose_prep_host(s, n, d_p1, d_p2, K, at<OrbxPosePt>(b, L.pts), at<int32_t>(b, L.n)));
  HIPCHK(c, orbx_launch_pose_ransac(s, 1, cap, at<OrbxPosePt>(b, L.pts), at<int32_t>(b, L.n), K, prob, threshold,
                                    max_iters, seed, at<OrbxPoseOut>(b, L.out), at<uint8_t>(b, L.mask)));
  OrbxPoseOut r;
  HIPCHK(c, hipMemcpyAsync(&r, at<OrbxPoseOut>(b, L.out), sizeof r, hipMemcpyDeviceToHost, s));
  if (mask && n > 0) HIPCHK(c, hipMemcpyAsync(mask, at<uint8_t>(b, L.mask), (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  pose_unpack(r, E, R, t, inliers, good, iters);
  return ORBX_OK;
}

int orbx_batch_pose_consecutive(orbx_ctx* c, const double* K, double prob, double threshold, int max_iters,
                                uint64_t seed) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!pose_args_ok(K, prob, threshold, max_iters)) return fail(c, ORBX_ERR_INVALID_ARG, "bad pose arguments");
  if (c->m.pairs <= 0 || c->m.serial != c->batch_serial)
    return fail(c, ORBX_ERR_INVALID_ARG, "the last batch has not been matched (orbx_batch_match_consecutive)");
  // the pose block is ONE per context, like the matcher's
  if (c->lanes[1].stream) HIPCHK(c, lanes_sync(c));
  const Block& B = last_block(c);
  const int npairs = c->m.pairs, cap = B.cap;
  const PoseBlock L(npairs, cap);
  DevBuf& b = c->pose.blk;
  ENSURE(c, b, L.bytes);
  const OutLayout& o = B.layout;
  hipStream_t s = batch_stream(c);
  HIPCHK(c, orbx_launch_pose_prep_batch(s, npairs, cap, (const int32_t*)(B.d + o.counts),
                                        (const orbx_keypoint*)(B.d + o.kp),
                                        at<int32_t>(c->m.res, MatchBlock(npairs, cap).match), K,
                                        at<OrbxPosePt>(b, L.pts), at<int32_t>(b, L.n)));
  HIPCHK(c, orbx_launch_pose_ransac(s, npairs, cap, at<OrbxPosePt>(b, L.pts), at<int32_t>(b, L.n), K, prob, threshold,
                                    max_iters, seed, at<OrbxPoseOut>(b, L.out), at<uint8_t>(b, L.mask)));
  c->pose.pairs = npairs;
  c->pose.cap = cap;
  c->pose.stream = s;
  c->pose.serial = c->batch_serial;
  c->pose.match_gen = c->m.gen;
  return ORBX_OK;
}

int orbx_batch_pose_fetch(orbx_ctx* c, int first, int n, double* E, double* R, double* t, int32_t* inliers,
                          int32_t* good, int32_t* iters) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->pose.pairs <= 0) return fail(c, ORBX_ERR_INVALID_ARG, "no batch has been posed");
  if (first < 0 || n < 0 || first + n > c->pose.pairs)
    return fail(c, ORBX_ERR_INVALID_ARG, "pairs outside the last posed batch");
  if (n == 0) return ORBX_OK;
  std::vector<OrbxPoseOut> r((size_t)n);
  const PoseBlock L(c->pose.pairs, c->pose.cap);
  HIPCHK(c, hipMemcpyAsync(r.data(), at<OrbxPoseOut>(c->pose.blk, L.out) + first, sizeof(OrbxPoseOut) * (size_t)n,
                           hipMemcpyDeviceToHost, c->pose.stream));
  HIPCHK(c, hipStreamSynchronize(c->pose.stream));
  for (int i = 0; i < n; i++)
    pose_unpack(r[(size_t)i], E ? E + 9 * i : nullptr, R ? R + 9 * i : nullptr, t ? t + 3 * i : nullptr,
                inliers ? inliers + i : nullptr, good ? good + i : nullptr, iters ? iters + i : nullptr);
  return ORBX_OK;
}

int orbx_batch_pose_mask(orbx_ctx* c, int pair, uint8_t* mask, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count || capacity < 0 || (capacity > 0 && !mask)) return fail(c, ORBX_ERR_INVALID_ARG, "bad mask arguments");
  if (pair < 0 || pair >= c->pose.pairs) return fail(c, ORBX_ERR_INVALID_ARG, "pair outside the last posed batch");
  const PoseBlock L(c->pose.pairs, c->pose.cap);
  int32_t np = 0;
  HIPCHK(c, hipMemcpyAsync(&np, at<int32_t>(c->pose.blk, L.n) + pair, sizeof np, hipMemcpyDeviceToHost, c->pose.stream));
  HIPCHK(c, hipStreamSynchronize(c->pose.stream));
  *count = np;
  if (np > capacity) return fail(c, ORBX_ERR_CAPACITY, "capacity smaller than the pair's match count");
  if (np > 0) {
    HIPCHK(c, hipMemcpyAsync(mask, at<uint8_t>(c->pose.blk, L.mask) + (size_t)pair * c->pose.cap, (size_t)np,
                             hipMemcpyDeviceToHost, c->pose.stream));
    HIPCHK(c, hipStreamSynchronize(c->pose.stream));
  }
  return ORBX_OK;
}

}  // extern "C"

// ---- triangulation, relative scale, trajectory chaining ------------

extern "C" {

int orbx_triangulate(orbx_ctx* c, const float* pts1_xy, const float* pts2_xy, int n, const double* K, const double* R,
                     const double* t, float* xyz, uint8_t* valid) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!pts1_xy || !pts2_xy || !xyz || !valid)) || !K || !R || !t || !finite_all(K, 9) ||
      !finite_all(R, 9) || !finite_all(t, 3))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad triangulation arguments");
  if (n == 0) return ORBX_OK;
  const TriHost L(n);
  DevBuf& b = c->scale.host;
  ENSURE(c, b, L.bytes);
  hipStream_t s = c->stream;
  float* d_p1 = at<float>(b, L.in);
  float* d_p2 = d_p1 + 2 * (size_t)n;
  HIPCHK(c, hipMemcpyAsync(d_p1, pts1_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_p2, pts2_xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  HIPCHK(c, orbx_launch_triangulate_host(s, n, d_p1, d_p2, K, R, t, at<float>(b, L.xyz), at<uint8_t>(b, L.valid)));
  HIPCHK(c, hipMemcpyAsync(xyz, at<float>(b, L.xyz), sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(valid, at<uint8_t>(b, L.valid), (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return ORBX_OK;
}

int orbx_estimate_scale(orbx_ctx* c, const float* prev_xyz, const uint8_t* prev_valid, int n_prev, const float* cur_xyz,
                        const uint8_t* cur_valid, int n_cur, double* scale, int32_t* ratios_used) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n_prev < 0 || n_cur < 0 || (n_prev > 0 && !prev_xyz) || (n_cur > 0 && !cur_xyz) || !scale || !ratios_used)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad scale arguments");
  const int m = std::min(n_prev, n_cur);
  if (m == 0) {  // src/feature_matching.cpp:248-249
    *scale = 1.0;
    *ratios_used = 0;
    return ORBX_OK;
  }
  if ((size_t)m * 8 > ORBX_SCALE_LDS_MAX)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more aligned points than the selection holds in LDS");
  // only the first m points of either list enter
  const ScaleHost L(m);
  DevBuf& b = c->scale.host;
  ENSURE(c, b, L.bytes);
  hipStream_t s = c->stream;
  float* d_prev = at<float>(b, L.xyz);
  float* d_cur = d_prev + 3 * (size_t)m;
  uint8_t* d_pv = at<uint8_t>(b, L.valid);
  uint8_t* d_cv = d_pv + m;
  HIPCHK(c, hipMemcpyAsync(d_prev, prev_xyz, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_cur, cur_xyz, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, s));
  if (prev_valid) HIPCHK(c, hipMemcpyAsync(d_pv, prev_valid, (size_t)m, hipMemcpyHostToDevice, s));
  if (cur_valid) HIPCHK(c, hipMemcpyAsync(d_cv, cur_valid, (size_t)m, hipMemcpyHostToDevice, s));
  HIPCHK(c, orbx_launch_scale_aligned(s, m, m, d_prev, prev_valid ? d_pv : nullptr, d_cur, cur_valid ? d_cv : nullptr,
                                      at<OrbxScaleOut>(b, L.out)));
  OrbxScaleOut r;
  HIPCHK(c, hipMemcpyAsync(&r, at<OrbxScaleOut>(b, L.out), sizeof r, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  *scale = r.scale;
  *ratios_used = r.ratios_used;
  return ORBX_OK;
}

int orbx_batch_scale_consecutive(orbx_ctx* c, const double* K) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!K || !finite_all(K, 9)) return fail(c, ORBX_ERR_INVALID_ARG, "bad scale arguments");
  if (c->pose.pairs <= 0 || c->pose.serial != c->batch_serial)
    return fail(c, ORBX_ERR_INVALID_ARG, "the last batch has not been posed (orbx_batch_pose_consecutive)");
  // the triangulation reads the match table again: it must still hold the matches the poses were computed from
  // (a host-array matcher call writes the same block and zeroes m.pairs; a second batch match bumps m.gen)
  if (c->m.pairs != c->pose.pairs || c->m.serial != c->batch_serial || c->pose.match_gen != c->m.gen)
    return fail(c, ORBX_ERR_INVALID_ARG, "the match table has been rewritten since the batch was posed");
  const int npairs = c->pose.pairs, cap = c->pose.cap;
  if ((size_t)cap * 16 > ORBX_SCALE_LDS_MAX)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more result slots per frame than the join holds in LDS");
  // the scale block is ONE per context, like the pose block
  if (c->lanes[1].stream) HIPCHK(c, lanes_sync(c));
  const ScaleBlock L(npairs, cap);
  DevBuf& b = c->scale.blk;
  ENSURE(c, b, L.bytes);
  const Block& B = last_block(c);
  const OutLayout& o = B.layout;
  hipStream_t s = c->pose.stream;
  const OrbxPoseOut* d_pose = at<OrbxPoseOut>(c->pose.blk, PoseBlock(npairs, cap).out);
  HIPCHK(c, orbx_launch_triangulate_batch(s, npairs, cap, (const int32_t*)(B.d + o.counts),
                                          (const orbx_keypoint*)(B.d + o.kp),
                                          at<int32_t>(c->m.res, MatchBlock(npairs, cap).match), d_pose, K,
                                          at<float>(b, L.xyz), at<uint8_t>(b, L.valid), at<int32_t>(b, L.mq),
                                          at<int32_t>(b, L.mt), at<int32_t>(b, L.n)));
  HIPCHK(c, orbx_launch_scale_join(s, npairs, npairs, cap, at<int32_t>(b, L.n), at<int32_t>(b, L.mq),
                                   at<int32_t>(b, L.mt), at<float>(b, L.xyz), at<uint8_t>(b, L.valid), d_pose,
                                   at<OrbxScaleOut>(b, L.out)));
  c->scale.pairs = npairs;
  c->scale.cap = cap;
  c->scale.stream = s;
  return ORBX_OK;
}

int orbx_batch_scale_fetch(orbx_ctx* c, int first, int n, double* scale, int32_t* triplets, int32_t* ratios_used) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (c->scale.pairs <= 0) return fail(c, ORBX_ERR_INVALID_ARG, "no batch has been scaled");
  if (first < 0 || n < 0 || first + n > c->scale.pairs)
    return fail(c, ORBX_ERR_INVALID_ARG, "pairs outside the last scaled batch");
  if (n == 0) return ORBX_OK;
  std::vector<OrbxScaleOut> r((size_t)n);
  const ScaleBlock L(c->scale.pairs, c->scale.cap);
  HIPCHK(c, hipMemcpyAsync(r.data(), at<OrbxScaleOut>(c->scale.blk, L.out) + first, sizeof(OrbxScaleOut) * (size_t)n,
                           hipMemcpyDeviceToHost, c->scale.stream));
  HIPCHK(c, hipStreamSynchronize(c->scale.stream));
  for (int i = 0; i < n; i++) {
    if (scale) scale[i] = r[(size_t)i].scale;
    if (triplets) triplets[i] = r[(size_t)i].triplets;
    if (ratios_used) ratios_used[i] = r[(size_t)i].ratios_used;
  }
  return ORBX_OK;
}

int orbx_batch_points_fetch(orbx_ctx* c, int pair, float* xyz, uint8_t* valid, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count || capacity < 0 || (capacity > 0 && (!xyz || !valid)))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad point output arguments");
  if (pair < 0 || pair >= c->scale.pairs) return fail(c, ORBX_ERR_INVALID_ARG, "pair outside the last scaled batch");
  hipStream_t s = c->scale.stream;
  const ScaleBlock L(c->scale.pairs, c->scale.cap);
  int32_t np = 0;
  HIPCHK(c, hipMemcpyAsync(&np, at<int32_t>(c->scale.blk, L.n) + pair, sizeof np, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  *count = np;
  if (np > capacity) return fail(c, ORBX_ERR_CAPACITY, "capacity smaller than the pair's match count");
  if (np > 0) {
    const size_t row = (size_t)pair * c->scale.cap;
    HIPCHK(c, hipMemcpyAsync(xyz, at<float>(c->scale.blk, L.xyz) + 3 * row, sizeof(float) * 3 * (size_t)np,
                             hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(valid, at<uint8_t>(c->scale.blk, L.valid) + row, (size_t)np, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return ORBX_OK;
}

int orbx_chain_trajectory(const double* T0, const double* R, const double* t, const double* scale, int n,
                          double* poses) {
  if (!T0 || !poses || n < 0 || (n > 0 && (!R || !t || !scale))) return ORBX_ERR_INVALID_ARG;
  std::memcpy(poses, T0, sizeof(double) * 16);
  for (int i = 0; i < n; i++) tri_chain(poses + 16 * i, R + 9 * i, t + 3 * i, scale[i], poses + 16 * (i + 1));
  return ORBX_OK;
}

}  // extern "C"

// ---- bundle adjustment -----------------------------------------------

static_assert(sizeof(orbx_ba_summary) == 32, "orbx_ba_summary is the kernel's BaSummary");

namespace orbx_host {

// orbx_bundle_adjust_batch, and with `prior` its twin with landmark priors (orbx_api_prior.cpp, rank 20): the same
// checks, staging and workspaces; the priors go up beside the stage as [points][4] and the solve is k_ba_lm<true>
int ba_batch(orbx_ctx* c, const double* K, int n_windows, const int32_t* pose_offset, double* poses6,
             const int32_t* point_offset, double* points3, const int32_t* obs_offset, const int32_t* obs_point,
             const int32_t* obs_pose, const double* obs_xy, double huber_delta, int max_iters,
             orbx_ba_summary* summaries, const BaPriorArgs* prior) {
  if (!K || !finite_all(K, 9) || n_windows < 0 || !(huber_delta > 0.0) || !std::isfinite(huber_delta) ||
      max_iters < 1 || max_iters > 1000)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  if (n_windows == 0) return ORBX_OK;
  if (!pose_offset || !poses6 || !point_offset || !points3 || !obs_offset || !obs_point || !obs_pose || !obs_xy ||
      !summaries)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  if (pose_offset[0] != 0 || point_offset[0] != 0 || obs_offset[0] != 0)
    return fail(c, ORBX_ERR_INVALID_ARG, "offset arrays start at 0");
  int cap = 1, ocap = 1;
  for (int w = 0; w < n_windows; w++) {
    const long long W = (long long)pose_offset[w + 1] - pose_offset[w], N = (long long)point_offset[w + 1] - point_offset[w],
                    M = (long long)obs_offset[w + 1] - obs_offset[w];
    if (W < 2 || W > ORBX_BA_MAX_POSES) return fail(c, ORBX_ERR_INVALID_ARG, "a window has 2 .. 8 poses");
    if (N < 1 || M < N || M > N * W)
      return fail(c, ORBX_ERR_INVALID_ARG, "every landmark has 1 .. n_poses observations");
    if (N > ORBX_BA_MAX_POINTS) return fail(c, ORBX_ERR_UNSUPPORTED, "more landmarks in a window than 65536");
    cap = std::max(cap, (int)N);
    ocap = std::max(ocap, (int)M);
  }
  const size_t tp = (size_t)pose_offset[n_windows], tn = (size_t)point_offset[n_windows], tm = (size_t)obs_offset[n_windows];
  if (tn + (size_t)n_windows > 0x7fffffffu || tm > 0x7fffffffu)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more landmarks or observations in a batch than 32-bit offsets hold");
  if (!finite_all(poses6, (int)(6 * tp))) return fail(c, ORBX_ERR_INVALID_ARG, "a pose is not finite");
  for (size_t i = 0; i < 3 * tn; i++)
    if (!std::isfinite(points3[i])) return fail(c, ORBX_ERR_INVALID_ARG, "a point is not finite");
  for (size_t i = 0; i < 2 * tm; i++)
    if (!std::isfinite(obs_xy[i])) return fail(c, ORBX_ERR_INVALID_ARG, "an observation is not finite");
  std::vector<double> prior4;  // rule P1: anchor and weight per landmark; no arrays: every weight is 0
  if (prior) {
    prior4.assign(4 * tn, 0.0);
    for (size_t j = 0; prior->xyz && j < tn; j++) {
      const double lam = prior->weight[j];
      const double* A = prior->xyz + 3 * j;
      if (!(lam >= 0.0) || !std::isfinite(lam)) return fail(c, ORBX_ERR_INVALID_ARG, "a prior weight is negative or not finite");
      if (lam > 0.0 && !finite_all(A, 3))
        return fail(c, ORBX_ERR_INVALID_ARG, "an anchor under a positive weight is not finite");
      prior4[4 * j] = A[0], prior4[4 * j + 1] = A[1], prior4[4 * j + 2] = A[2], prior4[4 * j + 3] = lam;
    }
  }
  // CSR by (landmark, pose), per window (src/with_bundle_adjustment.cpp:651-666 adds the residual blocks landmark by
  // landmark)
  std::vector<int32_t> rows(tn + (size_t)n_windows), order;
  std::vector<uint8_t> opose(tm);
  std::vector<double> oxy(2 * tm);
  for (int w = 0; w < n_windows; w++) {
    const int W = pose_offset[w + 1] - pose_offset[w], N = point_offset[w + 1] - point_offset[w];
    const int M = obs_offset[w + 1] - obs_offset[w];
    const int32_t* op = obs_point + obs_offset[w];
    const int32_t* oq = obs_pose + obs_offset[w];
    for (int k = 0; k < M; k++)
      if (op[k] < 0 || op[k] >= N || oq[k] < 0 || oq[k] >= W)
        return fail(c, ORBX_ERR_INVALID_ARG, "an observation's landmark or pose index is out of range");
    // every (landmark, pose) occurs at most once, so placing observation k at key landmark * W + pose and reading
    // the keys in ascending order IS the stable sort by (landmark, pose)
    order.assign((size_t)N * W, -1);
    for (int k = 0; k < M; k++) {
      int32_t& at = order[(size_t)op[k] * W + oq[k]];
      if (at >= 0) return fail(c, ORBX_ERR_INVALID_ARG, "a landmark is observed twice by one pose");
      at = k;
    }
    int32_t* row = rows.data() + point_offset[w] + w;
    std::fill(row, row + N + 1, 0);
    size_t dst = (size_t)obs_offset[w];
    for (size_t key = 0; key < order.size(); key++) {
      const int o = order[key];
      if (o < 0) continue;
      row[op[o] + 1]++;
      opose[dst] = (uint8_t)oq[o];
      oxy[2 * dst] = obs_xy[2 * ((size_t)obs_offset[w] + o)];
      oxy[2 * dst + 1] = obs_xy[2 * ((size_t)obs_offset[w] + o) + 1];
      dst++;
    }
    for (int j = 0; j < N; j++) {
      if (row[j + 1] == 0) return fail(c, ORBX_ERR_INVALID_ARG, "a landmark has no observation");
      row[j + 1] += row[j];
    }
  }
  const BaStage L(n_windows, tp, tn, tm);
  const LmWork W(n_windows, (size_t)cap, (size_t)ocap);
  DevBuf &b = c->ba.stage, &ws = c->ba.ws;
  ENSURE(c, b, L.bytes);
  ENSURE(c, ws, W.bytes);
  if (prior) ENSURE(c, c->ba.prior, sizeof(double) * prior4.size());
  hipStream_t s = c->stream;
  const size_t noff = (size_t)n_windows + 1;
  int32_t* d_off = at<int32_t>(b, L.off);
  HIPCHK(c, hipMemcpyAsync(d_off, pose_offset, sizeof(int32_t) * noff, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_off + noff, point_offset, sizeof(int32_t) * noff, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d_off + 2 * noff, obs_offset, sizeof(int32_t) * noff, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(at<double>(b, L.poses), poses6, sizeof(double) * 6 * tp, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(at<double>(b, L.points), points3, sizeof(double) * 3 * tn, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(at<int32_t>(b, L.rows), rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(at<uint8_t>(b, L.opose), opose.data(), tm, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(at<double>(b, L.oxy), oxy.data(), sizeof(double) * 2 * tm, hipMemcpyHostToDevice, s));
  const double K4[4] = {K[0], K[4], K[2], K[5]};
  if (prior) {
    HIPCHK(c, hipMemcpyAsync(c->ba.prior.p, prior4.data(), sizeof(double) * prior4.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, orbx_launch_ba_prior(s, n_windows, W.groups, max_iters, K4, huber_delta, d_off, d_off + noff,
                                   d_off + 2 * noff, at<double>(b, L.poses), at<double>(b, L.points),
                                   at<int32_t>(b, L.rows), at<uint8_t>(b, L.opose), at<double>(b, L.oxy), cap, ocap,
                                   at<double>(ws, W.wp), at<double>(ws, W.wo), at<unsigned long long>(ws, W.slot),
                                   at<void>(b, L.out), at<const double>(c->ba.prior, 0), prior->start));
  } else {
    HIPCHK(c, orbx_launch_ba(s, n_windows, W.groups, max_iters, K4, huber_delta, d_off, d_off + noff, d_off + 2 * noff,
                             at<double>(b, L.poses), at<double>(b, L.points), at<int32_t>(b, L.rows),
                             at<uint8_t>(b, L.opose), at<double>(b, L.oxy), cap, ocap, at<double>(ws, W.wp),
                             at<double>(ws, W.wo), at<unsigned long long>(ws, W.slot), at<void>(b, L.out)));
  }
  // the staged vectors are pageable: their copies above have left the host before the calls returned
  HIPCHK(c, hipMemcpyAsync(poses6, at<double>(b, L.poses), sizeof(double) * 6 * tp, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(points3, at<double>(b, L.points), sizeof(double) * 3 * tn, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(summaries, at<void>(b, L.out), sizeof(orbx_ba_summary) * (size_t)n_windows, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return ORBX_OK;
}

}  // namespace orbx_host

extern "C" {

int orbx_bundle_adjust_batch(orbx_ctx* c, const double* K, int n_windows, const int32_t* pose_offset, double* poses6,
                             const int32_t* point_offset, double* points3, const int32_t* obs_offset,
                             const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                             double huber_delta, int max_iters, orbx_ba_summary* summaries) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return ba_batch(c, K, n_windows, pose_offset, poses6, point_offset, points3, obs_offset, obs_point, obs_pose, obs_xy,
                  huber_delta, max_iters, summaries, nullptr);
}

int orbx_bundle_adjust(orbx_ctx* c, const double* K, int n_poses, double* poses6, int n_points, double* points3,
                       int n_obs, const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                       double huber_delta, int max_iters, orbx_ba_summary* summary) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n_poses < 0 || n_points < 0 || n_obs < 0) return fail(c, ORBX_ERR_INVALID_ARG, "bad bundle-adjustment arguments");
  const int32_t po[2] = {0, n_poses}, pt[2] = {0, n_points}, ob[2] = {0, n_obs};
  return orbx_bundle_adjust_batch(c, K, 1, po, poses6, pt, points3, ob, obs_point, obs_pose, obs_xy, huber_delta,
                                  max_iters, summary);
}

}  // extern "C"
