// orbx_api_search.cpp -- host layer of liborbx.so (orbx_host.h) behind include/orbx_search.h: the landmarks of the
// current block projected into a predicted view, and the re-association of two described sets inside a position gate
// (DESIGN.md §9 rank 21).  The reference keeps no point across a solve (src/with_bundle_adjustment.cpp:586-593) and
// matches two ORB sets without geometry (src/feature_tracking.cpp:203-219).
#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/orbx_search.h"
#include "orbx_host.h"
#include "orbx_lm_math.h"
#include "orbx_search_math.h"

using namespace orbx_host;

static_assert((int)ORBX_PROJ_NONE == (int)SP_NONE && (int)ORBX_PROJ_BEHIND == (int)SP_BEHIND &&
                  (int)ORBX_PROJ_OUTSIDE == (int)SP_OUTSIDE && (int)ORBX_PROJ_OK == (int)SP_OK,
              "orbx_proj_state");
static_assert(ORBX_PROJ_NONE == 0, "a cleared block is all ORBX_PROJ_NONE");

namespace {

struct ProjParams {
  const double* K;
  int width, height;
  double margin_px;
};

int proj_check_params(orbx_ctx* c, const ProjParams& p) {
  if (!p.K) return fail(c, ORBX_ERR_INVALID_ARG, "K is NULL");
  if (!(p.K[0] > 0 && p.K[4] > 0) || !std::isfinite(p.K[0]) || !std::isfinite(p.K[4]) || !std::isfinite(p.K[2]) ||
      !std::isfinite(p.K[5]))
    return fail(c, ORBX_ERR_INVALID_ARG, "K: focal lengths not positive, or an entry that is not finite");
  if (p.width < 1 || p.height < 1) return fail(c, ORBX_ERR_INVALID_ARG, "width or height < 1");
  if (!(p.margin_px >= 0.0) || !std::isfinite(p.margin_px))
    return fail(c, ORBX_ERR_INVALID_ARG, "margin_px is negative or not finite");
  return ORBX_OK;
}

// the projection of the old block `in` on s, which c->search.side has entered; arguments are checked
int proj_run(orbx_ctx* c, const OrbxCarryIn& in, int n, int cap, const double* d_pose6, size_t pose_stride,
             const ProjParams& p, hipStream_t s) {
  Search& r = c->search;
  const SpBlock B((size_t)n, (size_t)cap);
  const int st = r.side.grow(c, r.blk, B.bytes);
  if (st != ORBX_OK) return st;
  r.n = 0;  // from here on the previous block is being replaced
  const double K4[4] = {p.K[0], p.K[4], p.K[2], p.K[5]};
  HIPCHK(c, orbx_launch_sp_project(s, in, n, cap, d_pose6, pose_stride, K4, p.width, p.height, p.margin_px,
                                   at<double>(r.blk, B.xy), at<double>(r.blk, B.depth), at<int32_t>(r.blk, B.state),
                                   at<int32_t>(r.blk, B.count)));
  r.n = n;
  r.cap = cap;
  return ORBX_OK;
}

int proj_range(orbx_ctx* c, int first, int n) {
  if (c->search.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks have been projected");
  if (!range_ok(first, n, c->search.n)) return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the projection");
  return ORBX_OK;
}

struct GateParams {
  double radius_px, ratio;
  int max_distance, accept_lone, unique;
};

// the parameter rules of orbx_reassociate_device, then the gate's own
int gate_check_params(orbx_ctx* c, const GateParams& p) {
  if (!std::isfinite(p.ratio) || p.ratio < 0.0) return fail(c, ORBX_ERR_INVALID_ARG, "ratio must be finite, >= 0");
  if (p.max_distance < 0 || p.max_distance > 256) return fail(c, ORBX_ERR_INVALID_ARG, "max_distance outside [0, 256]");
  if (p.unique != 0 && p.unique != 1) return fail(c, ORBX_ERR_INVALID_ARG, "unique is neither 0 nor 1");
  if (!std::isfinite(p.radius_px) || !(p.radius_px > 0.0))
    return fail(c, ORBX_ERR_INVALID_ARG, "radius_px must be finite, > 0");
  if (p.accept_lone != 0 && p.accept_lone != 1) return fail(c, ORBX_ERR_INVALID_ARG, "accept_lone is neither 0 nor 1");
  return ORBX_OK;
}

int gate_check_sizes(orbx_ctx* c, int n, int qcap, int tcap) {
  if (n < 1 || qcap < 1 || tcap < 1) return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1 or a capacity < 1");
  if (n > 65535) return fail(c, ORBX_ERR_UNSUPPORTED, "more windows than 65535");
  if (qcap > (1 << 22) || tcap > (1 << 22)) return fail(c, ORBX_ERR_UNSUPPORTED, "a capacity above 2^22");
  if ((unsigned long long)n * (unsigned long long)std::max(qcap, tcap) > 0x7fffffffull)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more slots in a batch than 32-bit offsets hold");
  return ORBX_OK;
}

struct GateSets {
  const orbx_descriptor* qdesc;
  const int32_t* qstate;
  const float* qxy;
  size_t point_stride, frame_stride;
  int qcap;
  const orbx_descriptor* tdesc;
  const int32_t* tstate;
  const double* txy;
  const int32_t* tpstate;
  int tcap;
};

// enqueues the gated re-association on s, which c->reloc.side has entered; arguments are checked.  Every buffer
// grows before the first block is given up, so a failed allocation keeps all three results
int gate_run(orbx_ctx* c, const GateSets& g, int n, const GateParams& p, hipStream_t s) {
  Reloc& r = c->reloc;
  Search& h = c->search;
  const RaBlock B((size_t)n, (size_t)g.qcap);
  const SgBlock C((size_t)n, (size_t)g.qcap);
  const SgScratch S((size_t)n, (size_t)g.tcap, sizeof(OrbxSgGrid), ORBX_SG_CELLS_MAX);
  int st;
  if (p.unique && (st = r.side.grow(c, r.best, sizeof(uint32_t) * (size_t)n * g.tcap)) != ORBX_OK) return st;
  if ((st = r.side.grow(c, h.gscr, S.bytes)) != ORBX_OK) return st;
  if ((st = r.side.grow(c, h.gblk, C.bytes)) != ORBX_OK) return st;
  if ((st = r.side.grow(c, r.rblk, B.bytes)) != ORBX_OK) return st;
  r.rn = 0;  // from here on the previous blocks are being replaced
  h.gn = 0;
  HIPCHK(c, orbx_launch_reassociate_gated(
                s, n, g.qdesc, g.qstate, g.qxy, g.point_stride, g.frame_stride, g.qcap, g.tdesc, g.tstate, g.txy,
                g.tpstate, g.tcap, p.radius_px, p.ratio, p.max_distance, p.accept_lone, p.unique,
                at<OrbxSgGrid>(h.gscr, S.grids), at<int32_t>(h.gscr, S.starts), at<int32_t>(h.gscr, S.sslot),
                at<double>(h.gscr, S.sxy), at<orbx_descriptor>(h.gscr, S.sdesc), (uint32_t*)r.best.p,
                at<int32_t>(r.rblk, B.origin), at<int32_t>(r.rblk, B.dist), at<int32_t>(h.gblk, C.candidates),
                at<int32_t>(r.rblk, B.count)));
  r.rn = n;
  r.rq = g.qcap;
  r.rt = g.tcap;
  h.gn = n;
  h.gq = g.qcap;
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_landmarks_project_device(orbx_ctx* c, const double* K, const double* d_pose6, size_t pose_stride,
                                  int n_windows, int source, int width, int height, double margin_px, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const ProjParams p{K, width, height, margin_px};
  int st = proj_check_params(c, p);
  if (st != ORBX_OK) return st;
  if (!d_pose6) return fail(c, ORBX_ERR_INVALID_ARG, "d_pose6 is NULL");
  if ((uintptr_t)d_pose6 & 7u) return fail(c, ORBX_ERR_INVALID_ARG, "d_pose6 is not 8-byte aligned");
  if (pose_stride < 6 || pose_stride > ((size_t)1 << 40)) return fail(c, ORBX_ERR_INVALID_ARG, "pose_stride < 6");
  if (c->lm.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks block has been built");
  if (n_windows != c->lm.n) return fail(c, ORBX_ERR_INVALID_ARG, "n_windows differs from the landmarks block");
  if (source != ORBX_CARRY_BUILT && source != ORBX_CARRY_SOLVED)
    return fail(c, ORBX_ERR_INVALID_ARG, "source is neither ORBX_CARRY_BUILT nor ORBX_CARRY_SOLVED");
  if (source == ORBX_CARRY_SOLVED && !c->lm.solved)
    return fail(c, ORBX_ERR_INVALID_ARG, "the landmarks block has not been solved");
  hipStream_t s = stream_of(c, stream);
  if ((st = c->search.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->search.side, s};
  // the block and its solve may have been written on another stream; so may the poses: the carried PnP's, the chain's
  // or the write-back's.  A gated re-association may still be reading the block this call replaces
  if ((st = c->search.side.after(c, c->lm.side, s)) != ORBX_OK) return st;
  if ((st = c->search.side.after(c, c->carry.side, s)) != ORBX_OK) return st;
  if ((st = c->search.side.after(c, c->wp.side, s)) != ORBX_OK) return st;
  if ((st = c->search.side.after(c, c->reloc.side, s)) != ORBX_OK) return st;
  const LmBlock L((size_t)c->lm.n, (size_t)c->lm.cap, (size_t)c->lm.len);
  const LmSolve V((size_t)c->lm.n, (size_t)c->lm.cap, (size_t)c->lm.len);
  OrbxCarryIn in;
  in.status = at<const int32_t>(c->lm.blk, L.status);
  in.pt_off = at<const int32_t>(c->lm.blk, L.pt_off);
  in.slot = at<const int32_t>(c->lm.blk, L.slot);
  in.src = source == ORBX_CARRY_SOLVED ? at<const double>(c->lm.sol, V.points) : at<const double>(c->lm.blk, L.points);
  in.old_cap = c->lm.cap;
  return proj_run(c, in, n_windows, c->lm.cap, d_pose6, pose_stride, p, s);
}

int orbx_landmarks_project_results_device(orbx_ctx* c, orbx_landmarks_projection_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  const Search& r = c->search;
  if (r.n < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no landmarks have been projected");
  const SpBlock B((size_t)r.n, (size_t)r.cap);
  v->xy = at<const double>(r.blk, B.xy);
  v->depth = at<const double>(r.blk, B.depth);
  v->state = at<const int32_t>(r.blk, B.state);
  v->count = at<const int32_t>(r.blk, B.count);
  v->slot_capacity = r.cap;
  v->n_windows = r.n;
  return ORBX_OK;
}

int orbx_landmarks_project_fetch(orbx_ctx* c, int first, int n, double* xy, double* depth, int32_t* state,
                                 int32_t* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = proj_range(c, first, n);
  if (st != ORBX_OK) return st;
  if ((st = c->search.side.wait(c)) != ORBX_OK) return st;
  const Search& r = c->search;
  const SpBlock B((size_t)r.n, (size_t)r.cap);
  const size_t s0 = (size_t)first * r.cap, ns = (size_t)n * r.cap;
  if (xy)
    HIPCHK(c, hipMemcpy(xy, at<const double>(r.blk, B.xy) + 2 * s0, sizeof(double) * 2 * ns, hipMemcpyDeviceToHost));
  if (depth)
    HIPCHK(c, hipMemcpy(depth, at<const double>(r.blk, B.depth) + s0, sizeof(double) * ns, hipMemcpyDeviceToHost));
  if (state)
    HIPCHK(c, hipMemcpy(state, at<const int32_t>(r.blk, B.state) + s0, sizeof(int32_t) * ns, hipMemcpyDeviceToHost));
  if (count)
    HIPCHK(c, hipMemcpy(count, at<const int32_t>(r.blk, B.count) + first, sizeof(int32_t) * (size_t)n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_project_landmarks(orbx_ctx* c, const double* points3, const int32_t* slot_of_point, int n_old,
                           int slot_capacity, const double* K, const double* pose6, int width, int height,
                           double margin_px, double* xy, double* depth, int32_t* state, int32_t* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const ProjParams p{K, width, height, margin_px};
  int st = proj_check_params(c, p);
  if (st != ORBX_OK) return st;
  if (n_old < 0 || (n_old > 0 && (!points3 || !slot_of_point)) || !pose6 || slot_capacity < 1)
    return fail(c, ORBX_ERR_INVALID_ARG, "n_old < 0, slot_capacity < 1, or a NULL array");
  if (n_old > ORBX_BA_MAX_POINTS || slot_capacity > ORBX_BA_MAX_POINTS)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more landmarks or slots in a window than 65536");
  hipStream_t s = c->stream;
  {
    if ((st = c->search.side.enter(c, s)) != ORBX_OK) return st;
    const SideWork::Mark mark{c->search.side, s};
    if ((st = c->search.side.after(c, c->reloc.side, s)) != ORBX_OK) return st;  // (a gated call may read the block)
    const SpStage G((size_t)n_old);
    if ((st = c->search.side.grow(c, c->search.stage, G.bytes)) != ORBX_OK) return st;
    const int32_t head[3] = {LM_OK, 0, n_old};
    uint8_t* g = (uint8_t*)c->search.stage.p;
    HIPCHK(c, hipMemcpyAsync(g + G.status, &head[0], sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(g + G.pt_off, &head[1], sizeof(int32_t) * 2, hipMemcpyHostToDevice, s));
    if (n_old > 0) {
      HIPCHK(c, hipMemcpyAsync(g + G.slot, slot_of_point, sizeof(int32_t) * (size_t)n_old, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(g + G.points, points3, sizeof(double) * 3 * (size_t)n_old, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, hipMemcpyAsync(g + G.pose6, pose6, sizeof(double) * 6, hipMemcpyHostToDevice, s));
    OrbxCarryIn in;
    in.status = (const int32_t*)(g + G.status);
    in.pt_off = (const int32_t*)(g + G.pt_off);
    in.slot = (const int32_t*)(g + G.slot);
    in.src = (const double*)(g + G.points);
    in.old_cap = INT_MAX;
    if ((st = proj_run(c, in, 1, slot_capacity, (const double*)(g + G.pose6), 6, p, s)) != ORBX_OK) return st;
  }
  HIPCHK(c, hipStreamSynchronize(s));  // (also: the host arrays have been read)
  return orbx_landmarks_project_fetch(c, 0, 1, xy, depth, state, count);
}

int orbx_reassociate_gated_device(orbx_ctx* c, const orbx_descriptor* d_query_desc, const int32_t* d_query_state,
                                  const float* d_query_xy, size_t point_stride, size_t xy_frame_stride, int q_capacity,
                                  const orbx_descriptor* d_train_desc, const int32_t* d_train_state,
                                  const double* d_train_xy, const int32_t* d_train_pstate, int t_capacity,
                                  int n_windows, double radius_px, double ratio, int max_distance, int accept_lone,
                                  int unique, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!d_query_desc || !d_query_state || !d_train_desc || !d_train_state)
    return fail(c, ORBX_ERR_INVALID_ARG, "a descriptor or state array is NULL");
  if ((((uintptr_t)d_query_desc | (uintptr_t)d_train_desc) & 15u) ||
      (((uintptr_t)d_query_state | (uintptr_t)d_train_state) & 3u))
    return fail(c, ORBX_ERR_INVALID_ARG, "a descriptor array is not 16-byte or a state array not 4-byte aligned");
  if (!d_query_xy || ((uintptr_t)d_query_xy & 3u))
    return fail(c, ORBX_ERR_INVALID_ARG, "d_query_xy is NULL or not 4-byte aligned");
  if (!d_train_xy || ((uintptr_t)d_train_xy & 7u))
    return fail(c, ORBX_ERR_INVALID_ARG, "d_train_xy is NULL or not 8-byte aligned");
  if ((uintptr_t)d_train_pstate & 3u) return fail(c, ORBX_ERR_INVALID_ARG, "d_train_pstate is not 4-byte aligned");
  const GateParams p{radius_px, ratio, max_distance, accept_lone, unique};
  int st = gate_check_sizes(c, n_windows, q_capacity, t_capacity);
  if (st != ORBX_OK) return st;
  if (point_stride < 2 || point_stride > ((size_t)1 << 40) || xy_frame_stride > ((size_t)1 << 48) ||
      xy_frame_stride < point_stride * (size_t)(q_capacity - 1) + 2)
    return fail(c, ORBX_ERR_INVALID_ARG, "point strides too small for q_capacity slots of two floats");
  if ((st = gate_check_params(c, p)) != ORBX_OK) return st;
  hipStream_t s = stream_of(c, stream);
  // (the banks were written under the same event: on another stream they are finished once enter() returns)
  if ((st = c->reloc.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->reloc.side, s};
  // the train positions may be the projection's block, the query points the good-features, top-up or windows
  // tracker's, each written on another stream
  if ((st = c->reloc.side.after(c, c->search.side, s)) != ORBX_OK) return st;
  if ((st = c->reloc.side.after(c, c->gf.side, s)) != ORBX_OK) return st;
  if ((st = c->reloc.side.after(c, c->lkw.side, s)) != ORBX_OK) return st;
  const GateSets g{d_query_desc, d_query_state, d_query_xy, point_stride, xy_frame_stride, q_capacity,
                   d_train_desc, d_train_state, d_train_xy, d_train_pstate, t_capacity};
  return gate_run(c, g, n_windows, p, s);
}

int orbx_reassociate_gated_results_device(orbx_ctx* c, orbx_reassociate_gated_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  const Search& h = c->search;
  if (h.gn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no gated re-association has run");
  const SgBlock C((size_t)h.gn, (size_t)h.gq);
  v->candidates = at<const int32_t>(h.gblk, C.candidates);
  v->q_capacity = h.gq;
  v->n_windows = h.gn;
  return ORBX_OK;
}

int orbx_reassociate_gated_fetch(orbx_ctx* c, int first, int n, int32_t* candidates) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const Search& h = c->search;
  if (h.gn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no gated re-association has run");
  if (!range_ok(first, n, h.gn)) return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the gated re-association");
  const int st = c->reloc.side.wait(c);
  if (st != ORBX_OK) return st;
  const SgBlock C((size_t)h.gn, (size_t)h.gq);
  if (candidates)
    HIPCHK(c, hipMemcpy(candidates, at<const int32_t>(h.gblk, C.candidates) + (size_t)first * h.gq,
                        sizeof(int32_t) * (size_t)n * h.gq, hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_reassociate_gated(orbx_ctx* c, const orbx_descriptor* query_desc, const int32_t* query_state,
                           const float* query_xy, int nq, const orbx_descriptor* train_desc,
                           const int32_t* train_state, const double* train_xy, const int32_t* train_pstate, int nt,
                           double radius_px, double ratio, int max_distance, int accept_lone, int unique,
                           int32_t* origin, int32_t* dist, int32_t* count, int32_t* candidates) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (nq < 0 || nt < 0 || (nq > 0 && (!query_desc || !query_state || !query_xy)) ||
      (nt > 0 && (!train_desc || !train_state || !train_xy)))
    return fail(c, ORBX_ERR_INVALID_ARG, "nq < 0, nt < 0, or a NULL array");
  const GateParams p{radius_px, ratio, max_distance, accept_lone, unique};
  int st = gate_check_params(c, p);
  if (st != ORBX_OK) return st;
  if (nq == 0) {
    if (count) *count = 0;
    return ORBX_OK;
  }
  // an empty train set runs as one slot that is not OK
  const int tcap = std::max(nt, 1);
  if ((st = gate_check_sizes(c, 1, nq, tcap)) != ORBX_OK) return st;
  hipStream_t s = c->stream;
  {
    if ((st = c->reloc.side.enter(c, s)) != ORBX_OK) return st;
    const SideWork::Mark mark{c->reloc.side, s};
    const SgStage G((size_t)nq, (size_t)tcap);
    if ((st = c->reloc.side.grow(c, c->search.gstage, G.bytes)) != ORBX_OK) return st;
    uint8_t* g = (uint8_t*)c->search.gstage.p;
    HIPCHK(c, hipMemcpyAsync(g + G.qdesc, query_desc, sizeof(orbx_descriptor) * (size_t)nq, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(g + G.qstate, query_state, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(g + G.qxy, query_xy, sizeof(float) * 2 * (size_t)nq, hipMemcpyHostToDevice, s));
    if (nt > 0) {
      HIPCHK(c, hipMemcpyAsync(g + G.tdesc, train_desc, sizeof(orbx_descriptor) * (size_t)nt, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(g + G.tstate, train_state, sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(g + G.txy, train_xy, sizeof(double) * 2 * (size_t)nt, hipMemcpyHostToDevice, s));
      if (train_pstate)
        HIPCHK(c, hipMemcpyAsync(g + G.tpstate, train_pstate, sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, s));
    } else {
      HIPCHK(c, hipMemsetAsync(g + G.tdesc, 0, sizeof(orbx_descriptor), s));
      HIPCHK(c, hipMemsetAsync(g + G.tstate, 0, sizeof(int32_t), s));
      HIPCHK(c, hipMemsetAsync(g + G.txy, 0, sizeof(double) * 2, s));
    }
    const GateSets sets{(const orbx_descriptor*)(g + G.qdesc), (const int32_t*)(g + G.qstate),
                        (const float*)(g + G.qxy), 2, 2 * (size_t)nq, nq,
                        (const orbx_descriptor*)(g + G.tdesc), (const int32_t*)(g + G.tstate),
                        (const double*)(g + G.txy),
                        nt > 0 && train_pstate ? (const int32_t*)(g + G.tpstate) : nullptr, tcap};
    if ((st = gate_run(c, sets, 1, p, s)) != ORBX_OK) return st;
  }
  HIPCHK(c, hipStreamSynchronize(s));  // (also: the host arrays have been read)
  if ((st = orbx_reassociate_gated_fetch(c, 0, 1, candidates)) != ORBX_OK) return st;
  return orbx_reassociate_fetch(c, 0, 1, origin, dist, count);
}

}  // extern "C"
