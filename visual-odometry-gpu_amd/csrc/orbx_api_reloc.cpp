// orbx_api_reloc.cpp -- host layer of liborbx.so (orbx_host.h) behind include/orbx_reloc.h: ORB descriptors at points
// the caller holds, in two banks, and the re-association of two described sets into an `origin` block that the
// landmarks carry reads.  The reference runs ORB on the whole frame and matches when tracking
// leaves fewer than 150 points (src/feature_tracking.cpp:68-71, src/feature_tracking.cpp:203-219).
#include <algorithm>
#include <cmath>

#include "../../include/orbx_reloc.h"
#include "orbx_host.h"

using namespace orbx_host;

static_assert((int)ORBX_PD_NONE == (int)PD_NONE && (int)ORBX_PD_BORDER == (int)PD_BORDER && (int)ORBX_PD_OK == (int)PD_OK,
              "orbx_pd_state");
static_assert(ORBX_PD_BANKS == 2, "Reloc::bank");

namespace {

struct PdPoints {
  const float* d_xy;
  size_t point_stride, frame_stride;
  const int32_t* d_seen;
  int seen_min;
  const int32_t* d_counts;
  int cap;
};

bool bank_ok(int bank) { return bank >= 0 && bank < ORBX_PD_BANKS; }

// what rule D asks of k_pd_level0
int level0_kind(const orbx_ctx* c) { return c->p.blur_levels == ORBX_BLUR_ALL ? c->p.blur_kind : PD_LEVEL0_COPY; }

int pd_check(orbx_ctx* c, const PdPoints& p, int n, int bank) {
  if (!p.d_xy || p.cap < 1) return fail(c, ORBX_ERR_INVALID_ARG, "d_xy is NULL or slot_capacity < 1");
  if (!bank_ok(bank)) return fail(c, ORBX_ERR_INVALID_ARG, "bank outside [0, ORBX_PD_BANKS)");
  if (((uintptr_t)p.d_xy | (uintptr_t)p.d_seen | (uintptr_t)p.d_counts) & 3u)
    return fail(c, ORBX_ERR_INVALID_ARG, "d_xy / d_seen / d_counts is not 4-byte aligned");
  if (p.point_stride < 2 || p.point_stride > ((size_t)1 << 40) || p.frame_stride > ((size_t)1 << 48) ||
      p.frame_stride < p.point_stride * (size_t)(p.cap - 1) + 2)
    return fail(c, ORBX_ERR_INVALID_ARG, "point strides too small for slot_capacity slots of two floats");
  if (c->p.patch_size / 2 > PD_R_MIN) return fail(c, ORBX_ERR_UNSUPPORTED, "patch_size / 2 above 20");
  if ((unsigned long long)n * (unsigned long long)p.cap > 0x7fffffffull)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more slots in a batch than 32-bit offsets hold");
  return ORBX_OK;
}

// enqueues the describe of n device frames into `bank` on s, slice by slice; arguments are checked
int pd_run(orbx_ctx* c, const uint8_t* d_frames, int n, int w, int h, int row_stride, size_t frame_stride,
           const PdPoints& p, int bank, hipStream_t s) {
  Reloc& r = c->reloc;
  const PdBlock B((size_t)n, (size_t)p.cap);
  const int per = pd_slice_frames(r.ws_limit, n, w, h);
  const size_t img_stride = pd_img_stride(w, h);
  int st;
  if ((st = r.side.grow(c, r.ws, img_stride * (size_t)per)) != ORBX_OK) return st;
  if ((st = r.side.grow(c, r.list, sizeof(int32_t) * B.slots)) != ORBX_OK) return st;
  if ((st = r.side.grow(c, r.bank[bank], B.bytes)) != ORBX_OK) return st;
  r.n[bank] = 0;  // from here on the previous block is being replaced
  const int pitch = pd_pitch(w), kind = level0_kind(c);
  orbx_descriptor* desc = at<orbx_descriptor>(r.bank[bank], B.desc);
  float* angle = at<float>(r.bank[bank], B.angle);
  int32_t* state = at<int32_t>(r.bank[bank], B.state);
  int32_t* n_ok = at<int32_t>(r.bank[bank], B.n_ok);
  int32_t* list = (int32_t*)r.list.p;
  for (int f0 = 0; f0 < n; f0 += per) {
    const int m = std::min(per, n - f0);
    const size_t row = (size_t)p.cap * f0;
    HIPCHK(c, orbx_launch_pd_level0(s, d_frames + frame_stride * (size_t)f0, m, w, h, row_stride, frame_stride, kind,
                                    (uint8_t*)r.ws.p, pitch, img_stride));
    HIPCHK(c, orbx_launch_pd_describe(s, (const uint8_t*)r.ws.p, m, w, h, pitch, img_stride,
                                      p.d_xy + p.frame_stride * (size_t)f0, p.point_stride, p.frame_stride,
                                      p.d_seen ? p.d_seen + row : nullptr, p.seen_min,
                                      p.d_counts ? p.d_counts + f0 : nullptr, p.cap, c->p.patch_size, state + row,
                                      angle + row, desc + row, n_ok + f0, list + row));
  }
  r.n[bank] = n;
  r.cap[bank] = p.cap;
  return ORBX_OK;
}

int pd_bank_check(orbx_ctx* c, int bank) {
  if (!bank_ok(bank)) return fail(c, ORBX_ERR_INVALID_ARG, "bank outside [0, ORBX_PD_BANKS)");
  if (c->reloc.n[bank] < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no points have been described into this bank");
  return ORBX_OK;
}

struct RaParams {
  double ratio;
  int max_distance, unique;
};

int ra_check_params(orbx_ctx* c, const RaParams& p) {
  if (!std::isfinite(p.ratio) || p.ratio < 0.0) return fail(c, ORBX_ERR_INVALID_ARG, "ratio must be finite, >= 0");
  if (p.max_distance < 0 || p.max_distance > 256) return fail(c, ORBX_ERR_INVALID_ARG, "max_distance outside [0, 256]");
  if (p.unique != 0 && p.unique != 1) return fail(c, ORBX_ERR_INVALID_ARG, "unique is neither 0 nor 1");
  return ORBX_OK;
}

int ra_check_sizes(orbx_ctx* c, int n, int qcap, int tcap) {
  if (n < 1 || qcap < 1 || tcap < 1) return fail(c, ORBX_ERR_INVALID_ARG, "n_windows < 1 or a capacity < 1");
  if (n > 65535) return fail(c, ORBX_ERR_UNSUPPORTED, "more windows than 65535");
  if (qcap > (1 << 22) || tcap > (1 << 22)) return fail(c, ORBX_ERR_UNSUPPORTED, "a capacity above 2^22");
  if ((unsigned long long)n * (unsigned long long)std::max(qcap, tcap) > 0x7fffffffull)
    return fail(c, ORBX_ERR_UNSUPPORTED, "more slots in a batch than 32-bit offsets hold");
  return ORBX_OK;
}

// enqueues the re-association on s, which c->reloc.side has entered; arguments are checked
int ra_run(orbx_ctx* c, const orbx_descriptor* qd, const int32_t* qs, int qcap, const orbx_descriptor* td,
           const int32_t* ts, int tcap, int n, const RaParams& p, hipStream_t s) {
  Reloc& r = c->reloc;
  const RaBlock B((size_t)n, (size_t)qcap);
  int st;
  if (p.unique && (st = r.side.grow(c, r.best, sizeof(uint32_t) * (size_t)n * tcap)) != ORBX_OK) return st;
  if ((st = r.side.grow(c, r.rblk, B.bytes)) != ORBX_OK) return st;
  r.rn = 0;  // from here on the previous block is being replaced
  HIPCHK(c, orbx_launch_reassociate(s, n, qd, qs, qcap, td, ts, tcap, p.ratio, p.max_distance, p.unique,
                                    (uint32_t*)r.best.p, at<int32_t>(r.rblk, B.origin), at<int32_t>(r.rblk, B.dist),
                                    at<int32_t>(r.rblk, B.count)));
  r.rn = n;
  r.rq = qcap;
  r.rt = tcap;
  return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_describe_points_device(orbx_ctx* c, const void* d_frames, int n, int width, int height, int row_stride,
                                size_t frame_stride, const float* d_xy, size_t point_stride, size_t xy_frame_stride,
                                const int32_t* d_seen, int seen_min, const int32_t* d_counts, int slot_capacity,
                                int bank, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = check_device_frames(c, d_frames, n, 1, c->p.max_batch, width, height, row_stride, frame_stride,
                               {"d_frames is NULL", "n outside [1, max_batch]"});
  if (st != ORBX_OK) return st;
  const PdPoints p{d_xy, point_stride, xy_frame_stride, d_seen, seen_min, d_counts, slot_capacity};
  if ((st = pd_check(c, p, n, bank)) != ORBX_OK) return st;
  hipStream_t s = stream_of(c, stream);
  if ((st = c->reloc.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->reloc.side, s};
  // the points may be the good-features, top-up or windows tracker's block, written on another stream
  if ((st = c->reloc.side.after(c, c->gf.side, s)) != ORBX_OK) return st;
  if ((st = c->reloc.side.after(c, c->lkw.side, s)) != ORBX_OK) return st;
  return pd_run(c, (const uint8_t*)d_frames, n, width, height, row_stride, frame_stride, p, bank, s);
}

int orbx_describe_points_workspace_limit(orbx_ctx* c, size_t bytes) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  return set_workspace_limit(c, c->reloc.side, {&c->reloc.ws}, &c->reloc.ws_limit, bytes, ORBX_PD_WORKSPACE_DEFAULT);
}

int orbx_point_descriptors_results_device(orbx_ctx* c, int bank, orbx_point_descriptors_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  const int st = pd_bank_check(c, bank);
  if (st != ORBX_OK) return st;
  const Reloc& r = c->reloc;
  const PdBlock B((size_t)r.n[bank], (size_t)r.cap[bank]);
  v->desc = at<const orbx_descriptor>(r.bank[bank], B.desc);
  v->angle = at<const float>(r.bank[bank], B.angle);
  v->state = at<const int32_t>(r.bank[bank], B.state);
  v->n_ok = at<const int32_t>(r.bank[bank], B.n_ok);
  v->slot_capacity = r.cap[bank];
  v->n = r.n[bank];
  return ORBX_OK;
}

int orbx_point_descriptors_fetch(orbx_ctx* c, int bank, int first, int n, orbx_descriptor* desc, float* angle,
                                 int32_t* state, int32_t* n_ok) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  int st = pd_bank_check(c, bank);
  if (st != ORBX_OK) return st;
  const Reloc& r = c->reloc;
  if (!range_ok(first, n, r.n[bank])) return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the bank");
  if ((st = c->reloc.side.wait(c)) != ORBX_OK) return st;
  const PdBlock B((size_t)r.n[bank], (size_t)r.cap[bank]);
  const size_t s0 = (size_t)first * r.cap[bank], ns = (size_t)n * r.cap[bank];
  if (desc)
    HIPCHK(c, hipMemcpy(desc, at<const orbx_descriptor>(r.bank[bank], B.desc) + s0, sizeof(orbx_descriptor) * ns,
                        hipMemcpyDeviceToHost));
  if (angle)
    HIPCHK(c, hipMemcpy(angle, at<const float>(r.bank[bank], B.angle) + s0, sizeof(float) * ns, hipMemcpyDeviceToHost));
  if (state)
    HIPCHK(c, hipMemcpy(state, at<const int32_t>(r.bank[bank], B.state) + s0, sizeof(int32_t) * ns,
                        hipMemcpyDeviceToHost));
  if (n_ok)
    HIPCHK(c, hipMemcpy(n_ok, at<const int32_t>(r.bank[bank], B.n_ok) + first, sizeof(int32_t) * (size_t)n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_describe_points(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, const float* points_xy,
                         int n_points, float* angle, orbx_descriptor* desc, int32_t* state) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (n_points < 0 || (n_points > 0 && !points_xy))
    return fail(c, ORBX_ERR_INVALID_ARG, "n_points < 0 or points_xy is NULL");
  if (c->p.patch_size / 2 > PD_R_MIN) return fail(c, ORBX_ERR_UNSUPPORTED, "patch_size / 2 above 20");
  if (n_points == 0) return ORBX_OK;
  hipStream_t s = c->stream;
  const PdStage G((size_t)width, (size_t)height, (size_t)n_points);
  {
    if ((st = c->reloc.side.enter(c, s)) != ORBX_OK) return st;
    const SideWork::Mark mark{c->reloc.side, s};
    if ((st = c->reloc.side.grow(c, c->reloc.stage, G.bytes)) != ORBX_OK) return st;
    uint8_t* g = (uint8_t*)c->reloc.stage.p;
    const PdPoints p{(const float*)(g + G.xy), 2, 2 * (size_t)n_points, nullptr, 0, nullptr, n_points};
    if ((st = pd_check(c, p, 1, 0)) != ORBX_OK) return st;
    HIPCHK(c, hipMemcpy2DAsync(g + G.img, (size_t)width, image, (size_t)stride, (size_t)width, (size_t)height,
                               hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(g + G.xy, points_xy, sizeof(float) * 2 * (size_t)n_points, hipMemcpyHostToDevice,
                             s));
    if ((st = pd_run(c, g + G.img, 1, width, height, width, (size_t)width * height, p, 0, s)) != ORBX_OK) return st;
  }
  HIPCHK(c, hipStreamSynchronize(s));  // (also: the host arrays have been read)
  return orbx_point_descriptors_fetch(c, 0, 0, 1, desc, angle, state, nullptr);
}

int orbx_reassociate_device(orbx_ctx* c, const orbx_descriptor* d_query_desc, const int32_t* d_query_state,
                            int q_capacity, const orbx_descriptor* d_train_desc, const int32_t* d_train_state,
                            int t_capacity, int n_windows, double ratio, int max_distance, int unique, void* stream) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!d_query_desc || !d_query_state || !d_train_desc || !d_train_state)
    return fail(c, ORBX_ERR_INVALID_ARG, "a descriptor or state array is NULL");
  if ((((uintptr_t)d_query_desc | (uintptr_t)d_train_desc) & 15u) ||
      (((uintptr_t)d_query_state | (uintptr_t)d_train_state) & 3u))
    return fail(c, ORBX_ERR_INVALID_ARG, "a descriptor array is not 16-byte or a state array not 4-byte aligned");
  const RaParams p{ratio, max_distance, unique};
  int st = ra_check_sizes(c, n_windows, q_capacity, t_capacity);
  if (st != ORBX_OK) return st;
  if ((st = ra_check_params(c, p)) != ORBX_OK) return st;
  hipStream_t s = stream_of(c, stream);
  // (the banks were written under the same event: on another stream they are finished once enter() returns)
  if ((st = c->reloc.side.enter(c, s)) != ORBX_OK) return st;
  const SideWork::Mark mark{c->reloc.side, s};
  return ra_run(c, d_query_desc, d_query_state, q_capacity, d_train_desc, d_train_state, t_capacity, n_windows, p, s);
}

int orbx_reassociate_results_device(orbx_ctx* c, orbx_reassociate_view* v) {
  DeviceGuard _dg(c);
  if (!c || !v) return ORBX_ERR_INVALID_ARG;
  const Reloc& r = c->reloc;
  if (r.rn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no re-association has run");
  const RaBlock B((size_t)r.rn, (size_t)r.rq);
  v->origin = at<const int32_t>(r.rblk, B.origin);
  v->dist = at<const int32_t>(r.rblk, B.dist);
  v->count = at<const int32_t>(r.rblk, B.count);
  v->q_capacity = r.rq;
  v->t_capacity = r.rt;
  v->n_windows = r.rn;
  return ORBX_OK;
}

int orbx_reassociate_fetch(orbx_ctx* c, int first, int n, int32_t* origin, int32_t* dist, int32_t* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const Reloc& r = c->reloc;
  if (r.rn < 1) return fail(c, ORBX_ERR_INVALID_ARG, "no re-association has run");
  if (!range_ok(first, n, r.rn)) return fail(c, ORBX_ERR_INVALID_ARG, "[first, first + n) outside the re-association");
  const int st = c->reloc.side.wait(c);
  if (st != ORBX_OK) return st;
  const RaBlock B((size_t)r.rn, (size_t)r.rq);
  const size_t s0 = (size_t)first * r.rq, ns = (size_t)n * r.rq;
  if (origin)
    HIPCHK(c, hipMemcpy(origin, at<const int32_t>(r.rblk, B.origin) + s0, sizeof(int32_t) * ns, hipMemcpyDeviceToHost));
  if (dist)
    HIPCHK(c, hipMemcpy(dist, at<const int32_t>(r.rblk, B.dist) + s0, sizeof(int32_t) * ns, hipMemcpyDeviceToHost));
  if (count)
    HIPCHK(c, hipMemcpy(count, at<const int32_t>(r.rblk, B.count) + first, sizeof(int32_t) * (size_t)n,
                        hipMemcpyDeviceToHost));
  return ORBX_OK;
}

int orbx_reassociate(orbx_ctx* c, const orbx_descriptor* query_desc, const int32_t* query_state, int nq,
                     const orbx_descriptor* train_desc, const int32_t* train_state, int nt, double ratio,
                     int max_distance, int unique, int32_t* origin, int32_t* dist, int32_t* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (nq < 0 || nt < 0 || (nq > 0 && (!query_desc || !query_state)) || (nt > 0 && (!train_desc || !train_state)))
    return fail(c, ORBX_ERR_INVALID_ARG, "nq < 0, nt < 0, or a NULL array");
  const RaParams p{ratio, max_distance, unique};
  int st = ra_check_params(c, p);
  if (st != ORBX_OK) return st;
  if (nq == 0) {
    if (count) *count = 0;
    return ORBX_OK;
  }
  // an empty train set runs as one slot that is not OK
  const int tcap = std::max(nt, 1);
  if ((st = ra_check_sizes(c, 1, nq, tcap)) != ORBX_OK) return st;
  hipStream_t s = c->stream;
  {
    if ((st = c->reloc.side.enter(c, s)) != ORBX_OK) return st;
    const SideWork::Mark mark{c->reloc.side, s};
    const RaStage G((size_t)nq, (size_t)tcap);
    if ((st = c->reloc.side.grow(c, c->reloc.rstage, G.bytes)) != ORBX_OK) return st;
    uint8_t* g = (uint8_t*)c->reloc.rstage.p;
    HIPCHK(c, hipMemcpyAsync(g + G.qdesc, query_desc, sizeof(orbx_descriptor) * (size_t)nq, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(g + G.qstate, query_state, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, s));
    if (nt > 0) {
      HIPCHK(c, hipMemcpyAsync(g + G.tdesc, train_desc, sizeof(orbx_descriptor) * (size_t)nt, hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(g + G.tstate, train_state, sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, s));
    } else {
      HIPCHK(c, hipMemsetAsync(g + G.tdesc, 0, sizeof(orbx_descriptor), s));
      HIPCHK(c, hipMemsetAsync(g + G.tstate, 0, sizeof(int32_t), s));
    }
    if ((st = ra_run(c, (const orbx_descriptor*)(g + G.qdesc), (const int32_t*)(g + G.qstate), nq,
                     (const orbx_descriptor*)(g + G.tdesc), (const int32_t*)(g + G.tstate), tcap, 1, p, s)) != ORBX_OK)
      return st;
  }
  HIPCHK(c, hipStreamSynchronize(s));  // (also: the host arrays have been read)
  return orbx_reassociate_fetch(c, 0, 1, origin, dist, count);
}

}  // extern "C"
