// orbx_api_stage.cpp -- host layer of liborbx.so (orbx_host.h): the stage-level operators on one host image, on the
// context's stage scratch, and the descriptor matcher (host arrays and the last batch's frames).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "orbx_host.h"

using namespace orbx_host;

namespace {

// single-level plan over a scratch image, for the stage-level operators
OrbxPlan flat_plan(int w, int h, int cap) {
  OrbxPlan P;
  std::memset(&P, 0, sizeof(P));
  P.nlevels = 1;
  P.w0 = w;
  P.h0 = h;
  OrbxLevel& L = P.L[0];
  L.w = w;
  L.h = h;
  L.pitch = align_up(w, 64);
  L.mask_wpr = (w + 63) / 64;
  L.cap = cap;
  L.quota = cap;
  L.scale = 1.0f;
  P.frame_bytes = (int32_t)align_up_sz((size_t)L.pitch * h, 256);
  P.mask_words = L.mask_wpr * h;
  P.cand_total = cap;
  P.out_cap = cap;
  return P;
}

// upload a host image into a zero-padded, 64-aligned-pitch scratch image
int upload_flat(orbx_ctx* c, DevBuf& b, const uint8_t* img, int w, int h, int stride, int* pitch) {
  const int p = align_up(w, 64);
  ENSURE(c, b, (size_t)p * h + 256);
  HIPCHK(c, hipMemsetAsync(b.p, 0, (size_t)p * h, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(b.p, p, img, stride, w, h, hipMemcpyHostToDevice, c->stream));
  *pitch = p;
  return ORBX_OK;
}

}  // namespace

extern "C" {

// ---- stage-level operators --------------------------------------------------

int orbx_fast_score(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int threshold, int n,
                    float* scores) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!scores || n < 1 || n > 16 || threshold < 0 || threshold > 255)
    return fail(c, ORBX_ERR_INVALID_ARG, "scores NULL or n/threshold out of range");
  int pitch;
  st = upload_flat(c, c->s.img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  OrbxPlan P = flat_plan(width, height, 0);
  OrbxBandMap bm;
  std::string why;
  if ((st = make_bandmap(P, 0, &bm, &why)) != ORBX_OK) return fail(c, st, why);
  std::vector<OrbxTileDesc> t;
  build_fast_tiles(P, bm, 0, 1, &t);
  ENSURE(c, c->s.tiles, t.size() * sizeof(OrbxTileDesc));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->s.tiles.p, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
  const size_t npx = (size_t)width * height;
  ENSURE(c, c->s.u16, npx * 2);
  ENSURE(c, c->s.mask, (size_t)P.mask_words * 8);
  OrbxFastParams fp{threshold, n, 0};
  HIPCHK(c, orbx_launch_fast_nms(c->stream, (const OrbxTileDesc*)c->s.tiles.p, (int)t.size(), 1,
                                 (const uint8_t*)c->s.img_a.p, P.frame_bytes, P.mask_words, fp,
                                 (unsigned long long*)c->s.mask.p, (uint16_t*)c->s.u16.p, nullptr));
  std::vector<uint16_t> h(npx);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->s.u16.p, npx * 2, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < npx; i++) scores[i] = (float)h[i];
  return ORBX_OK;
}

static int compact_and_fetch(orbx_ctx* c, const OrbxPlan& P, int nfeatures, orbx_keypoint* keypoints, int* count,
                             int* total) {
  ENSURE(c, c->s.kps, sizeof(orbx_keypoint) * (size_t)std::max(nfeatures, 1));
  ENSURE(c, c->s.i32, 64);
  int32_t* d_cnt = (int32_t*)c->s.i32.p;
  HIPCHK(c, orbx_launch_compact(c->stream, P, 1, (const unsigned long long*)c->s.mask.p, (orbx_keypoint*)c->s.kps.p,
                                d_cnt, d_cnt + 1, 1));
  int32_t h[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[0] > 0)
    HIPCHK(c, hipMemcpy(keypoints, c->s.kps.p, sizeof(orbx_keypoint) * (size_t)h[0], hipMemcpyDeviceToHost));
  *count = h[0];
  if (total) *total = h[1];
  return ORBX_OK;
}

int orbx_fast(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int threshold, int n,
              int nms_window, int nfeatures, orbx_keypoint* keypoints, int* count, int* total) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!count || (!keypoints && nfeatures > 0) || nfeatures < 0 || n < 1 || n > 16 || threshold < 0 ||
      threshold > 255 || nms_window < 0 || nms_window / 2 > 3)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad Fast() arguments");
  int pitch;
  st = upload_flat(c, c->s.img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  OrbxPlan P = flat_plan(width, height, nfeatures);
  OrbxBandMap bm;
  std::string why;
  if ((st = make_bandmap(P, nms_window / 2, &bm, &why)) != ORBX_OK) return fail(c, st, why);
  std::vector<OrbxTileDesc> t;
  build_fast_tiles(P, bm, 0, 1, &t);
  ENSURE(c, c->s.tiles, t.size() * sizeof(OrbxTileDesc));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->s.tiles.p, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
  ENSURE(c, c->s.mask, (size_t)P.mask_words * 8);
  OrbxFastParams fp{threshold, n, nms_window / 2};
  // stage operator: exact totals are part of the contract -> no early exit
  HIPCHK(c, orbx_launch_fast_nms(c->stream, (const OrbxTileDesc*)c->s.tiles.p, (int)t.size(), 1,
                                 (const uint8_t*)c->s.img_a.p, P.frame_bytes, P.mask_words, fp,
                                 (unsigned long long*)c->s.mask.p, nullptr, nullptr));
  return compact_and_fetch(c, P, nfeatures, keypoints, count, total);
}

int orbx_nms(orbx_ctx* c, const float* scores, int width, int height, int nms_window, int nfeatures,
             float threshold, orbx_keypoint* keypoints, int* count, int* total) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!scores || !count || (!keypoints && nfeatures > 0) || nfeatures < 0 || width < 1 || height < 1 ||
      nms_window < 0 || nms_window / 2 > 3)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad NMS() arguments");
  const size_t npx = (size_t)width * height;
  ENSURE(c, c->s.f32, npx * 4);
  OrbxPlan P = flat_plan(width, height, nfeatures);
  ENSURE(c, c->s.mask, (size_t)P.mask_words * 8);
  HIPCHK(c, hipMemcpyAsync(c->s.f32.p, scores, npx * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_nms_f32(c->stream, (const float*)c->s.f32.p, width, height, nms_window / 2, threshold,
                                (unsigned long long*)c->s.mask.p, P.L[0].mask_wpr));
  return compact_and_fetch(c, P, nfeatures, keypoints, count, total);
}

static int describe_stage(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                          const orbx_keypoint* keypoints, int nkp, int patch_size, const float* angles_in,
                          float* angles_out, orbx_descriptor* desc_out) {
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (nkp < 0 || (nkp > 0 && !keypoints)) return fail(c, ORBX_ERR_INVALID_ARG, "keypoints NULL / nkp < 0");
  if (patch_size < 1 || patch_size / 2 > 20) return fail(c, ORBX_ERR_INVALID_ARG, "patch_size must be in [1, 41]");
  if (nkp == 0) return ORBX_OK;
  for (int i = 0; i < nkp; i++)
    if (keypoints[i].x < 0 || keypoints[i].y < 0 || keypoints[i].x >= width || keypoints[i].y >= height)
      return fail(c, ORBX_ERR_INVALID_ARG, "keypoint outside the image");
  if (angles_in)
    for (int i = 0; i < nkp; i++)
      if (!(std::fabs(angles_in[i]) < 100.0f))
        return fail(c, ORBX_ERR_INVALID_ARG, "orientation must be finite and |angle| < 100 rad");
  int pitch;
  st = upload_flat(c, c->s.img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  ENSURE(c, c->s.kps, sizeof(orbx_keypoint) * (size_t)nkp);
  ENSURE(c, c->s.f32b, sizeof(float) * (size_t)nkp);
  ENSURE(c, c->s.desc, sizeof(orbx_descriptor) * (size_t)nkp);
  HIPCHK(c, hipMemcpyAsync(c->s.kps.p, keypoints, sizeof(orbx_keypoint) * (size_t)nkp, hipMemcpyHostToDevice,
                           c->stream));
  if (angles_in)
    HIPCHK(c, hipMemcpyAsync(c->s.f32b.p, angles_in, sizeof(float) * (size_t)nkp, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_describe_flat(c->stream, (const uint8_t*)c->s.img_a.p, width, height, pitch,
                                      (const orbx_keypoint*)c->s.kps.p, nkp, patch_size, angles_in != nullptr,
                                      desc_out != nullptr, (float*)c->s.f32b.p, (orbx_descriptor*)c->s.desc.p));
  if (angles_out)
    HIPCHK(c, hipMemcpyAsync(angles_out, c->s.f32b.p, sizeof(float) * (size_t)nkp, hipMemcpyDeviceToHost, c->stream));
  if (desc_out)
    HIPCHK(c, hipMemcpyAsync(desc_out, c->s.desc.p, sizeof(orbx_descriptor) * (size_t)nkp, hipMemcpyDeviceToHost,
                             c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_orientations(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                      const orbx_keypoint* keypoints, int nkp, int patch_size, float* orientations) {
  DeviceGuard _dg(c);
  if (c && nkp > 0 && !orientations) return fail(c, ORBX_ERR_INVALID_ARG, "orientations is NULL");
  return describe_stage(c, image, width, height, stride, keypoints, nkp, patch_size, nullptr, orientations, nullptr);
}

int orbx_brief(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
               const orbx_keypoint* keypoints, const float* orientations, int nkp, orbx_descriptor* descriptors) {
  DeviceGuard _dg(c);
  if (c && nkp > 0 && (!orientations || !descriptors))
    return fail(c, ORBX_ERR_INVALID_ARG, "orientations/descriptors is NULL");
  return describe_stage(c, image, width, height, stride, keypoints, nkp, 31, orientations, nullptr, descriptors);
}

int orbx_harris(orbx_ctx* c, const uint8_t* image, int width, int height, int stride,
                const orbx_keypoint* keypoints, int nkp, int window, float k, float* responses) {
  DeviceGuard _dg(c);
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (nkp < 0 || (nkp > 0 && (!keypoints || !responses)) || window < 1 || (window % 2) == 0 || window > 15)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad HarrisScore() arguments");
  if (nkp == 0) return ORBX_OK;
  for (int i = 0; i < nkp; i++)
    if (keypoints[i].x < 0 || keypoints[i].y < 0 || keypoints[i].x >= width || keypoints[i].y >= height)
      return fail(c, ORBX_ERR_INVALID_ARG, "keypoint outside the image");
  int pitch;
  st = upload_flat(c, c->s.img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  std::vector<float> g((size_t)window * window);
  gaussian_kernel(window, -1.0f, g.data());
  ENSURE(c, c->s.kern, g.size() * 4);
  ENSURE(c, c->s.kps, sizeof(orbx_keypoint) * (size_t)nkp);
  ENSURE(c, c->s.f32b, sizeof(float) * (size_t)nkp);
  HIPCHK(c, hipMemcpyAsync(c->s.kern.p, g.data(), g.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->s.kps.p, keypoints, sizeof(orbx_keypoint) * (size_t)nkp, hipMemcpyHostToDevice,
                           c->stream));
  HIPCHK(c, orbx_launch_harris_flat(c->stream, (const uint8_t*)c->s.img_a.p, width, height, pitch,
                                    (const orbx_keypoint*)c->s.kps.p, nkp, (const float*)c->s.kern.p, window, k,
                                    (float*)c->s.f32b.p));
  HIPCHK(c, hipMemcpyAsync(responses, c->s.f32b.p, sizeof(float) * (size_t)nkp, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

static int blur_stage(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                      int dst_stride, int kind) {
  int st = check_image(c, image, width, height, stride);
  if (st != ORBX_OK) return st;
  if (!dst || dst_stride < width) return fail(c, ORBX_ERR_INVALID_ARG, "dst NULL or dst_stride < width");
  int pitch;
  st = upload_flat(c, c->s.img_a, image, width, height, stride, &pitch);
  if (st != ORBX_OK) return st;
  OrbxPlan P = flat_plan(width, height, 0);
  ENSURE(c, c->s.img_b, (size_t)P.frame_bytes + 256);
  OrbxTileMap tm;
  make_tilemap(P, ORBX_BLUR_TW, ORBX_BLUR_TH, true, &tm);
  std::vector<OrbxTileDesc> t;
  blur_tiles_for_impl(c->blur_impl, P, &t);
  ENSURE(c, c->s.tiles, t.size() * sizeof(OrbxTileDesc));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->s.tiles.p, t.data(), t.size() * sizeof(OrbxTileDesc), hipMemcpyHostToDevice));
  HIPCHK(c, launch_blur_auto(c->blur_impl, c->stream, P, tm, (const OrbxTileDesc*)c->s.tiles.p, (int)t.size(), 1,
                             (const uint8_t*)c->s.img_a.p, (uint8_t*)c->s.img_b.p, 0, kind));
  HIPCHK(c, hipMemcpy2DAsync(dst, dst_stride, c->s.img_b.p, pitch, width, height, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_blur5_sep(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                   int dst_stride) {
  DeviceGuard _dg(c);
  return blur_stage(c, image, width, height, stride, dst, dst_stride, ORBX_BLUR_SEP16);
}

int orbx_blur5_273(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                   int dst_stride) {
  DeviceGuard _dg(c);
  return blur_stage(c, image, width, height, stride, dst, dst_stride, ORBX_BLUR_K273);
}

static int conv_stage(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, const float* kernel,
                      int K, int reflect_pad, uint8_t* dst) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!image || !kernel || !dst || width < 1 || height < 1 || stride < width || K < 1 || (K % 2) == 0 || K > 31)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad conv2d() arguments (kernel_size must be odd, <= 31)");
  const int wo = reflect_pad ? width : width - K + 1, ho = reflect_pad ? height : height - K + 1;
  if (wo < 1 || ho < 1) return fail(c, ORBX_ERR_INVALID_ARG, "image smaller than the kernel");
  if (reflect_pad && (width < K / 2 + 1 || height < K / 2 + 1))
    return fail(c, ORBX_ERR_INVALID_ARG, "image too small for REFLECT_101 padding");
  int pitch;
  const int p = align_up(width, 64);
  ENSURE(c, c->s.img_a, (size_t)p * height + 256);
  HIPCHK(c, hipMemcpy2DAsync(c->s.img_a.p, p, image, stride, width, height, hipMemcpyHostToDevice, c->stream));
  pitch = p;
  ENSURE(c, c->s.img_b, (size_t)wo * ho + 256);
  ENSURE(c, c->s.kern, (size_t)K * K * 4);
  HIPCHK(c, hipMemcpyAsync(c->s.kern.p, kernel, (size_t)K * K * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_conv2d(c->stream, (const uint8_t*)c->s.img_a.p, width, height, pitch,
                               (const float*)c->s.kern.p, K, reflect_pad, (uint8_t*)c->s.img_b.p, wo));
  HIPCHK(c, hipMemcpyAsync(dst, c->s.img_b.p, (size_t)wo * ho, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

int orbx_conv2d(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, const float* kernel,
                int kernel_size, uint8_t* dst) {
  DeviceGuard _dg(c);
  return conv_stage(c, image, width, height, stride, kernel, kernel_size, 0, dst);
}

int orbx_gaussian_kernel(int kernel_size, float sigma, float* kernel) {
  return gaussian_kernel(kernel_size, sigma, kernel);
}

int orbx_gaussian_blur_conv(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int kernel_size,
                            uint8_t* dst) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (kernel_size < 1 || (kernel_size % 2) == 0 || kernel_size > 31)
    return fail(c, ORBX_ERR_INVALID_ARG, "kernel_size must be odd and <= 31 (src/GaussianBlur.cpp:8-11)");
  std::vector<float> g((size_t)kernel_size * kernel_size);
  gaussian_kernel(kernel_size, -1.0f, g.data());
  return conv_stage(c, image, width, height, stride, g.data(), kernel_size, 1, dst);
}

int orbx_sobel(orbx_ctx* c, const uint8_t* image, int width, int height, int stride, int dir, uint8_t* dst) {
  DeviceGuard _dg(c);
  static const float SX[9] = {-1.f, 0.f, 1.f, -2.f, 0.f, 2.f, -1.f, 0.f, 1.f};   // src/Sobel.cpp:6-10
  static const float SY[9] = {-1.f, -2.f, -1.f, 0.f, 0.f, 0.f, 1.f, 2.f, 1.f};   // src/Sobel.cpp:12-16
  return conv_stage(c, image, width, height, stride, dir == 0 ? SX : SY, 3, 1, dst);
}

int orbx_select_top(orbx_ctx* c, const float* responses, int n, int keep, int32_t* indices, int* kept) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (n < 0 || keep < 0 || (n > 0 && (!responses || !indices)) || !kept)
    return fail(c, ORBX_ERR_INVALID_ARG, "bad select_top arguments");
  const int m = std::min(n, keep);
  *kept = m;
  if (m == 0) return ORBX_OK;
  ENSURE(c, c->s.f32b, sizeof(float) * (size_t)n);
  ENSURE(c, c->s.i32, sizeof(int32_t) * (size_t)n);
  HIPCHK(c, hipMemcpyAsync(c->s.f32b.p, responses, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, orbx_launch_select_flat(c->stream, (const float*)c->s.f32b.p, n, keep, (int32_t*)c->s.i32.p));
  HIPCHK(c, hipMemcpyAsync(indices, c->s.i32.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ORBX_OK;
}

// ---- descriptor matching (next row) -----------------------------------------

// the host-array entry: the result block of one pair of nq slots, L = MatchBlock(1, nq), comes back whole in `r`
static int knn_host(orbx_ctx* c, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
                    double ratio, const MatchBlock& L, std::vector<int32_t>* r) {
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (nq < 0 || nt < 0 || (nq > 0 && !query) || (nt > 0 && !train))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad matcher arguments");
  if (nq == 0) return ORBX_OK;
  r->resize(L.bytes / sizeof(int32_t));
  const MatchInput I(nq, nt);
  DevBuf &in = c->m.in, &res = c->m.res;
  ENSURE(c, in, I.bytes);
  ENSURE(c, res, L.bytes);
  const int32_t cnt[2] = {nq, nt};
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(at<int32_t>(in, I.cnt), cnt, sizeof(cnt), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(at<orbx_descriptor>(in, I.q), query, sizeof(orbx_descriptor) * (size_t)nq, hipMemcpyHostToDevice, s));
  if (nt > 0)
    HIPCHK(c, hipMemcpyAsync(at<orbx_descriptor>(in, I.t), train, sizeof(orbx_descriptor) * (size_t)nt, hipMemcpyHostToDevice, s));
  HIPCHK(c, orbx_launch_knn2(s, 1, nq, at<orbx_descriptor>(in, I.q), at<int32_t>(in, I.cnt), 0,
                             at<orbx_descriptor>(in, I.t), at<int32_t>(in, I.cnt) + 1, 0, ratio, at<int32_t>(res, L.idx),
                             at<int32_t>(res, L.dist), at<int32_t>(res, L.match), 0));
  HIPCHK(c, hipMemcpyAsync(r->data(), res.p, L.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  c->m.pairs = 0;  // the block no longer holds a batch's matches
  return ORBX_OK;
}

static int compact_matches(orbx_ctx* c, const int32_t* match, const int32_t* dist2, int nq, int32_t* query_idx,
                           int32_t* train_idx, int32_t* dist1, int capacity, int* count) {
  int n = 0;
  for (int i = 0; i < nq; i++)
    if (match[i] >= 0) {
      if (n < capacity) {
        query_idx[n] = i;
        train_idx[n] = match[i];
        if (dist1) dist1[n] = dist2[2 * i];
      }
      n++;
    }
  *count = n;
  return n > capacity ? fail(c, ORBX_ERR_CAPACITY, "capacity smaller than match count") : (int)ORBX_OK;
}

int orbx_knn2(orbx_ctx* c, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
              int32_t* idx, int32_t* dist) {
  DeviceGuard _dg(c);
  if (c && nq > 0 && (!idx || !dist)) return fail(c, ORBX_ERR_INVALID_ARG, "idx/dist is NULL");
  const MatchBlock L(1, std::max(nq, 0));
  std::vector<int32_t> r;
  int st = knn_host(c, query, nq, train, nt, 0.8, L, &r);
  if (st != ORBX_OK) return st;
  if (nq > 0) {
    std::memcpy(idx, r.data() + L.idx / sizeof(int32_t), sizeof(int32_t) * 2 * (size_t)nq);
    std::memcpy(dist, r.data() + L.dist / sizeof(int32_t), sizeof(int32_t) * 2 * (size_t)nq);
  }
  return ORBX_OK;
}

int orbx_match_ratio(orbx_ctx* c, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
                     double ratio, int32_t* query_idx, int32_t* train_idx, int32_t* dist1, int capacity, int* count) {
  DeviceGuard _dg(c);
  if (c && (!count || capacity < 0 || (capacity > 0 && (!query_idx || !train_idx))))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad match output arguments");
  const MatchBlock L(1, std::max(nq, 0));
  std::vector<int32_t> r;
  int st = knn_host(c, query, nq, train, nt, ratio, L, &r);
  if (st != ORBX_OK) return st;
  return compact_matches(c, r.data() + L.match / sizeof(int32_t), r.data() + L.dist / sizeof(int32_t), nq, query_idx,
                         train_idx, dist1, capacity, count);
}

int orbx_batch_match_consecutive(orbx_ctx* c, double ratio) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  const Block& B = last_block(c);
  if (B.n < 2) return fail(c, ORBX_ERR_INVALID_ARG, "needs a batch of at least two frames");
  // the match block is ONE per context: a match of the other lane's batch may still be writing it
  if (c->lanes[1].stream) HIPCHK(c, lanes_sync(c));
  const int n = B.n, cap = B.cap;
  const MatchBlock L(n - 1, cap);
  DevBuf& res = c->m.res;
  ENSURE(c, res, L.bytes);
  const int32_t* counts = (const int32_t*)(B.d + B.layout.counts);
  const orbx_descriptor* desc = (const orbx_descriptor*)(B.d + B.layout.desc);
  hipStream_t s = batch_stream(c);
  // pair p: query = frame p, train = frame p+1 (same arrays, shifted by one slot block)
  HIPCHK(c, orbx_launch_knn2(s, n - 1, cap, desc, counts, (size_t)cap, desc + cap, counts + 1, (size_t)cap, ratio,
                             at<int32_t>(res, L.idx), at<int32_t>(res, L.dist), at<int32_t>(res, L.match), (size_t)cap));
  c->m.pairs = n - 1;
  c->m.cap = cap;
  c->m.serial = c->batch_serial;
  c->m.gen++;
  return ORBX_OK;
}

int orbx_batch_match_fetch(orbx_ctx* c, int pair, int32_t* query_idx, int32_t* train_idx, int32_t* dist1,
                           int capacity, int* count) {
  DeviceGuard _dg(c);
  if (!c) return ORBX_ERR_INVALID_ARG;
  if (!count || capacity < 0 || (capacity > 0 && (!query_idx || !train_idx)))
    return fail(c, ORBX_ERR_INVALID_ARG, "bad match output arguments");
  if (pair < 0 || pair >= c->m.pairs) return fail(c, ORBX_ERR_INVALID_ARG, "pair outside the last matched batch");
  const Block& B = last_block(c);
  const int cap = c->m.cap;
  const MatchBlock L(c->m.pairs, cap);
  hipStream_t s = batch_stream(c);
  int32_t nq = 0;
  std::vector<int32_t> vm((size_t)cap), vd((size_t)2 * cap);
  HIPCHK(c, hipMemcpyAsync(&nq, (const int32_t*)(B.d + B.layout.counts) + pair, sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(vm.data(), at<int32_t>(c->m.res, L.match) + (size_t)pair * cap, sizeof(int32_t) * cap,
                           hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(vd.data(), at<int32_t>(c->m.res, L.dist) + (size_t)2 * pair * cap, sizeof(int32_t) * 2 * cap,
                           hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  // (the rows are as wide as the matched batch's: a later batch's counts never reach past them)
  return compact_matches(c, vm.data(), vd.data(), std::min(nq, cap), query_idx, train_idx, dist1, capacity, count);
}

}  // extern "C"
