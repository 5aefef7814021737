// orb.hpp -- C++ host-side mirror of the reference's ORB interface, on top of
// the liborbx C ABI (include/orbx.h).  Header-only, C++17, no OpenCV needed.
//
// Same class / function names, constructor defaults, argument meaning and
// ownership as the reference, so code written against the reference headers
// keeps compiling after `#include "orb.hpp"` is pointed here:
//
//   reference                                   this header
//   ------------------------------------------  ---------------------------------
//   include/orb.hpp:4      struct Keypoint       Keypoint (layout == orbx_keypoint)
//   include/orb.hpp:6-8    struct ORBDescriptor  ORBDescriptor (== orbx_descriptor)
//   include/orb.hpp:10-22  class OrientedFAST    OrientedFAST
//   include/orb.hpp:24-32  class RotatedBRIEF    RotatedBRIEF
//   include/orb.hpp:34-49  class ORB             ORB
//   include/orb_cpu.hpp    *CPU twins            OrientedFASTCPU / RotatedBRIEFCPU / ORBCPU
//                                                (same GPU kernels, CPU-flavour semantics)
//   include/Fast.cuh:5-6   Fast, Orientations    Fast, Orientations
//   include/NMS.cuh:5      NMS                   NMS
//   include/HarrisScore.cuh:5  HarrisScore       HarrisScore
//   include/Brief.cuh:5    Brief                 Brief
//   include/Convolution.cuh:5  conv2d            conv2d
//   include/GaussianBlur.cuh:3-4  GaussianBlur, GaussianBlur1D
//   include/GaussianBlur.hpp:6  GaussianBlurCUDA GaussianBlurCUDA
//   include/Sobel.hpp:6    SobelCUDA             SobelCUDA
//
// Differences, all deliberate:
//   * images are passed as orbx::Image {data,width,height,stride}; a cv::Mat
//     overload set is enabled with -DORBX_WITH_OPENCV when OpenCV exists;
//   * ORB::detectAndCompute ASSIGNS its outputs like ORBCPU does
//     (orb_cpu.cpp:272-275) instead of appending (orb.cpp:100-102, D12);
//   * errors throw std::runtime_error (the reference prints and exit(1)s,
//     Fast.cu:8-18) and constructors print nothing;
//   * HarrisScore takes `float k` (the reference's `int k` truncates 0.04 to 0, D7).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/orbx.h"
#include "../../include/orbx_carry.h"
#include "../../include/orbx_lm.h"
#include "../../include/orbx_pnp.h"
#include "../../include/orbx_prior.h"
#include "../../include/orbx_reloc.h"
#include "../../include/orbx_search.h"
#include "../../include/orbx_stream.h"
#include "../../include/orbx_vo.h"

#ifdef ORBX_WITH_OPENCV
#include <opencv2/core.hpp>
#endif

struct Keypoint {
  int x, y;
};
struct ORBDescriptor {
  uint8_t data[32];
};
static_assert(sizeof(Keypoint) == sizeof(orbx_keypoint), "Keypoint layout");
static_assert(sizeof(ORBDescriptor) == sizeof(orbx_descriptor), "ORBDescriptor layout");

namespace orbx {

// 8-bit single-channel image view (what the reference passes as CV_8UC1 cv::Mat)
struct Image {
  const uint8_t* data = nullptr;
  int width = 0, height = 0, stride = 0;
  Image() = default;
  Image(const uint8_t* d, int w, int h, int s = 0) : data(d), width(w), height(h), stride(s ? s : w) {}
#ifdef ORBX_WITH_OPENCV
  Image(const cv::Mat& m) : data(m.data), width(m.cols), height(m.rows), stride((int)m.step) {  // NOLINT
    if (m.type() != CV_8UC1) throw std::runtime_error("orbx: image must be CV_8UC1");  // CV_Assert, orb_cpu.cpp:26
  }
#endif
};

// owned 8-bit image (what the reference returns in a cv::Mat `dst`)
struct Image8 {
  std::vector<uint8_t> pixels;
  int width = 0, height = 0;
  Image view() const { return Image(pixels.data(), width, height, width); }
};

namespace detail {

inline void check(orbx_ctx* c, int st, const char* what) {
  if (st != ORBX_OK)
    throw std::runtime_error(std::string(what) + ": " + orbx_status_string(st) + ": " + orbx_last_error_string(c));
}

// A context that grows with the largest image it has seen (the reference
// allocates per call; here device memory is owned by the object).
class Ctx {
 public:
  explicit Ctx(const orbx_params& p) : p_(p) {}
  ~Ctx() { orbx_destroy(c_); }
  Ctx(const Ctx&) = delete;
  Ctx& operator=(const Ctx&) = delete;
  orbx_ctx* get(int w, int h) {
    if (!c_ || w > p_.max_width || h > p_.max_height) {
      orbx_destroy(c_);
      c_ = nullptr;
      p_.max_width = w > p_.max_width ? w : p_.max_width;
      p_.max_height = h > p_.max_height ? h : p_.max_height;
      check(nullptr, orbx_create(&p_, &c_), "orbx_create");
    }
    return c_;
  }
  const orbx_params& params() const { return p_; }

 private:
  orbx_params p_;
  orbx_ctx* c_ = nullptr;
};

inline orbx_params gpu_defaults() {
  orbx_params p;
  orbx_params_default_gpu(&p);
  p.max_width = 8;
  p.max_height = 8;
  return p;
}
inline orbx_params cpu_defaults() {
  orbx_params p;
  orbx_params_default_cpu(&p);
  p.max_width = 8;
  p.max_height = 8;
  return p;
}
inline std::shared_ptr<Ctx>& stage_ctx() {  // shared by the free stage functions, the matcher and the tracker
  static std::shared_ptr<Ctx> c = [] {
    orbx_params p = gpu_defaults();
    p.nlevels = 1;  // the stage operators work on single images: any size >= 8x8 is a valid plan
    return std::make_shared<Ctx>(p);
  }();
  return c;
}
inline orbx_keypoint* kp(std::vector<Keypoint>& v) { return reinterpret_cast<orbx_keypoint*>(v.data()); }
inline const orbx_keypoint* kp(const std::vector<Keypoint>& v) {
  return reinterpret_cast<const orbx_keypoint*>(v.data());
}
inline orbx_descriptor* ds(std::vector<ORBDescriptor>& v) { return reinterpret_cast<orbx_descriptor*>(v.data()); }

}  // namespace detail
}  // namespace orbx

// ---- free stage functions (reference: include/*.cuh, *.hpp) -----------------

// Fast.cuh:5 -- returns the keypoint count; `keypoints` is resized to it.
inline int Fast(const orbx::Image& image, std::vector<Keypoint>& keypoints, int threshold, int n, int nms_window,
                int nfeatures) {
  orbx_ctx* c = orbx::detail::stage_ctx()->get(image.width, image.height);
  keypoints.resize(nfeatures > 0 ? nfeatures : 0);
  int count = 0;
  orbx::detail::check(c,
                      orbx_fast(c, image.data, image.width, image.height, image.stride, threshold, n, nms_window,
                                nfeatures, orbx::detail::kp(keypoints), &count, nullptr),
                      "Fast");
  keypoints.resize(count);
  return count;
}

// Fast.cuh:6
inline void Orientations(const orbx::Image& image, const std::vector<Keypoint>& keypoints,
                         std::vector<float>& orientations, int patch_size) {
  orbx_ctx* c = orbx::detail::stage_ctx()->get(image.width, image.height);
  orientations.assign(keypoints.size(), 0.0f);
  orbx::detail::check(c,
                      orbx_orientations(c, image.data, image.width, image.height, image.stride,
                                        orbx::detail::kp(keypoints), (int)keypoints.size(), patch_size,
                                        orientations.data()),
                      "Orientations");
}

// NMS.cuh:5 -- `scores` is a width*height float map (CV_32F in the reference)
inline void NMS(const float* scores, int width, int height, std::vector<Keypoint>& keypoints, int nms_window,
                int nfeatures, float threshold) {
  orbx_ctx* c = orbx::detail::stage_ctx()->get(width < 8 ? 8 : width, height < 8 ? 8 : height);
  keypoints.resize(nfeatures > 0 ? nfeatures : 0);
  int count = 0;
  orbx::detail::check(
      c, orbx_nms(c, scores, width, height, nms_window, nfeatures, threshold, orbx::detail::kp(keypoints), &count, nullptr),
      "NMS");
  keypoints.resize(count);
}

// HarrisScore.cuh:5
inline void HarrisScore(const orbx::Image& image, std::vector<Keypoint>& keypoints, std::vector<float>& harris_scores,
                        int corner_window, float k) {
  orbx_ctx* c = orbx::detail::stage_ctx()->get(image.width, image.height);
  harris_scores.assign(keypoints.size(), 0.0f);
  orbx::detail::check(c,
                      orbx_harris(c, image.data, image.width, image.height, image.stride, orbx::detail::kp(keypoints),
                                  (int)keypoints.size(), corner_window, k, harris_scores.data()),
                      "HarrisScore");
}

// Brief.cuh:5 -- n_bits must be 256 and patch_size 31, as in the reference
inline void Brief(const orbx::Image& image, const std::vector<Keypoint>& keypoints,
                  const std::vector<float>& orientations, std::vector<ORBDescriptor>& descriptors, int n_bits = 256,
                  int patch_size = 31) {
  if (n_bits != 256 || patch_size != 31) throw std::runtime_error("Brief: only n_bits=256, patch_size=31 exist");
  if (orientations.size() != keypoints.size()) throw std::runtime_error("Brief: size mismatch");
  orbx_ctx* c = orbx::detail::stage_ctx()->get(image.width, image.height);
  descriptors.assign(keypoints.size(), ORBDescriptor{});
  orbx::detail::check(c,
                      orbx_brief(c, image.data, image.width, image.height, image.stride, orbx::detail::kp(keypoints),
                                 orientations.data(), (int)keypoints.size(), orbx::detail::ds(descriptors)),
                      "Brief");
}

// Convolution.cuh:5 -- `image` is pre-padded; dst is (h-K+1) x (w-K+1)
inline void conv2d(const orbx::Image& image, orbx::Image8& dst, const float* kernel, int kernel_size) {
  orbx_ctx* c = orbx::detail::stage_ctx()->get(image.width, image.height);
  dst.width = image.width - kernel_size + 1;
  dst.height = image.height - kernel_size + 1;
  if (dst.width < 1 || dst.height < 1) throw std::runtime_error("conv2d: image smaller than kernel");
  dst.pixels.assign((size_t)dst.width * dst.height, 0);
  orbx::detail::check(
      c, orbx_conv2d(c, image.data, image.width, image.height, image.stride, kernel, kernel_size, dst.pixels.data()),
      "conv2d");
}

namespace orbx::detail {
template <class F>
inline void same_size_stage(const Image& image, Image8& dst, const char* what, F&& call) {
  orbx_ctx* c = stage_ctx()->get(image.width, image.height);
  dst.width = image.width;
  dst.height = image.height;
  dst.pixels.assign((size_t)dst.width * dst.height, 0);
  check(c, call(c), what);
}
}  // namespace orbx::detail

// GaussianBlur.cuh:3 (5x5 /273)
inline void GaussianBlur(const orbx::Image& image, orbx::Image8& dst) {
  orbx::detail::same_size_stage(image, dst, "GaussianBlur", [&](orbx_ctx* c) {
    return orbx_blur5_273(c, image.data, image.width, image.height, image.stride, dst.pixels.data(), dst.width);
  });
}
// GaussianBlur.cuh:4 (separable [1 4 6 4 1]/16)
inline void GaussianBlur1D(const orbx::Image& image, orbx::Image8& dst) {
  orbx::detail::same_size_stage(image, dst, "GaussianBlur1D", [&](orbx_ctx* c) {
    return orbx_blur5_sep(c, image.data, image.width, image.height, image.stride, dst.pixels.data(), dst.width);
  });
}
// GaussianBlur.hpp:6
inline void GaussianBlurCUDA(const orbx::Image& image, orbx::Image8& dst, int kernel_size) {
  orbx::detail::same_size_stage(image, dst, "GaussianBlurCUDA", [&](orbx_ctx* c) {
    return orbx_gaussian_blur_conv(c, image.data, image.width, image.height, image.stride, kernel_size,
                                   dst.pixels.data());
  });
}
// Sobel.hpp:6
inline void SobelCUDA(const orbx::Image& image, orbx::Image8& dst, int dir) {
  orbx::detail::same_size_stage(image, dst, "SobelCUDA", [&](orbx_ctx* c) {
    return orbx_sobel(c, image.data, image.width, image.height, image.stride, dir, dst.pixels.data());
  });
}

// ---- classes (reference: include/orb.hpp, include/orb_cpu.hpp) ---------------

class OrientedFAST {
 public:
  OrientedFAST(int threshold = 20, int n = 9, int nms_window = 3, int patch_size = 31)
      : threshold(threshold), n(n), nms_window(nms_window), patch_size(patch_size) {}
  // orb.cpp:22-27
  std::vector<Keypoint> detect(const orbx::Image& image, int nfeatures) {
    std::vector<Keypoint> keypoints;
    Fast(image, keypoints, threshold, n, nms_window, nfeatures);
    return keypoints;
  }
  // orb.cpp:29-33
  std::vector<float> compute_orientations(const orbx::Image& image, const std::vector<Keypoint>& keypoints) {
    std::vector<float> orientations;
    Orientations(image, keypoints, orientations, patch_size);
    return orientations;
  }

 private:
  int threshold, n, nms_window, patch_size;
};

class RotatedBRIEF {
 public:
  RotatedBRIEF() = default;
  // orb.cpp:40-44
  std::vector<ORBDescriptor> compute(const orbx::Image& image, const std::vector<Keypoint>& keypoints,
                                     const std::vector<float>& orientations) {
    std::vector<ORBDescriptor> descriptors;
    Brief(image, keypoints, orientations, descriptors, n_bits, patch_size);
    return descriptors;
  }

 private:
  int n_bits = 256;
  int patch_size = 31;
};

class ORB {
 public:
  // orb.hpp:36; the FAST/Harris knobs the reference hard-codes are exposed through params()
  ORB(int nfeatures = 500, float scaleFactor = 1.2f, int nlevels = 8) : ctx_(make(nfeatures, scaleFactor, nlevels)) {}
  explicit ORB(const orbx_params& p) : ctx_(std::make_shared<orbx::detail::Ctx>(p)) {}

  // orb.hpp:37 / orb.cpp:58-109.  Outputs are assigned (not appended).
  void detectAndCompute(const orbx::Image& image, std::vector<Keypoint>& keypoints, std::vector<float>& orientations,
                        std::vector<ORBDescriptor>& descriptors) {
    detectAndCompute(image, keypoints, orientations, descriptors, nullptr, nullptr);
  }
  // extended form: Harris responses and pyramid level per keypoint
  void detectAndCompute(const orbx::Image& image, std::vector<Keypoint>& keypoints, std::vector<float>& orientations,
                        std::vector<ORBDescriptor>& descriptors, std::vector<float>* responses,
                        std::vector<int32_t>* levels) {
    orbx_ctx* c = ctx_->get(image.width, image.height);
    int32_t cap = 0;
    orbx::detail::check(c, orbx_get_plan(c, image.width, image.height, nullptr, nullptr, nullptr, nullptr, nullptr, &cap),
                        "orbx_get_plan");
    if (cap < 1) cap = 1;
    keypoints.resize(cap);
    orientations.resize(cap);
    descriptors.resize(cap);
    if (responses) responses->resize(cap);
    if (levels) levels->resize(cap);
    int count = 0;
    orbx::detail::check(c,
                        orbx_detect_and_compute(c, image.data, image.width, image.height, image.stride,
                                                orbx::detail::kp(keypoints), orientations.data(),
                                                orbx::detail::ds(descriptors), responses ? responses->data() : nullptr,
                                                levels ? levels->data() : nullptr, nullptr, cap, &count),
                        "ORB::detectAndCompute");
    keypoints.resize(count);
    orientations.resize(count);
    descriptors.resize(count);
    if (responses) responses->resize(count);
    if (levels) levels->resize(count);
  }
  // descriptors at points the caller holds (include/orbx_reloc.h): n (x, y) pairs described at
  // level 0 under this object's parameters; angles in radians, states orbx_pd_state.  Outputs are assigned.
  void describePoints(const orbx::Image& image, const float* points_xy, int n, std::vector<float>& orientations,
                      std::vector<ORBDescriptor>& descriptors, std::vector<int32_t>& states) {
    orbx_ctx* c = ctx_->get(image.width, image.height);
    orientations.assign((size_t)n, 0.f);
    descriptors.assign((size_t)n, ORBDescriptor{});
    states.assign((size_t)n, (int32_t)ORBX_PD_NONE);
    orbx::detail::check(c,
                        orbx_describe_points(c, image.data, image.width, image.height, image.stride, points_xy, n,
                                             orientations.data(), orbx::detail::ds(descriptors), states.data()),
                        "ORB::describePoints");
  }
  const orbx_params& params() const { return ctx_->params(); }

 private:
  static std::shared_ptr<orbx::detail::Ctx> make(int nfeatures, float sf, int nlevels) {
    orbx_params p = orbx::detail::gpu_defaults();
    p.nfeatures = nfeatures;
    p.scale_factor = sf;
    p.nlevels = nlevels;
    return std::make_shared<orbx::detail::Ctx>(p);
  }
  std::shared_ptr<orbx::detail::Ctx> ctx_;
};

// ---- CPU-flavour twins (include/orb_cpu.hpp): same kernels, CPU semantics ----

class OrientedFASTCPU {
 public:
  OrientedFASTCPU(int nfeatures = 3000, int threshold = 50, int n = 9, int nms_window = 3, int patch_size = 9)
      : nfeatures(nfeatures), threshold(threshold), n(n), nms_window(nms_window), patch_size(patch_size) {}
  std::vector<Keypoint> detect(const orbx::Image& image) {  // orb_cpu.cpp:23-137
    std::vector<Keypoint> keypoints;
    Fast(image, keypoints, threshold, n, nms_window, nfeatures);
    return keypoints;
  }
  std::vector<float> compute_orientations(const orbx::Image& image, const std::vector<Keypoint>& keypoints) {
    std::vector<float> o;  // orb_cpu.cpp:139-183
    Orientations(image, keypoints, o, patch_size);
    return o;
  }

 private:
  int nfeatures, threshold, n, nms_window, patch_size;
};

using RotatedBRIEFCPU = RotatedBRIEF;  // orb_cpu.cpp:185-258: identical arithmetic

class ORBCPU {
 public:
  // orb_cpu.hpp:30; like the reference, nfeatures/scaleFactor/nlevels are
  // accepted and ignored (orb_cpu.cpp:271-276 runs one level with the
  // OrientedFASTCPU defaults, D16)
  ORBCPU(int = 500, float = 1.2f, int = 8) : orb_(orbx::detail::cpu_defaults()) {}
  void detectAndCompute(const orbx::Image& image, std::vector<Keypoint>& keypoints, std::vector<float>& orientations,
                        std::vector<ORBDescriptor>& descriptors) {
    orb_.detectAndCompute(image, keypoints, orientations, descriptors);
  }

 private:
  ORB orb_;
};

// ---- descriptor matching (next row: src/feature_matching.cpp:166-181) ---------
// Call shape of cv::DescriptorMatcher::knnMatch(des1, des2, matches, 2) as used by
// VisualOdom::get_matches; exact brute-force Hamming instead of FLANN's LSH.

struct DMatch {  // cv::DMatch
  int queryIdx = -1, trainIdx = -1;
  float distance = 0.f;
};

class HammingMatcher {
 public:
  HammingMatcher() : ctx_(orbx::detail::stage_ctx()) {}
  // matches[i] holds up to k (= 2) neighbours of des1[i], best first
  void knnMatch(const std::vector<ORBDescriptor>& des1, const std::vector<ORBDescriptor>& des2,
                std::vector<std::vector<DMatch>>& matches, int k = 2) {
    if (k != 2) throw std::runtime_error("HammingMatcher::knnMatch: only k = 2 (the reference's call) exists");
    orbx_ctx* c = ctx_->get(8, 8);
    std::vector<int32_t> idx(2 * des1.size()), dist(2 * des1.size());
    orbx::detail::check(c,
                        orbx_knn2(c, reinterpret_cast<const orbx_descriptor*>(des1.data()), (int)des1.size(),
                                  reinterpret_cast<const orbx_descriptor*>(des2.data()), (int)des2.size(), idx.data(),
                                  dist.data()),
                        "knnMatch");
    matches.assign(des1.size(), {});
    for (size_t i = 0; i < des1.size(); i++)
      for (int j = 0; j < 2; j++)
        if (idx[2 * i + j] >= 0) matches[i].push_back(DMatch{(int)i, idx[2 * i + j], (float)dist[2 * i + j]});
  }
  // knnMatch + `m.distance < ratio * n.distance` (feature_matching.cpp:172-181), in one device pass
  std::vector<DMatch> ratioMatch(const std::vector<ORBDescriptor>& des1, const std::vector<ORBDescriptor>& des2,
                                 double ratio = 0.8) {
    orbx_ctx* c = ctx_->get(8, 8);
    std::vector<int32_t> qi(des1.size()), ti(des1.size()), d1(des1.size());
    int n = 0;
    orbx::detail::check(c,
                        orbx_match_ratio(c, reinterpret_cast<const orbx_descriptor*>(des1.data()), (int)des1.size(),
                                         reinterpret_cast<const orbx_descriptor*>(des2.data()), (int)des2.size(), ratio,
                                         qi.data(), ti.data(), d1.data(), (int)des1.size(), &n),
                        "ratioMatch");
    std::vector<DMatch> out(n);
    for (int i = 0; i < n; i++) out[i] = DMatch{qi[i], ti[i], (float)d1[i]};
    return out;
  }

 private:
  std::shared_ptr<orbx::detail::Ctx> ctx_;
};

// ---- cv::Feature2D-shaped adapter (next row) ---------------
// What the VO executables hold is a `cv::Ptr<cv::Feature2D>` (`cv::ORB::create(3000)`,
// src/feature_tracking.cpp:31) on which they call `detectAndCompute(img, cv::noArray(),
// kp, des)` (src/feature_matching.cpp:164, src/feature_tracking.cpp:201) and `detect(img,
// kp)` (src/feature_tracking.cpp:61), and of whose results they read `kp.pt` and an
// N x 32 CV_8U descriptor matrix (src/feature_matching.cpp:179-180).  orbx::Feature2D gives
// this front-end that call shape; orbx::KeyPoint carries the cv::KeyPoint fields with the
// conventions cv::ORB uses for them (size = patch size x level scale, angle in degrees in
// [0, 360), response = Harris response, octave = pyramid level).  With -DORBX_WITH_OPENCV
// the cv::KeyPoint / cv::Mat overloads make it a literal replacement.
namespace orbx {

struct Point2f {  // cv::Point2f
  float x = 0.f, y = 0.f;
};

struct KeyPoint {  // cv::KeyPoint
  Point2f pt;
  float size = 0.f;
  float angle = -1.f;  // degrees, [0, 360); -1 = not computed (detect())
  float response = 0.f;
  int octave = 0;
  int class_id = -1;
  // cv::KeyPoint::convert(kp1, pts1), src/feature_tracking.cpp:62
  static void convert(const std::vector<KeyPoint>& keypoints, std::vector<Point2f>& points2f) {
    points2f.resize(keypoints.size());
    for (size_t i = 0; i < keypoints.size(); i++) points2f[i] = keypoints[i].pt;
  }
};

// N x 32 CV_8U descriptor matrix (row i = descriptor of keypoint i)
struct DescriptorMat {
  int rows = 0;
  static constexpr int cols = 32;
  std::vector<ORBDescriptor> d;
  const uint8_t* ptr(int r) const { return d[(size_t)r].data; }
  const uint8_t* data() const { return d.empty() ? nullptr : d[0].data; }  // rows x 32 contiguous bytes
  bool empty() const { return rows == 0; }
};

inline float angle_degrees(float radians) {  // atan2f's (-pi, pi] -> cv::KeyPoint's [0, 360)
  float a = radians * 57.29577951308232f;
  if (a < 0.f) a += 360.f;
  if (a >= 360.f) a -= 360.f;
  return a;
}

class Feature2D {
 public:
  // cv::ORB::create(nfeatures, scaleFactor, nlevels), src/feature_tracking.cpp:31
  static std::shared_ptr<Feature2D> create(int nfeatures = 500, float scaleFactor = 1.2f, int nlevels = 8) {
    return std::shared_ptr<Feature2D>(new Feature2D(::ORB(nfeatures, scaleFactor, nlevels)));
  }
  static std::shared_ptr<Feature2D> create(const orbx_params& p) {
    return std::shared_ptr<Feature2D>(new Feature2D(::ORB(p)));
  }
  // orb->detectAndCompute(img, cv::noArray(), kp, des); a mask is not supported (the
  // reference never passes one)
  void detectAndCompute(const Image& image, std::vector<KeyPoint>& keypoints, DescriptorMat& descriptors) {
    run(image, keypoints, &descriptors);
  }
  // orb->detect(img, kp)
  void detect(const Image& image, std::vector<KeyPoint>& keypoints) { run(image, keypoints, nullptr); }
  // orb->compute(img, kp, des), cv::Feature2D::compute's contract: keypoints that cannot be described (their state
  // is not ORBX_PD_OK: not finite, outside the image or closer than max(patch_size / 2, 20) to a border) are REMOVED,
  // the rest keep their order, `angle` is filled in degrees and row i of `descriptors` belongs to keypoint i.  The
  // octaves are ignored: every keypoint is described at level 0, at pt rounded to the nearest pixel (ties to even),
  // as include/orbx_reloc.h states.  The reference computes with the detection, src/feature_tracking.cpp:201
  void compute(const Image& image, std::vector<KeyPoint>& keypoints, DescriptorMat& descriptors) {
    static_assert(sizeof(Point2f) == 2 * sizeof(float), "point layout");
    std::vector<Point2f> pts;
    KeyPoint::convert(keypoints, pts);
    std::vector<int32_t> states;
    orb_.describePoints(image, pts.empty() ? nullptr : &pts[0].x, (int)pts.size(), angles_, desc_, states);
    size_t kept = 0;
    descriptors.d.clear();
    for (size_t i = 0; i < keypoints.size(); i++) {
      if (states[i] != ORBX_PD_OK) continue;
      keypoints[kept] = keypoints[i];
      keypoints[kept].angle = angle_degrees(angles_[i]);
      descriptors.d.push_back(desc_[i]);
      kept++;
    }
    keypoints.resize(kept);
    descriptors.rows = (int)kept;
  }
  int descriptorSize() const { return 32; }
  const orbx_params& params() const { return orb_.params(); }

#ifdef ORBX_WITH_OPENCV
  void detectAndCompute(const cv::Mat& image, cv::InputArray /*mask = cv::noArray()*/,
                        std::vector<cv::KeyPoint>& keypoints, cv::Mat& descriptors) {
    std::vector<KeyPoint> k;
    DescriptorMat d;
    run(Image(image), k, &d);
    to_cv(k, keypoints);
    descriptors.create((int)k.size(), 32, CV_8U);
    if (!k.empty()) std::memcpy(descriptors.data, d.data(), k.size() * 32);
  }
  void detect(const cv::Mat& image, std::vector<cv::KeyPoint>& keypoints) {
    std::vector<KeyPoint> k;
    run(Image(image), k, nullptr);
    to_cv(k, keypoints);
  }
#endif

 private:
  explicit Feature2D(::ORB orb) : orb_(std::move(orb)) {}
  void run(const Image& image, std::vector<KeyPoint>& keypoints, DescriptorMat* descriptors) {
    orb_.detectAndCompute(image, kps_, angles_, desc_, &resp_, &levels_);
    const orbx_params& p = orb_.params();
    keypoints.resize(kps_.size());
    for (size_t i = 0; i < kps_.size(); i++) {
      KeyPoint& k = keypoints[i];
      k.pt.x = (float)kps_[i].x;
      k.pt.y = (float)kps_[i].y;
      k.octave = levels_[i];
      k.size = (float)p.patch_size * (float)std::pow((double)p.scale_factor, (double)levels_[i]);
      k.angle = descriptors ? angle_degrees(angles_[i]) : -1.f;
      k.response = resp_[i];
      k.class_id = -1;
    }
    if (descriptors) {
      descriptors->rows = (int)desc_.size();
      descriptors->d = desc_;
    }
  }
#ifdef ORBX_WITH_OPENCV
  static void to_cv(const std::vector<KeyPoint>& k, std::vector<cv::KeyPoint>& out) {
    out.resize(k.size());
    for (size_t i = 0; i < k.size(); i++)
      out[i] = cv::KeyPoint(k[i].pt.x, k[i].pt.y, k[i].size, k[i].angle, k[i].response, k[i].octave, k[i].class_id);
  }
#endif
  ::ORB orb_;
  std::vector<Keypoint> kps_;
  std::vector<float> angles_, resp_;
  std::vector<ORBDescriptor> desc_;
  std::vector<int32_t> levels_;
};

// ---- descriptors at held points and the re-association by descriptor -----------------------
// The device half of the reference's ORB + matcher fallback below 150 tracks (src/feature_tracking.cpp:68-71,
// :203-219), on host arrays: describe_points describes `points` on `image` at level 0 under the stage context's
// parameters (the GPU defaults: patch 31, no blur), reassociate joins two described sets -- only ORBX_PD_OK slots take
// part, ratio test, distance gate, and with `unique` one query per train slot -- into origin[q] = the train slot or
// -1, the array orbx::localise_carried_window takes as `origin`.
struct PointDescriptors {
  std::vector<float> angle;             // radians; 0 where the state is not ORBX_PD_OK
  std::vector<ORBDescriptor> desc;      // zeros where the state is not ORBX_PD_OK
  std::vector<int32_t> state;           // an orbx_pd_state per point
};
inline PointDescriptors describe_points(const Image& image, const std::vector<Point2f>& points) {
  static_assert(sizeof(Point2f) == 2 * sizeof(float), "point layout");
  const int n = (int)points.size();
  PointDescriptors out;
  out.angle.assign((size_t)n, 0.f);
  out.desc.assign((size_t)n, ORBDescriptor{});
  out.state.assign((size_t)n, (int32_t)ORBX_PD_NONE);
  orbx_ctx* c = detail::stage_ctx()->get(image.width, image.height);
  detail::check(c,
                orbx_describe_points(c, image.data, image.width, image.height, image.stride,
                                     n > 0 ? &points[0].x : nullptr, n, out.angle.data(), detail::ds(out.desc),
                                     out.state.data()),
                "orbx_describe_points");
  return out;
}
struct Reassociation {
  std::vector<int32_t> origin, dist;  // per query: the train slot and the Hamming distance to it, or -1
  int32_t count = 0;
};
inline Reassociation reassociate(const PointDescriptors& query, const PointDescriptors& train, double ratio = 0.8,
                                 int max_distance = 256, bool unique = true) {
  if (query.desc.size() != query.state.size() || train.desc.size() != train.state.size())
    throw std::invalid_argument("reassociate: desc and state differ in size");
  const int nq = (int)query.desc.size(), nt = (int)train.desc.size();
  Reassociation out;
  out.origin.assign((size_t)nq, -1);
  out.dist.assign((size_t)nq, -1);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_reassociate(c, nq > 0 ? reinterpret_cast<const orbx_descriptor*>(query.desc.data()) : nullptr,
                                 nq > 0 ? query.state.data() : nullptr, nq,
                                 nt > 0 ? reinterpret_cast<const orbx_descriptor*>(train.desc.data()) : nullptr,
                                 nt > 0 ? train.state.data() : nullptr, nt, ratio, max_distance, unique ? 1 : 0,
                                 out.origin.data(), out.dist.data(), &out.count),
                "orbx_reassociate");
  return out;
}

// VisualOdom::get_matches (src/feature_matching.cpp:155-183): detect + describe frame 2,
// 2-NN match frame 1 -> 2, keep `m.distance < 0.8 * n.distance`, return the matched points.
inline void get_matches(Feature2D& orb, HammingMatcher& matcher, const std::vector<KeyPoint>& kp1,
                        const DescriptorMat& des1, const Image& img2, std::vector<KeyPoint>& kp2, DescriptorMat& des2,
                        std::vector<Point2f>& pts1, std::vector<Point2f>& pts2) {
  orb.detectAndCompute(img2, kp2, des2);
  std::vector<std::vector<DMatch>> matches;
  matcher.knnMatch(des1.d, des2.d, matches, 2);
  pts1.clear();
  pts2.clear();
  for (size_t i = 0; i < matches.size(); i++) {
    if (matches[i].size() < 2) continue;
    const DMatch& m = matches[i][0];
    const DMatch& n = matches[i][1];
    if (m.distance < 0.8 * n.distance) {
      pts1.push_back(kp1[(size_t)m.queryIdx].pt);
      pts2.push_back(kp2[(size_t)m.trainIdx].pt);
    }
  }
}

// ---- pyramidal Lucas-Kanade tracking (next row) ---------------
// cv::calcOpticalFlowPyrLK(img1, img2, pts1, pts2, status, err, cv::Size(21,21), 3,
//     cv::TermCriteria(COUNT + EPS, 30, 0.01))                 src/feature_tracking.cpp:175-181
struct Size {  // cv::Size
  int width = 21, height = 21;
  Size() = default;
  Size(int w, int h) : width(w), height(h) {}
};
struct TermCriteria {  // cv::TermCriteria(COUNT + EPS, maxCount, epsilon)
  int maxCount = 30;
  double epsilon = 0.01;
  TermCriteria() = default;
  TermCriteria(int count, double eps) : maxCount(count), epsilon(eps) {}
};

class LKTracker {
 public:
  // the tracker owns its context: the pyramid of the previous frame is cached in it, and a free stage
  // function called on a larger image re-creates the shared stage context (which would drop that cache)
  LKTracker() : ctx_([] {
    orbx_params p = detail::gpu_defaults();
    p.nlevels = 1;
    return std::make_shared<detail::Ctx>(p);
  }()) {}
  // prevImg == nullptr: the previous call's nextImg is this call's prevImg (its pyramid is still on the
  // device): the `img1 = img2.clone()` of the reference's loop, src/feature_tracking.cpp:112
  void calcOpticalFlowPyrLK(const Image* prevImg, const Image& nextImg, const std::vector<Point2f>& prevPts,
                            std::vector<Point2f>& nextPts, std::vector<uint8_t>& status, std::vector<float>& err,
                            Size winSize = Size(21, 21), int maxLevel = 3, TermCriteria criteria = TermCriteria()) {
    if (winSize.width != winSize.height) throw std::runtime_error("calcOpticalFlowPyrLK: square windows only");
    if (prevImg && (prevImg->width != nextImg.width || prevImg->height != nextImg.height))
      throw std::runtime_error("calcOpticalFlowPyrLK: image sizes differ");
    orbx_ctx* c = ctx_->get(nextImg.width, nextImg.height);
    const int n = (int)prevPts.size();
    nextPts.resize(prevPts.size());
    status.resize(prevPts.size());
    err.resize(prevPts.size());
    detail::check(c,
                  orbx_lk_track(c, prevImg ? prevImg->data : nullptr, prevImg ? prevImg->stride : 0, nextImg.data,
                                nextImg.stride, nextImg.width, nextImg.height,
                                reinterpret_cast<const float*>(prevPts.data()), n,
                                reinterpret_cast<float*>(nextPts.data()), status.data(), err.data(), winSize.width,
                                maxLevel, criteria.maxCount, criteria.epsilon),
                  "calcOpticalFlowPyrLK");
  }

  // trackPointsAcrossWindow's tracking (src/with_bundle_adjustment.cpp:464-499) in ONE launch: pts0 of imgs[0]
  // followed through imgs[1], imgs[2], ...  tracks: pts0.size() x imgs.size() points (entry 0: the input point),
  // seen: frames each point was observed in, err: pts0.size() x (imgs.size() - 1); zero past `seen`.  The pairs are
  // computed as calcOpticalFlowPyrLK computes them; the cached pyramid of the per-pair calls is left alone.
  void trackWindow(const std::vector<Image>& imgs, const std::vector<Point2f>& pts0, std::vector<Point2f>& tracks,
                   std::vector<int32_t>& seen, std::vector<float>& err, Size winSize = Size(21, 21), int maxLevel = 3,
                   TermCriteria criteria = TermCriteria()) {
    trackWindowImpl(imgs, pts0, tracks, seen, err, nullptr, nullptr, nullptr, winSize, maxLevel, criteria);
  }
  // The same with the forward-backward check, still ONE launch: every pair is tracked forward
  // and back again, and a track ends with the first pair whose return lies farther than fbThreshold from its start.
  // fbD2: pts0.size() x (imgs.size() - 1) squared return distances of the pairs that passed, lost: why each track
  // ended (0: alive through the window, 1: forward pass, 2: backward pass, 3: distance).
  void trackWindow(const std::vector<Image>& imgs, const std::vector<Point2f>& pts0, float fbThreshold,
                   std::vector<Point2f>& tracks, std::vector<int32_t>& seen, std::vector<float>& err,
                   std::vector<float>& fbD2, std::vector<int32_t>& lost, Size winSize = Size(21, 21), int maxLevel = 3,
                   TermCriteria criteria = TermCriteria()) {
    trackWindowImpl(imgs, pts0, tracks, seen, err, &fbThreshold, &fbD2, &lost, winSize, maxLevel, criteria);
  }

 private:
  void trackWindowImpl(const std::vector<Image>& imgs, const std::vector<Point2f>& pts0, std::vector<Point2f>& tracks,
                       std::vector<int32_t>& seen, std::vector<float>& err, const float* fbThreshold,
                       std::vector<float>* fbD2, std::vector<int32_t>* lost, Size winSize, int maxLevel,
                       TermCriteria criteria) {
    if (winSize.width != winSize.height) throw std::runtime_error("trackWindow: square windows only");
    if (imgs.size() < 2) throw std::runtime_error("trackWindow: a window has at least two frames");
    const int w = imgs[0].width, h = imgs[0].height, nf = (int)imgs.size(), n = (int)pts0.size();
    // the frames side by side in one allocation (the entry takes one base address and a frame stride)
    std::vector<uint8_t> packed((size_t)w * h * nf);
    for (int f = 0; f < nf; f++) {
      if (imgs[(size_t)f].width != w || imgs[(size_t)f].height != h)
        throw std::runtime_error("trackWindow: image sizes differ");
      for (int y = 0; y < h; y++)
        std::memcpy(packed.data() + ((size_t)f * h + y) * w, imgs[(size_t)f].data + (size_t)y * imgs[(size_t)f].stride,
                    (size_t)w);
    }
    orbx_ctx* c = ctx_->get(w, h);
    tracks.assign((size_t)n * nf, Point2f());
    seen.assign((size_t)n, 0);
    err.assign((size_t)n * (nf - 1), 0.f);
    if (!fbThreshold) {
      detail::check(c,
                    orbx_lk_track_window(c, packed.data(), nf, w, h, w, (size_t)w * h,
                                         reinterpret_cast<const float*>(pts0.data()), n,
                                         reinterpret_cast<float*>(tracks.data()), seen.data(), err.data(),
                                         winSize.width, maxLevel, criteria.maxCount, criteria.epsilon),
                    "trackWindow");
      return;
    }
    fbD2->assign((size_t)n * (nf - 1), 0.f);
    lost->assign((size_t)n, 0);
    detail::check(c,
                  orbx_lk_track_window_fb(c, packed.data(), nf, w, h, w, (size_t)w * h,
                                          reinterpret_cast<const float*>(pts0.data()), n,
                                          reinterpret_cast<float*>(tracks.data()), seen.data(), err.data(),
                                          winSize.width, maxLevel, criteria.maxCount, criteria.epsilon, *fbThreshold,
                                          fbD2->data(), lost->data()),
                  "trackWindow");
  }

  std::shared_ptr<detail::Ctx> ctx_;
};

// VisualOdom::track_optical_flow (src/feature_tracking.cpp:166-193): track pts1 into img2, drop lost tracks
inline void track_optical_flow(LKTracker& lk, const Image* img1, const Image& img2, std::vector<Point2f>& pts1,
                               std::vector<Point2f>& pts2) {
  std::vector<uint8_t> status;
  std::vector<float> err;
  // also with no points: the call uploads img2, so that the tracker's cached "previous frame" stays
  // in step with the caller's loop (img1 == nullptr on the next call means THIS img2)
  lk.calcOpticalFlowPyrLK(img1, img2, pts1, pts2, status, err, Size(21, 21), 3, TermCriteria(30, 0.01));
  if (pts1.empty()) return;
  std::vector<Point2f> v1, v2;
  for (size_t i = 0; i < status.size(); i++)
    if (status[i]) {
      v1.push_back(pts1[i]);
      v2.push_back(pts2[i]);
    }
  pts1 = v1;
  pts2 = v2;
}

// ---- relative pose (next row) -----------------------------------
// VisualOdom::get_pose (src/feature_matching.cpp:185-206, src/feature_tracking.cpp:222-242):
//   E = cv::findEssentialMat(pts1, pts2, K, cv::RANSAC, 0.999, 1.0, mask); cv::recoverPose(E, pts1, pts2, K, R, t, mask);
// K, R: row-major 3x3; t: unit translation with x2 = R x1 + t; mask: recoverPose's final mask.
inline void get_pose(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2, const double K[9],
                     double R[9], double t[3], std::vector<uint8_t>& mask, double prob = 0.999,
                     double threshold = 1.0, int max_iters = 1000, uint64_t seed = 0) {
  if (pts1.size() != pts2.size()) throw std::invalid_argument("get_pose: pts1 and pts2 differ in size");
  const int n = (int)pts1.size();
  std::vector<float> a((size_t)2 * n), b((size_t)2 * n);
  for (int i = 0; i < n; i++) {
    a[2 * i] = pts1[(size_t)i].x, a[2 * i + 1] = pts1[(size_t)i].y;
    b[2 * i] = pts2[(size_t)i].x, b[2 * i + 1] = pts2[(size_t)i].y;
  }
  mask.assign((size_t)n, 0);
  double E[9];
  int32_t inliers = 0, good = 0, iters = 0;
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c, orbx_estimate_pose(c, a.data(), b.data(), n, K, prob, threshold, max_iters, seed, E, R, t,
                              n > 0 ? mask.data() : nullptr, &inliers, &good, &iters),
        "orbx_estimate_pose");
}

// ---- triangulation, relative scale, pose chaining (next row) -------
struct Point3f {  // cv::Point3f
  float x = 0.f, y = 0.f, z = 0.f;
};

// The members of the reference's VisualOdom that the scale step carries from frame to frame
// (src/feature_matching.cpp:119-120): the previous pair's triangulated points and the camera pose.
// *_valid: one byte per point (cv::triangulatePoints leaves w = 0 as inf / NaN; here such a point is
// (0, 0, 0) with valid = 0 and enters no ratio).
struct VisualOdomState {
  std::vector<Point3f> prev_points_3d;
  std::vector<uint8_t> prev_valid, points_valid;  // points_valid: of the points_3d the last get_scale returned
  std::array<double, 16> cur_pose{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};  // row-major 4x4
  // prev_points_3d = points_3d (src/feature_matching.cpp:87), with the points' valid bytes
  void shift(const std::vector<Point3f>& points_3d) {
    prev_points_3d = points_3d;
    prev_valid = points_valid;
  }
};

// VisualOdom::get_scale (src/feature_matching.cpp:208-275, src/feature_tracking.cpp:244-310): triangulate the
// pair's correspondences under P1 = K [I|0], P2 = K [R|t], then the clamped median of the distance ratios between
// the previous pair's points (vo.prev_points_3d) and these, aligned by bare index as the C++ flavours do.  K, R:
// row-major 3x3.  A prev_valid whose size differs from prev_points_3d (the points were assigned directly) counts
// as all valid.
inline double get_scale(const double R[9], const double t[3], const std::vector<Point2f>& pts1,
                        const std::vector<Point2f>& pts2, const double K[9], std::vector<Point3f>& points_3d,
                        VisualOdomState& vo) {
  if (pts1.size() != pts2.size()) throw std::invalid_argument("get_scale: pts1 and pts2 differ in size");
  static_assert(sizeof(Point2f) == 2 * sizeof(float) && sizeof(Point3f) == 3 * sizeof(float), "point layouts");
  const int n = (int)pts1.size();
  points_3d.assign((size_t)n, Point3f());
  vo.points_valid.assign((size_t)n, 0);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_triangulate(c, reinterpret_cast<const float*>(pts1.data()),
                                 reinterpret_cast<const float*>(pts2.data()), n, K, R, t,
                                 reinterpret_cast<float*>(points_3d.data()), vo.points_valid.data()),
                "orbx_triangulate");
  double scale = 1.0;
  int32_t used = 0;
  const bool have_valid = vo.prev_valid.size() == vo.prev_points_3d.size();
  detail::check(c,
                orbx_estimate_scale(c, reinterpret_cast<const float*>(vo.prev_points_3d.data()),
                                    have_valid ? vo.prev_valid.data() : nullptr, (int)vo.prev_points_3d.size(),
                                    reinterpret_cast<const float*>(points_3d.data()), vo.points_valid.data(), n, &scale,
                                    &used),
                "orbx_estimate_scale");
  return scale;
}

// cur_pose = cur_pose * T.inv() with T = [R | scale * t] (src/feature_matching.cpp:77-82)
inline void chain_pose(std::array<double, 16>& cur_pose, const double R[9], const double t[3], double scale) {
  double poses[32];
  detail::check(nullptr, orbx_chain_trajectory(cur_pose.data(), R, t, &scale, 1, poses), "orbx_chain_trajectory");
  std::memcpy(cur_pose.data(), poses + 16, sizeof(double) * 16);
}

// ---- sliding-window bundle adjustment (next row) --------------------
// The host glue of src/with_bundle_adjustment.cpp around the solve (orbx_bundle_adjust).  Poses of a window are
// camera -> world, row-major 4x4, as the reference's pose_window.
struct Point2d {  // cv::Point2d
  double x = 0.0, y = 0.0;
};
struct Point3d {  // cv::Point3d
  double x = 0.0, y = 0.0, z = 0.0;
};
struct Landmark {  // src/with_bundle_adjustment.cpp:20-25
  int id = 0;
  Point3d pos;
  std::vector<std::pair<int, Point2d>> observations;  // (frame index in the window, pixel)
};
using Track = std::vector<std::pair<int, Point2f>>;
using Pose4x4 = std::array<double, 16>;

namespace detail {
// world -> camera [R | t] of a camera -> world pose (the reference's pose.inv(), in closed form)
inline void invert_rigid(const Pose4x4& T, double R[9], double t[3]) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = T[(size_t)(j * 4 + i)];
  for (int i = 0; i < 3; i++) t[i] = -(R[i * 3] * T[3] + R[i * 3 + 1] * T[7] + R[i * 3 + 2] * T[11]);
}
inline Pose4x4 compose_inverse(const double R[9], const double t[3]) {  // ([R | t])^-1 as a 4x4
  Pose4x4 T{{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[(size_t)(i * 4 + j)] = R[j * 3 + i];
    T[(size_t)(i * 4 + 3)] = -(R[0 * 3 + i] * t[0] + R[1 * 3 + i] * t[1] + R[2 * 3 + i] * t[2]);
  }
  return T;
}
// cv::Rodrigues, vector -> matrix
inline void rodrigues(const double w[3], double R[9]) {
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double k[3] = {w[0], w[1], w[2]}, s = 1.0, c1 = 0.5;  // th -> 0: R = I + [w]x + [w]x^2 / 2
  if (th > 1e-12) {
    for (double& v : k) v /= th;
    s = std::sin(th), c1 = 1.0 - std::cos(th);
  }
  const double K2[9] = {-(k[1] * k[1] + k[2] * k[2]), k[0] * k[1], k[0] * k[2], k[0] * k[1], -(k[0] * k[0] + k[2] * k[2]),
                        k[1] * k[2], k[0] * k[2], k[1] * k[2], -(k[0] * k[0] + k[1] * k[1])};
  const double K1[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
  for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + s * K1[i] + c1 * K2[i];
}
// cv::Rodrigues, matrix -> vector, angle in [0, pi] (through the unit quaternion: stable near pi)
inline void rodrigues_inv(const double R[9], double w[3]) {
  double q[4] = {1.0 + R[0] + R[4] + R[8], R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  if (q[0] < 1e-3) {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    q[1 + i] = 1.0 + R[i * 4] - R[j * 4] - R[k * 4];
    q[1 + j] = R[i * 3 + j] + R[j * 3 + i];
    q[1 + k] = R[i * 3 + k] + R[k * 3 + i];
    q[0] = R[k * 3 + j] - R[j * 3 + k];
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sg = q[0] < 0 ? -1.0 : 1.0;
  for (double& v : q) v = sg * v / n;
  const double s = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double f = s > 0 ? 2.0 * std::atan2(s, q[0]) / s : 0.0;
  for (int i = 0; i < 3; i++) w[i] = f * q[1 + i];
}
}  // namespace detail

// trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499): the points of frame 0 propagated frame by
// frame; a track ends with the first frame LK loses it in.  One LK call per consecutive image pair on all live
// points replaces the reference's one call per point and pair (LK treats every point on its own).
inline std::vector<Track> track_points_across_window(LKTracker& lk, const std::vector<Image>& imgs_window,
                                                     const std::vector<Point2f>& keypoints0) {
  std::vector<Track> tracks(keypoints0.size());
  std::vector<size_t> live(keypoints0.size());
  std::vector<Point2f> prev = keypoints0, next;
  for (size_t i = 0; i < keypoints0.size(); i++) {
    tracks[i].emplace_back(0, keypoints0[i]);
    live[i] = i;
  }
  std::vector<uint8_t> status;
  std::vector<float> err;
  for (size_t fi = 1; fi < imgs_window.size() && !live.empty(); fi++) {
    // after the first pair the tracker still holds the pyramid of imgs_window[fi - 1]
    lk.calcOpticalFlowPyrLK(fi == 1 ? &imgs_window[0] : nullptr, imgs_window[fi], prev, next, status, err, Size(21, 21),
                            3, TermCriteria(30, 0.01));
    std::vector<size_t> still;
    std::vector<Point2f> kept;
    for (size_t k = 0; k < live.size(); k++)
      if (status[k]) {
        tracks[live[k]].emplace_back((int)fi, next[k]);
        still.push_back(live[k]);
        kept.push_back(next[k]);
      }
    live.swap(still);
    prev.swap(kept);
  }
  return tracks;
}

// The same in one launch (LKTracker::trackWindow): no host compaction between the pairs, no round trip per pair.
// Returns exactly what track_points_across_window returns.
inline std::vector<Track> track_points_across_window_one_launch(LKTracker& lk, const std::vector<Image>& imgs_window,
                                                                const std::vector<Point2f>& keypoints0) {
  std::vector<Track> tracks(keypoints0.size());
  for (size_t i = 0; i < keypoints0.size(); i++) tracks[i].emplace_back(0, keypoints0[i]);
  if (imgs_window.size() < 2 || keypoints0.empty()) return tracks;
  std::vector<Point2f> xy;
  std::vector<int32_t> seen;
  std::vector<float> err;
  lk.trackWindow(imgs_window, keypoints0, xy, seen, err, Size(21, 21), 3, TermCriteria(30, 0.01));
  const size_t nf = imgs_window.size();
  for (size_t i = 0; i < keypoints0.size(); i++)
    for (int k = 1; k < seen[i]; k++) tracks[i].emplace_back(k, xy[i * nf + (size_t)k]);
  return tracks;
}

// trackPointsAcrossWindow with the forward-backward check every KLT front end puts behind calcOpticalFlowPyrLK
// (DESIGN.md §9 rank 13), pair by pair on the host: the live points tracked from frame fi - 1 into frame fi, the
// survivors tracked back, and a track kept iff both passes keep it and the return lies within thr of the start.  Two
// LK calls and two compactions per pair.  lost (optional): why each track ended, 0 for one alive through the window,
// 1 forward pass, 2 backward pass, 3 distance.
inline std::vector<Track> track_points_across_window_fb(LKTracker& lk, const std::vector<Image>& imgs_window,
                                                        const std::vector<Point2f>& keypoints0, float thr,
                                                        std::vector<int32_t>* lost = nullptr) {
  if (!(thr >= 0.f)) throw std::runtime_error("track_points_across_window_fb: the threshold is NaN or negative");
  std::vector<Track> tracks(keypoints0.size());
  std::vector<size_t> live(keypoints0.size());
  std::vector<Point2f> prev = keypoints0, next, back;
  for (size_t i = 0; i < keypoints0.size(); i++) {
    tracks[i].emplace_back(0, keypoints0[i]);
    live[i] = i;
  }
  if (lost) lost->assign(keypoints0.size(), 0);
  const double thr2 = (double)thr * (double)thr;
  std::vector<uint8_t> status;
  std::vector<float> err;
  for (size_t fi = 1; fi < imgs_window.size() && !live.empty(); fi++) {
    lk.calcOpticalFlowPyrLK(&imgs_window[fi - 1], imgs_window[fi], prev, next, status, err, Size(21, 21), 3,
                            TermCriteria(30, 0.01));
    std::vector<size_t> fwd;
    std::vector<Point2f> p, q;
    for (size_t k = 0; k < live.size(); k++)
      if (status[k]) {
        fwd.push_back(live[k]);
        p.push_back(prev[k]);
        q.push_back(next[k]);
      } else if (lost) {
        (*lost)[live[k]] = 1;
      }
    live.clear();
    prev.clear();
    if (fwd.empty()) break;
    // back from q: the tracker still holds the pyramid of imgs_window[fi]
    lk.calcOpticalFlowPyrLK(nullptr, imgs_window[fi - 1], q, back, status, err, Size(21, 21), 3,
                            TermCriteria(30, 0.01));
    for (size_t k = 0; k < fwd.size(); k++) {
      int why = 0;
      if (!status[k]) {
        why = 2;
      } else {
        const float dx = back[k].x - p[k].x, dy = back[k].y - p[k].y;
        const double d2 = (double)dx * (double)dx + (double)dy * (double)dy;  // exact products, one rounding
        if (!(d2 <= thr2)) why = 3;
      }
      if (why) {
        if (lost) (*lost)[fwd[k]] = why;
        continue;
      }
      tracks[fwd[k]].emplace_back((int)fi, q[k]);
      live.push_back(fwd[k]);
      prev.push_back(q[k]);
    }
  }
  return tracks;
}

// The same in one launch (LKTracker::trackWindow with fbThreshold).  Returns exactly what
// track_points_across_window_fb returns.
inline std::vector<Track> track_points_across_window_fb_one_launch(LKTracker& lk,
                                                                   const std::vector<Image>& imgs_window,
                                                                   const std::vector<Point2f>& keypoints0, float thr,
                                                                   std::vector<int32_t>* lost = nullptr) {
  if (!(thr >= 0.f)) throw std::runtime_error("track_points_across_window_fb: the threshold is NaN or negative");
  std::vector<Track> tracks(keypoints0.size());
  for (size_t i = 0; i < keypoints0.size(); i++) tracks[i].emplace_back(0, keypoints0[i]);
  if (lost) lost->assign(keypoints0.size(), 0);
  if (imgs_window.size() < 2 || keypoints0.empty()) return tracks;
  std::vector<Point2f> xy;
  std::vector<int32_t> seen, why;
  std::vector<float> err, d2;
  lk.trackWindow(imgs_window, keypoints0, thr, xy, seen, err, d2, why, Size(21, 21), 3, TermCriteria(30, 0.01));
  const size_t nf = imgs_window.size();
  for (size_t i = 0; i < keypoints0.size(); i++)
    for (int k = 1; k < seen[i]; k++) tracks[i].emplace_back(k, xy[i * nf + (size_t)k]);
  if (lost) *lost = why;
  return tracks;
}

// The motion of every consecutive frame pair of one tracked window: what the reference's
// tracking loop computes per frame with track_optical_flow's surviving lists, get_pose and get_scale
// (src/feature_tracking.cpp:66-93, src/with_bundle_adjustment.cpp:180-203), for the window's pairs in one call.
// tracks / seen: what LKTracker::trackWindow returns (n x n_frames points, n counts).  Pair k is frames k, k + 1: its
// list is the slots with seen >= k + 2 in ascending slot order.  The scale of pair k >= 1 joins its points with
// pair k - 1's ON THE SLOT (the reference aligns them by list position, which misaligns after a lost track); pair
// 0 has scale 1.
struct PairMotion {
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  double scale = 1.0;
  std::vector<int32_t> slots;  // the surviving slots: the pair's correspondence list
};
inline std::vector<PairMotion> get_pose_and_scale_on_tracks(const std::vector<Point2f>& tracks,
                                                            const std::vector<int32_t>& seen, int n_frames,
                                                            const double K[9], double prob = 0.999,
                                                            double threshold = 1.0, int max_iters = 1000,
                                                            uint64_t seed = 0) {
  if (n_frames < 2) throw std::invalid_argument("get_pose_and_scale_on_tracks: a window has at least two frames");
  if (tracks.size() != seen.size() * (size_t)n_frames)
    throw std::invalid_argument("get_pose_and_scale_on_tracks: tracks and seen differ in size");
  static_assert(sizeof(Point2f) == 2 * sizeof(float), "point layout");
  const int n = (int)seen.size(), pairs = n_frames - 1;
  std::vector<PairMotion> out((size_t)pairs);
  if (n == 0) return out;
  std::vector<double> R((size_t)9 * pairs), t((size_t)3 * pairs), scale((size_t)pairs);
  std::vector<int32_t> counts((size_t)pairs);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_tracks_pose(c, K, reinterpret_cast<const float*>(tracks.data()), seen.data(), n, n_frames, prob,
                                 threshold, max_iters, seed, nullptr, R.data(), t.data(), nullptr, nullptr, nullptr,
                                 counts.data(), scale.data(), nullptr, nullptr),
                "orbx_tracks_pose");
  for (int p = 0; p < pairs; p++) {
    PairMotion& m = out[(size_t)p];
    std::memcpy(m.R, R.data() + 9 * p, sizeof m.R);
    std::memcpy(m.t, t.data() + 3 * p, sizeof m.t);
    m.scale = scale[(size_t)p];
    m.slots.assign((size_t)counts[(size_t)p], 0);
    int count = 0;
    detail::check(c,
                  orbx_tracks_pose_pair_fetch(c, p, m.slots.data(), nullptr, nullptr, nullptr, counts[(size_t)p], &count),
                  "orbx_tracks_pose_pair_fetch");
  }
  return out;
}

// buildLandmarksFromFirstTwoFramesAndTracks (src/with_bundle_adjustment.cpp:502-575): the baseline gate
// 0.1 .. 100 on |t0 - t1| of the world -> camera translations, triangulation of every track seen in frame 1 from
// frames 0 / 1, the reference's depth check `X.z > 0` (on the world-frame point, as there), the track's
// observations attached.  The triangulation runs in camera 0's frame (orbx_triangulate with the relative pose)
// and the point is then moved to the world frame; the reference solves the DLT in world coordinates.  The two
// agree up to rounding and the conditioning of the 4x4 system; parity is unpinned either way.
inline bool build_landmarks(const std::vector<Pose4x4>& pose_window, const double K[9], const std::vector<Track>& tracks,
                            std::vector<Landmark>& landmarks) {
  if (pose_window.size() < 2) return false;
  double R0[9], t0[3], R1[9], t1[3];
  detail::invert_rigid(pose_window[0], R0, t0);
  detail::invert_rigid(pose_window[1], R1, t1);
  const double baseline = std::sqrt((t0[0] - t1[0]) * (t0[0] - t1[0]) + (t0[1] - t1[1]) * (t0[1] - t1[1]) +
                                    (t0[2] - t1[2]) * (t0[2] - t1[2]));
  if (baseline < 0.1 || baseline > 100) return false;
  double Rr[9], tr[3];  // camera 0 -> camera 1
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rr[i * 3 + j] = R1[i * 3] * R0[j * 3] + R1[i * 3 + 1] * R0[j * 3 + 1] + R1[i * 3 + 2] * R0[j * 3 + 2];
  for (int i = 0; i < 3; i++) tr[i] = t1[i] - (Rr[i * 3] * t0[0] + Rr[i * 3 + 1] * t0[1] + Rr[i * 3 + 2] * t0[2]);
  std::vector<float> p0, p1;
  std::vector<size_t> original;
  for (size_t i = 0; i < tracks.size(); i++)
    for (const auto& obs : tracks[i])
      if (obs.first == 1 && !tracks[i].empty()) {
        p0.push_back(tracks[i][0].second.x), p0.push_back(tracks[i][0].second.y);
        p1.push_back(obs.second.x), p1.push_back(obs.second.y);
        original.push_back(i);
        break;
      }
  const int n = (int)original.size();
  std::vector<float> xyz((size_t)3 * n);
  std::vector<uint8_t> valid((size_t)n);
  if (n > 0) {
    orbx_ctx* c = detail::stage_ctx()->get(8, 8);
    detail::check(c, orbx_triangulate(c, p0.data(), p1.data(), n, K, Rr, tr, xyz.data(), valid.data()), "orbx_triangulate");
  }
  landmarks.reserve(landmarks.size() + (size_t)n);
  for (int j = 0; j < n; j++) {
    if (!valid[(size_t)j]) continue;
    const double d[3] = {xyz[3 * (size_t)j] - t0[0], xyz[3 * (size_t)j + 1] - t0[1], xyz[3 * (size_t)j + 2] - t0[2]};
    Landmark lm;
    lm.pos.x = R0[0] * d[0] + R0[3] * d[1] + R0[6] * d[2];  // X = R0^T (x - t0)
    lm.pos.y = R0[1] * d[0] + R0[4] * d[1] + R0[7] * d[2];
    lm.pos.z = R0[2] * d[0] + R0[5] * d[1] + R0[8] * d[2];
    if (lm.pos.z <= 0) continue;  // "Simple depth check", :559
    lm.id = j;
    for (const auto& obs : tracks[original[(size_t)j]])
      lm.observations.emplace_back(obs.first, Point2d{(double)obs.second.x, (double)obs.second.y});
    landmarks.push_back(std::move(lm));
  }
  return true;
}

namespace detail {
// The write-back gate of run_bundle_adjustment (src/with_bundle_adjustment.cpp:683-718) after a converged solve:
// pose i (world -> camera block `poses`, before the solve `old`) is written back as a camera -> world 4x4 iff it
// moved by less than 0.5 rad and 50 units.
inline void ba_write_back(std::vector<Pose4x4>& pose_window, const std::vector<double>& poses,
                          const std::vector<double>& old, std::vector<uint8_t>* updated) {
  const int W = (int)pose_window.size();
  for (int i = 0; i < W; i++) {
    double R[9], Ro[9], Rd[9], wd[3];
    rodrigues(&poses[(size_t)6 * i], R);
    rodrigues(&old[(size_t)6 * i], Ro);
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) Rd[a * 3 + b] = R[a * 3] * Ro[b * 3] + R[a * 3 + 1] * Ro[b * 3 + 1] + R[a * 3 + 2] * Ro[b * 3 + 2];
    rodrigues_inv(Rd, wd);
    const double angle = std::sqrt(wd[0] * wd[0] + wd[1] * wd[1] + wd[2] * wd[2]);
    double tn = 0.0;
    for (int k = 0; k < 3; k++) tn += (poses[(size_t)6 * i + 3 + k] - old[(size_t)6 * i + 3 + k]) * (poses[(size_t)6 * i + 3 + k] - old[(size_t)6 * i + 3 + k]);
    if (angle < 0.5 && std::sqrt(tn) < 50.0) {  // MAX_ROT_DIFF, MAX_TRANS_DIFF
      pose_window[(size_t)i] = compose_inverse(R, &poses[(size_t)6 * i + 3]);
      if (updated) (*updated)[(size_t)i] = 1;
    }
  }
}
}  // namespace detail

// The solve and write-back of run_bundle_adjustment (src/with_bundle_adjustment.cpp:612-720): world -> camera
// angle-axis blocks from the camera -> world poses, orbx_bundle_adjust (HuberLoss(1.0), 200 iterations, pose 0
// constant), and -- only on convergence -- each pose written back iff it moved by less than 0.5 rad and 50 units
// (:708-718).  updated[i]: pose i was written back.  Returns false when there is nothing to solve.
inline bool run_bundle_adjustment(std::vector<Pose4x4>& pose_window, const double K[9],
                                  const std::vector<Landmark>& landmarks, orbx_ba_summary* summary = nullptr,
                                  std::vector<uint8_t>* updated = nullptr, double huber_delta = 1.0,
                                  int max_iters = 200) {
  const int W = (int)pose_window.size();
  if (updated) updated->assign((size_t)W, 0);
  if (landmarks.empty() || W < 2) return false;
  std::vector<double> poses((size_t)6 * W), points, xy;
  std::vector<int32_t> op, oq;
  for (int i = 0; i < W; i++) {
    double R[9], t[3];
    detail::invert_rigid(pose_window[(size_t)i], R, t);
    detail::rodrigues_inv(R, &poses[(size_t)6 * i]);
    for (int k = 0; k < 3; k++) poses[(size_t)6 * i + 3 + k] = t[k];
  }
  for (const Landmark& lm : landmarks) {
    int used = 0;
    for (const auto& obs : lm.observations) {
      if (obs.first < 0 || obs.first >= W) continue;  // :655
      op.push_back((int32_t)(points.size() / 3)), oq.push_back(obs.first);
      xy.push_back(obs.second.x), xy.push_back(obs.second.y);
      used++;
    }
    if (used) points.push_back(lm.pos.x), points.push_back(lm.pos.y), points.push_back(lm.pos.z);
  }
  if (points.empty()) return false;
  const std::vector<double> old = poses;
  orbx_ba_summary s{};
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c, orbx_bundle_adjust(c, K, W, poses.data(), (int)(points.size() / 3), points.data(), (int)op.size(),
                                      op.data(), oq.data(), xy.data(), huber_delta, max_iters, &s),
                "orbx_bundle_adjust");
  if (summary) *summary = s;
  if (s.termination != ORBX_BA_CONVERGENCE) return true;  // :683
  detail::ba_write_back(pose_window, poses, old, updated);
  return true;
}

// LandmarkOptions (include/orbx_lm.h): the views a track's point is triangulated from and the
// largest reprojection error in pixels a landmark may have (0: no gate).  The overload taking them builds the
// landmarks through orbx_bundle_adjust_tracks_views; the defaults are the reference's own build.
struct LandmarkOptions {
  int tri_mode = ORBX_LM_TRI_FIRST_TWO;
  double max_reproj_px = 0.0;
};
namespace detail {
// behind both overloads of run_bundle_adjustment_on_tracks; options: NULL for the reference's own build
inline bool ba_on_tracks(std::vector<Pose4x4>& pose_window, const double K[9], const std::vector<Point2f>& xy,
                         const std::vector<int32_t>& seen, const LandmarkOptions* options, orbx_ba_summary* summary,
                         std::vector<uint8_t>* updated, int32_t* lm_status, std::vector<Point3d>* points,
                         std::vector<int32_t>* slot_of_point, double huber_delta, int max_iters) {
  static_assert(sizeof(Point2f) == 2 * sizeof(float), "point layout");
  const int W = (int)pose_window.size();
  const size_t n = seen.size();
  if (updated) updated->assign((size_t)W, 0);
  if (points) points->clear();
  if (slot_of_point) slot_of_point->clear();
  if (W < 2 || n == 0) return false;
  if (xy.size() != n * (size_t)W) throw std::runtime_error("run_bundle_adjustment_on_tracks: xy is not n x window");
  std::vector<double> poses((size_t)6 * W);
  for (int i = 0; i < W; i++) {
    double R[9], t[3];
    detail::invert_rigid(pose_window[(size_t)i], R, t);
    detail::rodrigues_inv(R, &poses[(size_t)6 * i]);
    for (int k = 0; k < 3; k++) poses[(size_t)6 * i + 3 + k] = t[k];
  }
  const std::vector<double> old = poses;
  orbx_ba_summary s{};
  int32_t st = ORBX_LM_OK;
  int count = 0;
  std::vector<double> p3(3 * n);
  std::vector<int32_t> slots(n);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  if (options)
    detail::check(c, orbx_bundle_adjust_tracks_views(c, K, reinterpret_cast<const float*>(xy.data()), seen.data(), (int)n,
                                                     W, poses.data(), huber_delta, max_iters, &st, &s, p3.data(),
                                                     slots.data(), (int)n, &count, options->tri_mode,
                                                     options->max_reproj_px),
                  "orbx_bundle_adjust_tracks_views");
  else
    detail::check(c, orbx_bundle_adjust_tracks(c, K, reinterpret_cast<const float*>(xy.data()), seen.data(), (int)n, W,
                                               poses.data(), huber_delta, max_iters, &st, &s, p3.data(), slots.data(),
                                               (int)n, &count),
                  "orbx_bundle_adjust_tracks");
  if (summary) *summary = s;
  if (lm_status) *lm_status = st;
  if (st != ORBX_LM_OK) return false;
  for (int j = 0; j < count; j++) {
    if (points) points->push_back(Point3d{p3[3 * (size_t)j], p3[3 * (size_t)j + 1], p3[3 * (size_t)j + 2]});
    if (slot_of_point) slot_of_point->push_back(slots[(size_t)j]);
  }
  if (s.termination != ORBX_BA_CONVERGENCE) return true;  // :683
  detail::ba_write_back(pose_window, poses, old, updated);
  return true;
}
}  // namespace detail

// The whole window from what LKTracker::trackWindow returns: landmarks built on the device
// from the tracks (buildLandmarksFromFirstTwoFramesAndTracks, src/with_bundle_adjustment.cpp:502-575; the DLT in
// WORLD coordinates, the point kept in binary64) and solved there (src/with_bundle_adjustment.cpp:612-720) through
// orbx_bundle_adjust_tracks, then the same write-back gate as run_bundle_adjustment.  xy: n x pose_window.size()
// points, seen: n.  build_landmarks + run_bundle_adjustment triangulate in camera 0's frame through float instead:
// the two routes differ by that, and both are unpinned against OpenCV / Ceres.  lm_status: the orbx_lm_status of
// the window; points / slot_of_point: the refined landmarks and the track each came from.  Returns false when
// there is nothing to solve.
inline bool run_bundle_adjustment_on_tracks(std::vector<Pose4x4>& pose_window, const double K[9],
                                            const std::vector<Point2f>& xy, const std::vector<int32_t>& seen,
                                            orbx_ba_summary* summary = nullptr, std::vector<uint8_t>* updated = nullptr,
                                            int32_t* lm_status = nullptr, std::vector<Point3d>* points = nullptr,
                                            std::vector<int32_t>* slot_of_point = nullptr, double huber_delta = 1.0,
                                            int max_iters = 200) {
  return detail::ba_on_tracks(pose_window, K, xy, seen, nullptr, summary, updated, lm_status, points, slot_of_point,
                              huber_delta, max_iters);
}
// the same window with the landmarks built by `options` (orbx_bundle_adjust_tracks_views)
inline bool run_bundle_adjustment_on_tracks(std::vector<Pose4x4>& pose_window, const double K[9],
                                            const std::vector<Point2f>& xy, const std::vector<int32_t>& seen,
                                            const LandmarkOptions& options, orbx_ba_summary* summary = nullptr,
                                            std::vector<uint8_t>* updated = nullptr, int32_t* lm_status = nullptr,
                                            std::vector<Point3d>* points = nullptr,
                                            std::vector<int32_t>* slot_of_point = nullptr, double huber_delta = 1.0,
                                            int max_iters = 200) {
  return detail::ba_on_tracks(pose_window, K, xy, seen, &options, summary, updated, lm_status, points, slot_of_point,
                              huber_delta, max_iters);
}

// ---- window poses and the gated window ------------------------------
// The poses of one window from its pair motions (src/with_bundle_adjustment.cpp:196-208): pose_window[0] = pose0,
// pose_window[k + 1] = pose_window[k] * [R_k | s_k t_k]^-1 with s_0 = scale0 and the motions' own scale after; blocks
// receives the world -> camera 6-double block of every pose (:615-628).  orbx_chain_window_poses: the arithmetic the
// device chain runs, from the same source.
inline std::vector<Pose4x4> chain_window_poses(const Pose4x4& pose0, const std::vector<PairMotion>& motions,
                                               double scale0 = 1.0,
                                               std::vector<std::array<double, 6>>* blocks = nullptr) {
  const size_t n = motions.size();
  std::vector<double> R(9 * n), t(3 * n), s(n);
  for (size_t k = 0; k < n; k++) {
    std::memcpy(&R[9 * k], motions[k].R, sizeof motions[k].R);
    std::memcpy(&t[3 * k], motions[k].t, sizeof motions[k].t);
    s[k] = k == 0 ? scale0 : motions[k].scale;
  }
  std::vector<Pose4x4> poses(n + 1);
  std::vector<std::array<double, 6>> b6(n + 1);
  static_assert(sizeof(Pose4x4) == 16 * sizeof(double) && sizeof(std::array<double, 6>) == 6 * sizeof(double), "layout");
  detail::check(nullptr,
                orbx_chain_window_poses(pose0.data(), R.data(), t.data(), s.data(), (int)n, poses[0].data(), b6[0].data()),
                "orbx_chain_window_poses");
  if (blocks) *blocks = std::move(b6);
  return poses;
}

struct WindowOdometry {
  std::vector<Pose4x4> pose_window;  // camera -> world, after the write-back gate
  std::vector<uint8_t> updated;      // pose i was written back
  int32_t wp_status = ORBX_WP_OK, lm_status = ORBX_LM_OK;
  orbx_ba_summary summary{};
};
// One window from what LKTracker::trackWindow returns to the gated pose_window, everything between on the device
// (src/with_bundle_adjustment.cpp:180-208, :502-575, :612-720): pose and scale of every pair, the chain from pose0,
// landmarks, the solve and the write-back gate, through orbx_window_odometry_tracks.  xy: n x n_frames points,
// seen: n.  run_bundle_adjustment_on_tracks is the same window with the poses given.
inline WindowOdometry run_window_odometry_on_tracks(const Pose4x4& pose0, const double K[9],
                                                    const std::vector<Point2f>& xy, const std::vector<int32_t>& seen,
                                                    int n_frames, double scale0 = 1.0, double prob = 0.999,
                                                    double threshold = 1.0, int pose_max_iters = 1000,
                                                    uint64_t seed = 0, double huber_delta = 1.0, int ba_max_iters = 200,
                                                    double max_rot = 0.5, double max_trans = 50.0) {
  static_assert(sizeof(Point2f) == 2 * sizeof(float), "point layout");
  if (n_frames < 2) throw std::invalid_argument("run_window_odometry_on_tracks: a window has at least two frames");
  if (seen.empty() || xy.size() != seen.size() * (size_t)n_frames)
    throw std::invalid_argument("run_window_odometry_on_tracks: xy is not n x n_frames");
  WindowOdometry out;
  out.pose_window.resize((size_t)n_frames);
  out.updated.assign((size_t)n_frames, 0);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_window_odometry_tracks(c, K, reinterpret_cast<const float*>(xy.data()), seen.data(),
                                            (int)seen.size(), n_frames, pose0.data(), scale0, prob, threshold,
                                            pose_max_iters, seed, huber_delta, ba_max_iters, max_rot, max_trans,
                                            out.pose_window[0].data(), out.updated.data(), &out.wp_status,
                                            &out.lm_status, &out.summary),
                "orbx_window_odometry_tracks");
  return out;
}

// ---- a stream of overlapping windows joined into one trajectory ------------------------
// What the reference does across solves, cur_pose = prev_pose * T.inv() and cur_pose = pose_window.back()
// (src/with_bundle_adjustment.cpp:203, :234-249), for windows that each live in a frame of their own: window w of
// window_len poses starts at stream frame w * stride.  orbx_stitch_windows: the arithmetic the device stitch runs, from
// the same source; needs no GPU.
struct StitchedStream {
  std::vector<Pose4x4> trajectory;  // camera -> world, one per stream frame; [0] = pose0
  std::vector<int32_t> owner;       // the window a frame's pose was taken from
  std::vector<Pose4x4> anchors;     // the stream pose of every window's first frame
  std::vector<double> lambda;       // the scale every window's translations were multiplied by
  std::vector<int32_t> status;      // bits of orbx_st_status per window
};
inline StitchedStream stitch_windows(const std::vector<Pose4x4>& window_poses, int n_windows, int window_len, int stride,
                                     const Pose4x4& pose0, bool align_scale = false) {
  static_assert(sizeof(Pose4x4) == 16 * sizeof(double), "layout");
  if (n_windows < 1 || window_len < 2 || window_poses.size() != (size_t)n_windows * (size_t)window_len)
    throw std::invalid_argument("stitch_windows: window_poses is not n_windows x window_len");
  if (stride < 1 || stride > window_len - 1) throw std::invalid_argument("stitch_windows: stride outside [1, window_len - 1]");
  const size_t F = (size_t)(n_windows - 1) * stride + window_len, W = (size_t)n_windows;
  StitchedStream out;
  out.trajectory.resize(F);
  out.owner.resize(F);
  out.anchors.resize(W);
  out.lambda.resize(W);
  out.status.resize(W);
  detail::check(nullptr,
                orbx_stitch_windows(window_poses[0].data(), n_windows, window_len, stride, pose0.data(), align_scale,
                                    out.trajectory[0].data(), out.owner.data(), out.anchors[0].data(),
                                    out.lambda.data(), out.status.data()),
                "orbx_stitch_windows");
  return out;
}

struct StreamOdometry {
  std::vector<Pose4x4> trajectory;           // camera -> world, one per stream frame
  std::vector<int32_t> st_status, wp_status, lm_status;  // per window
  std::vector<orbx_ba_summary> summaries;    // per window
};
// A stream of n_windows overlapping windows from what LKTracker::trackWindow returns for each to one trajectory,
// everything between on the device (src/with_bundle_adjustment.cpp:180-208, :234-249, :502-575, :612-720), through
// orbx_stream_odometry_tracks.  xy: n_windows x n x n_frames points, seen: n_windows x n.  run_window_odometry_on_tracks
// is one window of it, with the pose of its first frame and the scale of its first pair handed in.
inline StreamOdometry run_stream_odometry_on_tracks(const Pose4x4& pose0, const double K[9],
                                                    const std::vector<Point2f>& xy, const std::vector<int32_t>& seen,
                                                    int n_windows, int n_frames, int stride, double scale0 = 1.0,
                                                    const LandmarkOptions& options = LandmarkOptions(),
                                                    bool align_scale = false, double prob = 0.999,
                                                    double threshold = 1.0, int pose_max_iters = 1000, uint64_t seed = 0,
                                                    double huber_delta = 1.0, int ba_max_iters = 200,
                                                    double max_rot = 0.5, double max_trans = 50.0) {
  static_assert(sizeof(Point2f) == 2 * sizeof(float), "point layout");
  if (n_windows < 1 || n_frames < 2 || stride < 1 || stride > n_frames - 1)
    throw std::invalid_argument("run_stream_odometry_on_tracks: no stream of n_windows windows of n_frames at this stride");
  if (seen.empty() || seen.size() % (size_t)n_windows || xy.size() != seen.size() * (size_t)n_frames)
    throw std::invalid_argument("run_stream_odometry_on_tracks: xy is not n_windows x n x n_frames");
  const size_t W = (size_t)n_windows;
  StreamOdometry out;
  out.trajectory.resize((W - 1) * (size_t)stride + (size_t)n_frames);
  out.st_status.resize(W);
  out.wp_status.resize(W);
  out.lm_status.resize(W);
  out.summaries.resize(W);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_stream_odometry_tracks(c, K, reinterpret_cast<const float*>(xy.data()), seen.data(), n_windows,
                                            (int)(seen.size() / W), n_frames, stride, pose0.data(), scale0, prob,
                                            threshold, pose_max_iters, seed, options.tri_mode, options.max_reproj_px,
                                            huber_delta, ba_max_iters, max_rot, max_trans, align_scale,
                                            out.trajectory[0].data(), out.st_status.data(), out.wp_status.data(),
                                            out.lm_status.data(), out.summaries.data()),
                "orbx_stream_odometry_tracks");
  return out;
}

// ---- perspective-n-point with RANSAC ----------------------------------------------------
// cv::solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, rvec, tvec, useExtrinsicGuess,
//                    iterationsCount, reprojectionError, confidence, inliers)
// in the call shape OpenCV gives it; the reference calls none -- its window poses come from the chain of
// src/with_bundle_adjustment.cpp:196-208 alone.  No distortion coefficients and no extrinsic guess.  K: row-major 3x3.
// rvec (angle-axis) and tvec are world -> camera and are ASSIGNED only when a pose was found (the return value);
// inliers receives the indices of the inliers as OpenCV's does.  P3P samples, at most refine_iters Levenberg-Marquardt
// steps on the inliers of the best model; a model needs min_inliers inliers.  The samples depend on (seed, iteration).
struct PnPInfo {
  int32_t status = 0;  // an orbx_pnp_status
  int32_t inliers = 0, iters = 0;
  double rms_px = 0.0;
};
inline bool solvePnPRansac(const std::vector<Point3d>& objectPoints, const std::vector<Point2d>& imagePoints,
                           const double K[9], double rvec[3], double tvec[3], int iterationsCount = 100,
                           double reprojectionError = 8.0, double confidence = 0.99,
                           std::vector<int>* inliers = nullptr, uint64_t seed = 0, int refine_iters = 10,
                           int min_inliers = 4, PnPInfo* info = nullptr) {
  static_assert(sizeof(Point3d) == 3 * sizeof(double) && sizeof(Point2d) == 2 * sizeof(double), "point layouts");
  if (objectPoints.size() != imagePoints.size())
    throw std::invalid_argument("solvePnPRansac: objectPoints and imagePoints differ in size");
  const int n = (int)objectPoints.size();
  std::vector<uint8_t> mask((size_t)n, 0);
  double pose6[6];
  PnPInfo r;
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_pnp_ransac(c, n > 0 ? &objectPoints[0].x : nullptr, n > 0 ? &imagePoints[0].x : nullptr, n, K,
                                confidence, reprojectionError, iterationsCount, seed, refine_iters, min_inliers, pose6,
                                n > 0 ? mask.data() : nullptr, &r.inliers, &r.iters, &r.rms_px, &r.status),
                "orbx_pnp_ransac");
  if (info) *info = r;
  if (inliers) {
    inliers->clear();
    for (int i = 0; i < n; i++)
      if (mask[(size_t)i]) inliers->push_back(i);
  }
  if (r.status != ORBX_PNP_OK) return false;
  for (int i = 0; i < 3; i++) rvec[i] = pose6[i], tvec[i] = pose6[3 + i];
  return true;
}

// ---- landmarks carried into the next window and the window localised against them -------
// The map-tracking step of a KLT front-end, where the reference re-detects at every solve
// (src/with_bundle_adjustment.cpp:586-593) and chains cur_pose = prev_pose * T.inv()
// (src/with_bundle_adjustment.cpp:196-208): the new window's slot s continues the old window's slot origin[s] (-1: a
// fresh point), the old window's landmarks are old_points with old_slot_of_point (ascending), and EVERY frame of the
// new window -- tracks (slots x n_frames) and seen, the layout of track_points_across_window's one-launch forms -- is
// localised against the carried landmarks by solvePnPRansac's rules, in the old window's own metric frame.
struct CarriedWindow {
  std::vector<orbx_pnp_record> records;  // one per frame
  std::vector<double> poses6;            // n_frames x 6: angle-axis and translation, world -> camera
  int32_t status = ORBX_CARRY_LOST;      // an orbx_carry_status
  std::vector<int32_t> carried_point;    // per slot: the landmark's index in old_points, or -1
  bool ok() const { return status == ORBX_CARRY_OK; }
};
inline CarriedWindow localise_carried_window(const std::vector<Point3d>& old_points,
                                             const std::vector<int32_t>& old_slot_of_point,
                                             const std::vector<int32_t>& origin, const std::vector<Point2f>& tracks,
                                             const std::vector<int32_t>& seen, int n_frames, const double K[9],
                                             int iterationsCount = 100, double reprojectionError = 8.0,
                                             double confidence = 0.99, uint64_t seed = 0, int refine_iters = 10,
                                             int min_inliers = 4) {
  static_assert(sizeof(Point3d) == 3 * sizeof(double) && sizeof(Point2f) == 2 * sizeof(float), "point layouts");
  if (old_points.size() != old_slot_of_point.size())
    throw std::invalid_argument("localise_carried_window: old_points and old_slot_of_point differ in size");
  if (n_frames < 2) throw std::invalid_argument("localise_carried_window: a window has at least two frames");
  if (origin.size() != seen.size() || tracks.size() != seen.size() * (size_t)n_frames)
    throw std::invalid_argument("localise_carried_window: origin, tracks and seen differ in size");
  const int n_old = (int)old_points.size(), n = (int)seen.size();
  CarriedWindow out;
  out.records.resize((size_t)n_frames);
  out.poses6.assign((size_t)6 * n_frames, 0.0);
  out.carried_point.assign((size_t)n, -1);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_localise_carried_window(c, n_old > 0 ? &old_points[0].x : nullptr,
                                             n_old > 0 ? old_slot_of_point.data() : nullptr, n_old, origin.data(),
                                             reinterpret_cast<const float*>(tracks.data()), seen.data(), n, n_frames, K,
                                             confidence, reprojectionError, iterationsCount, seed, refine_iters,
                                             min_inliers, out.records.data(), out.poses6.data(), &out.status,
                                             out.carried_point.data()),
                "orbx_localise_carried_window");
  return out;
}

// ---- landmark priors in the window solve --------------------------------------------------
// The reference's Ceres problem of one window (src/with_bundle_adjustment.cpp:612-679: reprojection residuals,
// HuberLoss, pose 0 constant) with one more residual block sqrt(weight) (X - anchor) per anchored landmark, which ties
// the window to the map the anchors come from and fixes the scale the reference leaves free.  poses6 (6 per pose:
// angle-axis and translation, world -> camera) and points are the start and, on ORBX_BA_CONVERGENCE only, the result.
// anchors and weights are one per point, or both empty: no priors.  start: an orbx_prior_start.
struct PriorSolve {
  std::vector<double> poses6;
  std::vector<Point3d> points;
  orbx_ba_summary summary{};
  bool converged() const { return summary.termination == ORBX_BA_CONVERGENCE; }
};
inline PriorSolve bundle_adjust_with_priors(const double K[9], const std::vector<double>& poses6,
                                            const std::vector<Point3d>& points, const std::vector<int32_t>& obs_point,
                                            const std::vector<int32_t>& obs_pose, const std::vector<Point2d>& obs_xy,
                                            const std::vector<Point3d>& anchors, const std::vector<double>& weights,
                                            int start = ORBX_PRIOR_START_GIVEN, double huber_delta = 1.0,
                                            int max_iters = 200) {
  static_assert(sizeof(Point3d) == 3 * sizeof(double) && sizeof(Point2d) == 2 * sizeof(double), "point layouts");
  if (poses6.size() % 6 != 0) throw std::invalid_argument("bundle_adjust_with_priors: poses6 holds 6 doubles per pose");
  if (obs_point.size() != obs_pose.size() || obs_point.size() != obs_xy.size())
    throw std::invalid_argument("bundle_adjust_with_priors: obs_point, obs_pose and obs_xy differ in size");
  if (anchors.size() != weights.size() || (!anchors.empty() && anchors.size() != points.size()))
    throw std::invalid_argument("bundle_adjust_with_priors: anchors and weights are one per point, or both empty");
  PriorSolve out;
  out.poses6 = poses6;
  out.points = points;
  const int n = (int)points.size(), m = (int)obs_point.size();
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_bundle_adjust_prior(c, K, (int)(poses6.size() / 6), out.poses6.data(), n,
                                         n > 0 ? &out.points[0].x : nullptr, m, obs_point.data(), obs_pose.data(),
                                         m > 0 ? &obs_xy[0].x : nullptr, anchors.empty() ? nullptr : &anchors[0].x,
                                         anchors.empty() ? nullptr : weights.data(), start, huber_delta, max_iters,
                                         &out.summary),
                "orbx_bundle_adjust_prior");
  return out;
}

// ---- the search by projection ------------------------------------------------------------
// ORB-SLAM's SearchByProjection, where the reference keeps no point across a solve
// (src/with_bundle_adjustment.cpp:586-593) and its only matcher is the global ratio test
// (src/feature_tracking.cpp:203-219).  project_landmarks: the old window's landmarks -- old_points with the ascending
// old_slot_of_point, as localise_carried_window takes them -- under a predicted pose6 (angle-axis and translation,
// world -> camera), per OLD SLOT.  reassociate_gated: the matcher of two described sets whose candidates lie within
// radius_px of the predictions; its origin is what localise_carried_window takes.
struct ProjectedLandmarks {
  std::vector<Point2d> xy;     // per old slot: the predicted pixel, zeros unless the state is ORBX_PROJ_OK
  std::vector<double> depth;   // per old slot
  std::vector<int32_t> state;  // per old slot: an orbx_proj_state
  int32_t count = 0;           // the ORBX_PROJ_OK slots
};
inline ProjectedLandmarks project_landmarks(const std::vector<Point3d>& old_points,
                                            const std::vector<int32_t>& old_slot_of_point, int slot_capacity,
                                            const double K[9], const double pose6[6], int width, int height,
                                            double margin_px = 0.0) {
  static_assert(sizeof(Point3d) == 3 * sizeof(double) && sizeof(Point2d) == 2 * sizeof(double), "point layouts");
  if (old_points.size() != old_slot_of_point.size())
    throw std::invalid_argument("project_landmarks: old_points and old_slot_of_point differ in size");
  if (slot_capacity < 1) throw std::invalid_argument("project_landmarks: slot_capacity < 1");
  const int n_old = (int)old_points.size();
  ProjectedLandmarks out;
  out.xy.assign((size_t)slot_capacity, Point2d{0.0, 0.0});
  out.depth.assign((size_t)slot_capacity, 0.0);
  out.state.assign((size_t)slot_capacity, ORBX_PROJ_NONE);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_project_landmarks(c, n_old > 0 ? &old_points[0].x : nullptr,
                                       n_old > 0 ? old_slot_of_point.data() : nullptr, n_old, slot_capacity, K, pose6,
                                       width, height, margin_px, &out.xy[0].x, out.depth.data(), out.state.data(),
                                       &out.count),
                "orbx_project_landmarks");
  return out;
}

struct GatedMatches {
  std::vector<int32_t> origin;      // per query: the train slot, or -1
  std::vector<int32_t> dist;        // per query: the Hamming distance to it, or -1
  std::vector<int32_t> candidates;  // per query: the train slots inside its gate
  int32_t count = 0;                // the accepted queries
};
// train_pstate: one orbx_proj_state per train slot (ProjectedLandmarks::state), or empty: every slot is positioned
inline GatedMatches reassociate_gated(const std::vector<ORBDescriptor>& query_desc,
                                      const std::vector<int32_t>& query_state, const std::vector<Point2f>& query_xy,
                                      const std::vector<ORBDescriptor>& train_desc,
                                      const std::vector<int32_t>& train_state, const std::vector<Point2d>& train_xy,
                                      const std::vector<int32_t>& train_pstate, double radius_px, double ratio = 0.8,
                                      int max_distance = 256, bool accept_lone = false, bool unique = true) {
  static_assert(sizeof(ORBDescriptor) == sizeof(orbx_descriptor) && sizeof(Point2f) == 2 * sizeof(float) &&
                    sizeof(Point2d) == 2 * sizeof(double),
                "layouts");
  if (query_desc.size() != query_state.size() || query_desc.size() != query_xy.size())
    throw std::invalid_argument("reassociate_gated: query_desc, query_state and query_xy differ in size");
  if (train_desc.size() != train_state.size() || train_desc.size() != train_xy.size() ||
      (!train_pstate.empty() && train_pstate.size() != train_desc.size()))
    throw std::invalid_argument("reassociate_gated: the train arrays differ in size");
  const int nq = (int)query_desc.size(), nt = (int)train_desc.size();
  GatedMatches out;
  out.origin.assign((size_t)nq, -1);
  out.dist.assign((size_t)nq, -1);
  out.candidates.assign((size_t)nq, 0);
  orbx_ctx* c = detail::stage_ctx()->get(8, 8);
  detail::check(c,
                orbx_reassociate_gated(c, reinterpret_cast<const orbx_descriptor*>(query_desc.data()),
                                       query_state.data(), reinterpret_cast<const float*>(query_xy.data()), nq,
                                       reinterpret_cast<const orbx_descriptor*>(train_desc.data()), train_state.data(),
                                       nt > 0 ? &train_xy[0].x : nullptr,
                                       train_pstate.empty() ? nullptr : train_pstate.data(), nt, radius_px, ratio,
                                       max_distance, accept_lone ? 1 : 0, unique ? 1 : 0, out.origin.data(),
                                       out.dist.data(), &out.count, out.candidates.data()),
                "orbx_reassociate_gated");
  return out;
}

// ---- Shi-Tomasi corners (next row) ----------------------------------
// cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance)
//                                           src/with_bundle_adjustment.cpp:586-593, src/t.cpp:285
// (no mask, blockSize 3, gradientSize 3, minimum eigenvalue: the defaults the reference leaves in place).
// The handle owns the context, hence the workspace of the detector, as LKTracker owns its pyramids.
class CornerDetector {
 public:
  CornerDetector() : ctx_([] {
    orbx_params p = detail::gpu_defaults();
    p.nlevels = 1;
    return std::make_shared<detail::Ctx>(p);
  }()) {}
  orbx_ctx* get(int w, int h) { return ctx_->get(w, h); }

 private:
  std::shared_ptr<detail::Ctx> ctx_;
};

// corners are ASSIGNED; maxCorners <= 0: no limit
inline void goodFeaturesToTrack(CornerDetector& handle, const Image& image, std::vector<Point2f>& corners,
                                int maxCorners, double qualityLevel, double minDistance) {
  static_assert(sizeof(Point2f) == 2 * sizeof(float), "point layout");
  orbx_ctx* c = handle.get(image.width, image.height);
  int count = 0;
  // sized for the usual case first; ORBX_ERR_CAPACITY reports what an unlimited call needs
  size_t capacity = maxCorners > 0 ? (size_t)maxCorners : 4096;
  for (;;) {
    corners.resize(capacity);
    const int st = orbx_good_features_to_track(c, image.data, image.width, image.height, image.stride, maxCorners,
                                               qualityLevel, minDistance, reinterpret_cast<float*>(corners.data()),
                                               (int)capacity, &count);
    if (st == ORBX_ERR_CAPACITY && (size_t)count > capacity) {
      capacity = (size_t)count;
      continue;
    }
    if (st != ORBX_OK) corners.clear();
    detail::check(c, st, "goodFeaturesToTrack");
    break;
  }
  corners.resize((size_t)count);
}
#ifdef ORBX_WITH_OPENCV
inline void goodFeaturesToTrack(CornerDetector& handle, const cv::Mat& image, std::vector<cv::Point2f>& corners,
                                int maxCorners, double qualityLevel, double minDistance) {
  std::vector<Point2f> out;
  goodFeaturesToTrack(handle, Image(image), out, maxCorners, qualityLevel, minDistance);
  corners.clear();
  for (const Point2f& p : out) corners.emplace_back(p.x, p.y);
}
#endif

// cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance, mask) -- the argument the reference
// leaves empty (src/with_bundle_adjustment.cpp:586-593): a pixel whose mask byte is 0 is no corner and does not count
// for the maximum that qualityLevel scales.  corners are ASSIGNED; maxCorners <= 0: no limit.
inline void goodFeaturesToTrack(CornerDetector& handle, const Image& image, std::vector<Point2f>& corners,
                                int maxCorners, double qualityLevel, double minDistance, const Image& mask) {
  if (mask.width != image.width || mask.height != image.height)
    throw std::runtime_error("goodFeaturesToTrack: mask and image differ in size");
  orbx_ctx* c = handle.get(image.width, image.height);
  int count = 0;
  size_t capacity = maxCorners > 0 ? (size_t)maxCorners : 4096;
  for (;;) {
    corners.resize(capacity);
    const int st = orbx_good_features_to_track_masked(c, image.data, image.width, image.height, image.stride,
                                                      mask.data, mask.stride, maxCorners, qualityLevel, minDistance,
                                                      reinterpret_cast<float*>(corners.data()), (int)capacity, &count);
    if (st == ORBX_ERR_CAPACITY && (size_t)count > capacity) {
      capacity = (size_t)count;
      continue;
    }
    if (st != ORBX_OK) corners.clear();
    detail::check(c, st, "goodFeaturesToTrack (mask)");
    break;
  }
  corners.resize((size_t)count);
}

// What a KLT front-end does between two windows, goodFeaturesToTrack(img, maxCorners - alive, q, d, mask around the
// live tracks) -- the reference's own answers are a fresh detection (src/with_bundle_adjustment.cpp:586-593) or ORB
// plus the matcher below 150 survivors (src/feature_tracking.cpp:68-71).  The usable tracked points come first, in
// their order, then new corners at least minDistance from every one of them; origin[i] is the index into `tracked`
// a point came from, -1 for a new corner.
struct ToppedUp {
  std::vector<Point2f> points;
  std::vector<int32_t> origin;
  int carried = 0;
};
inline ToppedUp top_up_keypoints(CornerDetector& handle, const Image& img, const std::vector<Point2f>& tracked,
                                 int maxCorners, double qualityLevel, double minDistance) {
  orbx_ctx* c = handle.get(img.width, img.height);
  ToppedUp out;
  const size_t capacity = (size_t)std::max(maxCorners, 1);
  out.points.resize(capacity);
  out.origin.resize(capacity);
  int count = 0;
  const int st = orbx_good_features_topup(c, img.data, img.width, img.height, img.stride,
                                          reinterpret_cast<const float*>(tracked.data()), (int)tracked.size(),
                                          maxCorners, qualityLevel, minDistance,
                                          reinterpret_cast<float*>(out.points.data()), out.origin.data(),
                                          (int)capacity, &count, &out.carried);
  detail::check(c, st, "top_up_keypoints");
  out.points.resize((size_t)count);
  out.origin.resize((size_t)count);
  return out;
}

// The initial keypoints of run_bundle_adjustment (src/with_bundle_adjustment.cpp:586-593): the caller's
// observations of frame 0 if there are any, else goodFeaturesToTrack(img0, 2000, 0.01, 8).
inline std::vector<Point2f> initial_keypoints(CornerDetector& handle, const std::vector<Point2d>& observations0,
                                              const Image& img0) {
  std::vector<Point2f> keypoints0;
  if (!observations0.empty()) {
    for (const Point2d& p : observations0) {
      Point2f q;
      q.x = (float)p.x, q.y = (float)p.y;
      keypoints0.push_back(q);
    }
  } else {
    goodFeaturesToTrack(handle, img0, keypoints0, 2000, 0.01, 8);
  }
  return keypoints0;
}

}  // namespace orbx
