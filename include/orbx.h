/* orbx.h -- C ABI of the MI355X-native ORB feature front-end (liborbx.so).
 *
 * Drop-in boundary for the reference's `orb.hpp` detectAndCompute path
 * (WeeFav/Visual-Odometry-GPU).  Every entry point names the reference
 * interface it replaces (paths relative to the reference root).  Plain
 * pointers and sizes only; no C++ or torch types.  All functions return an
 * orbx_status (0 = ok); none of them calls exit() or prints.
 *
 * A context owns every device allocation (pyramids, masks, candidate and
 * result slots for `max_batch` frames of up to max_width x max_height), its
 * own HIP stream, and is single-threaded; distinct contexts are independent
 * (one per GPU / per host thread).  Nothing is allocated on the per-frame
 * path.
 */
#ifndef ORBX_H
#define ORBX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_MAX_LEVELS 16

typedef enum {
  ORBX_OK = 0,
  ORBX_ERR_INVALID_ARG = 1,  /* bad pointer / size / parameter */
  ORBX_ERR_CAPACITY = 2,     /* caller buffer too small; *count still reports the required size */
  ORBX_ERR_HIP = 3,          /* HIP runtime error; see orbx_last_error_string */
  ORBX_ERR_NO_DEVICE = 4,    /* no gfx950 device / kernels not loadable */
  ORBX_ERR_UNSUPPORTED = 5   /* parameter combination outside the supported range */
} orbx_status;

/* include/orb.hpp:4  struct Keypoint { int x, y; } */
typedef struct {
  int32_t x, y;
} orbx_keypoint;

/* include/orb.hpp:6-8  struct ORBDescriptor { uint8_t data[32]; }
 * bit i lives at data[i>>3] & (1 << (i&7))  (src/orb_cpu.cpp:251) */
typedef struct {
  uint8_t data[32];
} orbx_descriptor;

typedef enum {
  /* GPU flavour, src/orb.cpp:58-109: per level FAST cap = 2*quota in row-major
   * order, Harris response, keep the `quota` best, output sorted by
   * (response desc, row-major index asc) within a level. */
  ORBX_SELECT_HARRIS = 0,
  /* CPU flavour, src/orb_cpu.cpp:271-276: keep the first `cap` NMS survivors
   * in row-major order, no Harris (responses are reported as 0). */
  ORBX_SELECT_ROWMAJOR = 1
} orbx_select_mode;

typedef enum { ORBX_BLUR_NONE = 0, ORBX_BLUR_UPPER = 1, ORBX_BLUR_ALL = 2 } orbx_blur_levels;
typedef enum { ORBX_BLUR_SEP16 = 0, ORBX_BLUR_K273 = 1 } orbx_blur_kind;

/* One POD for every knob of both reference flavours (SURVEY.md §5 "Config"). */
typedef struct {
  int32_t nfeatures;     /* ORB(nfeatures=500)            include/orb.hpp:36 */
  float scale_factor;    /* ORB(scaleFactor=1.2f)         include/orb.hpp:36 */
  int32_t nlevels;       /* ORB(nlevels=8)                include/orb.hpp:36 */
  int32_t threshold;     /* OrientedFAST(threshold=20)    include/orb.hpp:12 */
  int32_t n;             /* OrientedFAST(n=9)             include/orb.hpp:12 */
  int32_t nms_window;    /* OrientedFAST(nms_window=3)    include/orb.hpp:12 */
  int32_t patch_size;    /* OrientedFAST(patch_size=31)   include/orb.hpp:12 */
  int32_t harris_window; /* HarrisScore(..., 7, ...)      src/orb.cpp:65 */
  float harris_k;        /* HarrisScore(..., 0.04)        src/orb.cpp:65 */
  int32_t select_mode;   /* orbx_select_mode */
  int32_t blur_levels;   /* orbx_blur_levels: none = src/orb.cpp:111-120, upper = src/orb_cpu.cpp:278-290 */
  int32_t blur_kind;     /* orbx_blur_kind: src/cuda/GaussianBlur1D.cu / src/cuda/GaussianBlur.cu */
  int32_t max_width;     /* largest frame the context must handle */
  int32_t max_height;
  int32_t max_batch;     /* frames in flight per batched call */
  int32_t device;        /* HIP device ordinal, -1 = current device */
} orbx_params;

typedef struct orbx_ctx orbx_ctx;

/* Defaults of the GPU flavour: ORB(500,1.2f,8) + OrientedFAST(20,9,3,31)
 * (include/orb.hpp:12,36), HarrisScore(7,0.04) (src/orb.cpp:65), no blur. */
int orbx_params_default_gpu(orbx_params* p);
/* Defaults of the CPU flavour: OrientedFASTCPU(3000,50,9,3,9), one level,
 * row-major selection (include/orb_cpu.hpp:6, src/orb_cpu.cpp:271-276). */
int orbx_params_default_cpu(orbx_params* p);

/* replaces the ORB / OrientedFAST / RotatedBRIEF constructors
 * (src/orb.cpp:10-56); no stdout noise. */
int orbx_create(const orbx_params* p, orbx_ctx** out);
void orbx_destroy(orbx_ctx* ctx);

/* replaces cudaCheckErrors -> fprintf + exit(1) (src/cuda/Fast.cu:8-18).
 * ctx may be NULL (reports the last create failure of this thread). */
const char* orbx_last_error_string(const orbx_ctx* ctx);
const char* orbx_status_string(int status);
/* "liborbx <version> gfx950" */
const char* orbx_version(void);

/* Per-level geometry the context derived for a w x h frame (src/orb.cpp:62,
 * :117-118): sizes, quota and FAST cap.  Arrays must hold nlevels entries. */
int orbx_get_plan(orbx_ctx* ctx, int width, int height, int32_t* level_w, int32_t* level_h, int32_t* quota,
                  int32_t* fast_cap, float* level_scale, int32_t* out_capacity);

/* ---- whole path ---------------------------------------------------------- */

/* ORB::detectAndCompute(image, keypoints, orientations, descriptors)
 * (include/orb.hpp:37, src/orb.cpp:58-109; CPU twin src/orb_cpu.cpp:271-276).
 * Host image in, host arrays out (ASSIGN semantics).
 * keypoints are in level-0 coordinates ((int)(x*scale_l), src/orb.cpp:94-98).
 * responses / levels / level_kps may be NULL.  *count = keypoints produced;
 * if it exceeds `capacity` only `capacity` entries are written and
 * ORBX_ERR_CAPACITY is returned. */
int orbx_detect_and_compute(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                            orbx_keypoint* keypoints, float* orientations, orbx_descriptor* descriptors,
                            float* responses, int32_t* levels, orbx_keypoint* level_kps, int capacity,
                            int* count);

/* Batched, device-resident variant (the benchmark path; BASELINE.json configs
 * 2-4): `n` frames already in HBM at d_frames + i*frame_stride, each
 * height rows of row_stride bytes.  Runs asynchronously on the context's
 * stream (or `stream`, a hipStream_t, if non-NULL); results stay in the
 * context's device-side result slots until the next batched call.
 * Strides and alignment: a frame may be a region of a larger image and the frames may have gaps between them.
 *   - d_frames, row_stride and frame_stride need NO alignment: any byte address, any residue (the kernels read
 *     the frame with byte-granular buffer descriptors and unaligned loads);
 *   - row_stride >= width, and frame_stride >= row_stride * (height - 1) + width (frames do not overlap; the last
 *     row of a frame need not be followed by row_stride - width padding bytes);
 *   - row_stride * (height - 1) + width <= 2^31 - 1 (a frame is addressed with 32-bit offsets);
 *   - 8 <= width <= max_width, 8 <= height <= max_height, 1 <= n <= max_batch.
 * Anything else is ORBX_ERR_INVALID_ARG and leaves the context usable.  Only the width x height pixels of each
 * frame are ever read: the bytes between rows and between frames may hold anything and never influence a result
 * (tests/test_batch_inputs.py).  The frame size may change from call to call (the tables of the new size are
 * rebuilt, which waits for the batches in flight). */
int orbx_detect_and_compute_batch_device(orbx_ctx* ctx, const void* d_frames, int n, int width, int height,
                                         int row_stride, size_t frame_stride, void* stream);
/* Same for `n` host frames (H2D copy from the caller's memory included; pass pinned memory for an
 * asynchronous copy, pageable memory is staged by the HIP runtime).  The same rules for row_stride and frame_stride
 * (frame_stride is not looked at when n == 1; no 2^31 limit: the frames are packed tightly on their way to the
 * device). */
int orbx_detect_and_compute_batch_host(orbx_ctx* ctx, const uint8_t* frames, int n, int width, int height,
                                       int row_stride, size_t frame_stride);
/* Blocks until the last batched call has finished. */
int orbx_wait(orbx_ctx* ctx);

/* Device-side result slots of the last batch (fixed stride `slot_capacity`
 * entries per frame), for consumers that stay on the GPU. */
typedef struct {
  const int32_t* counts;            /* [n] */
  const orbx_keypoint* keypoints;   /* [n][slot_capacity] level-0 coords */
  const orbx_keypoint* level_kps;   /* [n][slot_capacity] level coords */
  const float* orientations;        /* [n][slot_capacity] */
  const float* responses;           /* [n][slot_capacity] */
  const int32_t* levels;            /* [n][slot_capacity] */
  const orbx_descriptor* descriptors; /* [n][slot_capacity] */
  int32_t slot_capacity;
  int32_t n;
  const uint32_t* keypoints16;      /* [n][slot_capacity] the same level-0 coords packed, x | y << 16 (both <= 16384) */
} orbx_batch_view;
int orbx_batch_results_device(orbx_ctx* ctx, orbx_batch_view* view);

/* Copies frames [first, first+n) of the last batch to host arrays with
 * `capacity` entries per frame (any output may be NULL except counts). */
int orbx_batch_fetch(orbx_ctx* ctx, int first, int n, int32_t* counts, orbx_keypoint* keypoints,
                     float* orientations, orbx_descriptor* descriptors, float* responses, int32_t* levels,
                     orbx_keypoint* level_kps, int capacity);

/* Pipelined consumers (a VO loop that wants the keypoints of frame batch i on the host while
 * batch i+1 is being processed; the reference copies results back synchronously after every
 * kernel, src/cuda/Fast.cu:238-239, src/cuda/Brief.cu:131).  The context keeps a ring of FOUR result
 * blocks, one per batch in turn:
 *   orbx_detect_and_compute_batch_device(batch i);  orbx_batch_prefetch();
 *   orbx_detect_and_compute_batch_device(batch i+1);          -- kernels overlap the copy of i
 *   orbx_batch_fetch_previous(...)  -> results of batch i (waits for the copy only);  orbx_batch_prefetch();  ...
 * (The copy is the runtime's copy kernel behind a wait for the batch's end.  Enqueued once the previous batch's
 * results have been read, as above, it costs 5-7 % of the frame rate; enqueued right behind its batch it may sit in
 * a hardware queue in front of the other lane's kernels for the whole batch -- measured between 0.7 and 0.99 of the
 * rate without copies, depending on the streams the process has.  orbx_set_host_results below needs no copy at all.)
 * orbx_batch_prefetch starts an asynchronous D2H copy of the last batch's block into its pinned
 * mirror on the context's copy stream; orbx_batch_fetch / _previous then wait for that copy
 * instead of copying.  The results of batch i stay in its block until batch i+4 is submitted; the views
 * reach batch i (the last one) and batch i-1. */
int orbx_batch_prefetch(orbx_ctx* ctx);
/* The same for consumers that want what the reference's detectAndCompute returns and nothing else (keypoints,
 * orientations, descriptors: include/orb.hpp:37): only the counts | keypoints16 | orientations | descriptors
 * sections of the block are copied, the keypoints as packed 16-bit pairs -- 40 instead of 64 bytes per keypoint
 * slot, which is what keeps the copy under the host link's rate at the benchmark's frame rate.
 * orbx_batch_results_host then reports keypoints / responses / levels / level_kps as NULL (keypoints16 is always
 * there); a fetch unpacks the keypoints from keypoints16, and one that asks for responses / levels / level_kps
 * copies the remaining sections first (blocking). */
int orbx_batch_prefetch_compact(orbx_ctx* ctx);
/* Host results without a copy (default off): with enable = 1 the kernel that finishes a batch (orientation + BRIEF)
 * writes the compact record -- counts | keypoints16 | orientations | descriptors -- of every keypoint into the block's
 * PINNED HOST mirror as well, in coalesced stores that travel the host link while the kernel runs.
 * The block then counts as compact-copied from the moment its batch is enqueued: orbx_batch_prefetch_compact has
 * nothing to do (nothing is copied, no copy kernel competes with the next batch, the copy stream is not involved),
 * orbx_batch_prefetch copies the other sections, and the host views / fetches wait for the batch's end and deliver
 * the same bytes as before (orbx_batch_results_host without a preceding orbx_batch_prefetch: the compact view).  The device-side result block is written as always.  (The reference copies every stage's results back
 * with a blocking cudaMemcpy: src/cuda/Fast.cu:238-239, src/cuda/Brief.cu:131.)  bench.py: fps_with_d2h. */
int orbx_set_host_results(orbx_ctx* ctx, int enable);
/* Zero-copy host view of a result block: pointers into the context's PINNED mirror of the last batch
 * (previous = 0) or of the batch `previous` calls before it (1..3: the ring has four blocks), same layout
 * as the device view (fixed stride `slot_capacity` entries per frame; only the first counts[f] entries of
 * frame f are valid).  Waits for the block's copy (starts it if orbx_batch_prefetch was not called).  The
 * view stays valid until the block is written again, i.e. until the fourth batched call after the one it
 * belongs to.  A streaming consumer that reads batch i - 2 while batches i - 1 and i run keeps both lanes of
 * the pipelined mode busy (bench.py: fps_with_d2h). */
int orbx_batch_results_host(orbx_ctx* ctx, int previous, orbx_batch_view* view);
int orbx_batch_fetch_previous(orbx_ctx* ctx, int first, int n, int32_t* counts, orbx_keypoint* keypoints,
                              float* orientations, orbx_descriptor* descriptors, float* responses, int32_t* levels,
                              orbx_keypoint* level_kps, int capacity);

/* Per-stage device timings (ms) of the last batched call, in order:
 * pyramid, blur, fast+nms, compact, harris, select, orient+brief, total. */
#define ORBX_NUM_STAGE_TIMES 8
/* enable: 0 = off, 1 = events around every stage, 2 = only around the two
 * roofline stages (blur, fast+nms; the other entries and `total` read 0). */
int orbx_enable_stage_timing(orbx_ctx* ctx, int enable);
int orbx_last_stage_times(orbx_ctx* ctx, float* ms);
/* Same for the timed batched call `back` calls ago (0 = the last one; up to
 * ORBX_EVENT_SETS-1): several timed calls may be enqueued back to back and read
 * after one orbx_wait(), so timing adds no host synchronisation between steps. */
#define ORBX_EVENT_SETS 64
int orbx_stage_times_history(orbx_ctx* ctx, int back, float* ms);

/* FAST/NMS tiles that provably cannot contribute to the first `cap` row-major
 * survivors exit early in the batched path (results are identical either way;
 * DESIGN.md "Early exit").  enable = 0 makes every tile do the full work (used
 * to measure the kernel's full-work throughput).  Default: enabled. */
int orbx_set_fast_early_exit(orbx_ctx* ctx, int enable);

/* With blur on every level (ORBX_BLUR_ALL, separable kind) the batched path builds and blurs the
 * pyramid in ONE kernel (buildPyramid + GaussianBlur of src/orb_cpu.cpp:278-290 fused: the
 * un-blurred pyramid is never written).  enable = 0 runs the two kernels separately (identical
 * results; used to time / profile each kernel on its own).  Default: enabled. */
int orbx_set_fused_pyramid_blur(orbx_ctx* ctx, int enable);

/* Diagnostics of the last whole-path batch: how many FAST/NMS tiles did the full
 * work (`worked`) out of all tiles of the batch (`total`); the rest took the early
 * exit.  With the early exit disabled worked == total. */
int orbx_fast_tile_counts(orbx_ctx* ctx, long long* worked, long long* total);

/* Top-rows-first pyramid (whole path, blur on every level, FAST early exit on, large batches): the pyramid
 * rows the top FAST tile rows need are produced first, FAST runs on those tile rows, and the remaining rows
 * of a level are produced only if the level does not yet hold its `cap` survivors -- keypoints are kept in
 * row-major order up to the cap (src/orb_cpu.cpp:108-110, src/orb.cpp:63), so nothing below is ever read.
 * Results are identical in every mode.  mode 0: never (one pass), 1: whenever eligible, 2 (default): adaptive
 * -- the second pass reports how many levels it could skip, and while that is less than a quarter the batches
 * run in one pass (with a probe every 128th batch); and the DEPTH of the first pass follows the stream: the
 * selection reports in which row each level's cap filled, and the FAST tile rows of the level are sized so that
 * the first pass ends just below it (the work is re-partitioned a few times per stream; never a result changes). */
int orbx_set_top_rows_first(orbx_ctx* ctx, int mode);

/* DEBUG entry, for tests only (not part of the product path, never called by bench.py): fills the working pools of
 * both lanes -- pyramids, survivor masks, tile-row statistics, candidate / response / level-candidate pools and
 * their counts -- with `byte` (0..255), after waiting for everything in flight.  Every batch must compute the same
 * results whatever the pools held before it.  Of the blurred pyramid only the pixels of the current frame size's
 * levels are filled: the padding bytes of its levels are the one thing in the pools that has to stay zero. */
int orbx_debug_fill_pools(orbx_ctx* ctx, int byte);

/* DEBUG entry, for tests only: reads back one level of one frame of the blurred pyramid of the current lane -- what
 * the last whole-path batch left in its pool -- after waiting for everything in flight: level_w x level_h bytes of the
 * current frame size's plan, rows packed, into `out` (`out_bytes` >= level_w * level_h).  Rows that the top-rows-first
 * pipeline did not produce hold whatever the pool held before the batch. */
int orbx_debug_read_pyramid_level(orbx_ctx* ctx, int frame, int level, uint8_t* out, size_t out_bytes);

/* Pipelined batches (default off).  With enable = 1, consecutive orbx_detect_and_compute_batch_device calls on the
 * context's own stream (stream = NULL) alternate between two LANES -- each with its own stream and its own working
 * pools; batch k uses the lane of its result block -- so the kernels of one batch overlap the tails and the nearly
 * empty launches of the other (KITTI, 256 frames per batch: ~8 % more frames/s).  Results are unchanged.  What a
 * caller may do between two such calls without losing the overlap: orbx_batch_prefetch, orbx_batch_results_host /
 * orbx_batch_fetch_previous (they follow the result block's own events); orbx_wait and orbx_batch_fetch wait for the
 * batches concerned; set_plan (a new frame size), the stage operators that use the pools, orbx_batch_match_consecutive
 * and orbx_destroy wait for both lanes first.  Costs a second set of pools (the first call allocates it; if that
 * fails -- ORBX_ERR_HIP -- what had been allocated is freed and the mode stays off).  Batches on a caller's stream,
 * host-frame batches and single frames are not pipelined, and may be mixed freely with pipelined ones: a batch that
 * comes to a lane's pools or to a result block on another stream than their previous user makes its stream wait
 * for that user's event (device-side, no host stall). */
int orbx_set_pipelined_batches(orbx_ctx* ctx, int enable);

/* Same for the pyramid: pyramid pixels the last whole-path batch PRODUCED out of all pyramid pixels of its
 * frames.  With blur on every level, the FAST early exit on and a large batch, the pyramid is built top rows
 * first and the remaining rows of a level are produced only if its top FAST tile rows did not already hold
 * the level's `cap` survivors (they are never read otherwise; results are identical).  Otherwise
 * produced == total. */
int orbx_pyramid_pixel_counts(orbx_ctx* ctx, long long* produced, long long* total);

/* Runs only the blur + FAST/NMS stages of the last-built pyramid `reps` times
 * (the roofline kernels) and reports the average duration of
 * each, measured with HIP events on the context's stream. */
int orbx_bench_stage(orbx_ctx* ctx, int n_frames, int stage, int reps, float* avg_ms);
#define ORBX_STAGE_PYRAMID 0
#define ORBX_STAGE_BLUR 1
#define ORBX_STAGE_FAST 2
#define ORBX_STAGE_COMPACT 3
#define ORBX_STAGE_HARRIS 4
#define ORBX_STAGE_SELECT 5
#define ORBX_STAGE_DESCRIBE 6

/* ---- stage-level operators (host buffers; each testable alone) ----------- */

/* d_Fast (src/cuda/Fast.cu:30-209) / OrientedFASTCPU::detect part 1
 * (src/orb_cpu.cpp:23-103): scores[h*w] float, 0 where not a corner. */
int orbx_fast_score(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, int threshold, int n,
                    float* scores);

/* NMS(scores, keypoints, nms_window, nfeatures, threshold)
 * (include/NMS.cuh:5, src/cuda/NMS.cu:21-161) with the CPU flavour's
 * deterministic row-major order and cap (src/orb_cpu.cpp:105-134).
 * *count = min(survivors, nfeatures); *total (optional) = survivors. */
int orbx_nms(orbx_ctx* ctx, const float* scores, int width, int height, int nms_window, int nfeatures,
             float threshold, orbx_keypoint* keypoints, int* count, int* total);

/* Fast(image, keypoints, threshold, n, nms_window, nfeatures) -> count
 * (include/Fast.cuh:5, src/cuda/Fast.cu:211-269); OrientedFAST::detect
 * (src/orb.cpp:22-27), OrientedFASTCPU::detect (src/orb_cpu.cpp:23-137). */
int orbx_fast(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, int threshold, int n,
              int nms_window, int nfeatures, orbx_keypoint* keypoints, int* count, int* total);

/* Orientations(image, keypoints, orientations, patch_size)
 * (include/Fast.cuh:6, src/cuda/Orientations.cu:22-97;
 * src/orb_cpu.cpp:139-183). */
int orbx_orientations(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                      const orbx_keypoint* keypoints, int nkp, int patch_size, float* orientations);

/* Brief(image, keypoints, orientations, descriptors, 256, 31)
 * (include/Brief.cuh:5, src/cuda/Brief.cu:40-136; src/orb_cpu.cpp:203-258). */
int orbx_brief(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
               const orbx_keypoint* keypoints, const float* orientations, int nkp, orbx_descriptor* descriptors);

/* HarrisScore(image, keypoints, scores, corner_window, k)
 * (include/HarrisScore.cuh:5, src/cuda/HarrisScore.cu:23-89; intent, see
 * DESIGN.md "Harris"). */
int orbx_harris(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                const orbx_keypoint* keypoints, int nkp, int window, float k, float* responses);

/* GaussianBlur1D(image, dst) (include/GaussianBlur.cuh:4,
 * src/cuda/GaussianBlur1D.cu:34-163): separable [1 4 6 4 1]/16, REFLECT_101. */
int orbx_blur5_sep(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                   int dst_stride);
/* GaussianBlur(image, dst) (include/GaussianBlur.cuh:3,
 * src/cuda/GaussianBlur.cu:35-130): 5x5 /273, REFLECT_101. */
int orbx_blur5_273(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, uint8_t* dst,
                   int dst_stride);

/* conv2d(image, dst, kernel, kernel_size) (include/Convolution.cuh:5,
 * src/cuda/Convolution.cu:20-101): valid KxK correlation of a pre-padded u8
 * image, float accumulate, result rounded half-to-even and saturated to u8.
 * dst is (height-K+1) x (width-K+1), pitch width-K+1. */
int orbx_conv2d(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, const float* kernel,
                int kernel_size, uint8_t* dst);
/* GaussianBlurCUDA(image, dst, kernel_size) (include/GaussianBlur.hpp:6,
 * src/GaussianBlur.cpp:39-49). dst pitch = width. */
int orbx_gaussian_blur_conv(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                            int kernel_size, uint8_t* dst);
/* createGaussianKernel(kernelSize, sigma) (src/GaussianBlur.cpp:7-37). */
int orbx_gaussian_kernel(int kernel_size, float sigma, float* kernel);
/* SobelCUDA(image, dst, dir) (include/Sobel.hpp:6, src/Sobel.cpp:18-32). */
int orbx_sobel(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, int dir, uint8_t* dst);

/* ORB::buildPyramid (src/orb.cpp:111-120; with blur src/orb_cpu.cpp:278-290):
 * writes level `level` (tightly packed, pitch = level width) to dst. */
int orbx_build_pyramid_level(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, int level,
                             uint8_t* dst, int* level_w, int* level_h);

/* keep-top-N of src/orb.cpp:67-86 (intent): indices of the `keep` largest
 * responses ordered by (response desc, index asc). */
int orbx_select_top(orbx_ctx* ctx, const float* responses, int n, int keep, int32_t* indices, int* kept);

/* ---- next row: descriptor matching ------------------ */

/* flann->knnMatch(des1, des2, matches, 2) (src/feature_matching.cpp:166-168,
 * src/feature_tracking.cpp:203-204) as an EXACT brute-force Hamming 2-NN search
 * (the reference's FLANN LSH index is approximate).  idx/dist: nq x 2 (best,
 * second best; -1 when the train set has fewer descriptors); ties keep the lower
 * train index. */
int orbx_knn2(orbx_ctx* ctx, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
              int32_t* idx, int32_t* dist);

/* knnMatch + the ratio test `m.distance < ratio * n.distance`
 * (src/feature_matching.cpp:172-181; ratio = 0.8 there), matches in query order.
 * dist1 may be NULL.  *count = number of matches; ORBX_ERR_CAPACITY if > capacity. */
int orbx_match_ratio(orbx_ctx* ctx, const orbx_descriptor* query, int nq, const orbx_descriptor* train, int nt,
                     double ratio, int32_t* query_idx, int32_t* train_idx, int32_t* dist1, int capacity, int* count);

/* Device-resident: matches frame i (query) against frame i+1 (train) for every
 * consecutive pair of the last batch -- the VO loop's get_matches() shape -- on
 * the batch's stream, straight from the result slots (no host round trip). */
int orbx_batch_match_consecutive(orbx_ctx* ctx, double ratio);
/* matches of pair `pair` (frames pair, pair+1) of the last orbx_batch_match_consecutive. */
int orbx_batch_match_fetch(orbx_ctx* ctx, int pair, int32_t* query_idx, int32_t* train_idx, int32_t* dist1,
                           int capacity, int* count);

/* ---- next row: pyramidal Lucas-Kanade tracking ---------
 * Replaces
 *   cv::calcOpticalFlowPyrLK(img1, img2, pts1, pts2, status, err, cv::Size(21,21), 3,
 *       cv::TermCriteria(COUNT + EPS, 30, 0.01))            src/feature_tracking.cpp:175-181
 * (flags = 0, minEigThreshold = 1e-4: the defaults the reference leaves in place).
 * prev / next: 8-bit gray images of the same size.  prev == NULL: the `next` image of
 * the previous call on this context is this call's `prev` (the reference's
 * `img1 = img2.clone()`, src/feature_tracking.cpp:112; its pyramid is still on the
 * device).  prev_pts_xy / next_pts_xy: n (x, y) float pairs; status: n bytes (1 =
 * tracked); err (optional): n floats, mean absolute window difference at level 0.
 * A coordinate that is NaN, or whose floor does not fit an int32, is outside the image wherever a window position
 * is tested (the previous point, every Newton step, the error window): status 0 and err 0 at level 0, the level
 * skipped above it; the position is passed through as it is, NaN included (LK rule 9).
 * OpenCV is absent from the image this library was written in: the arithmetic
 * restates OpenCV 4.x's published algorithm (parity unpinned). */
int orbx_lk_track(orbx_ctx* ctx, const uint8_t* prev, int prev_stride, const uint8_t* next, int next_stride,
                  int width, int height, const float* prev_pts_xy, int n, float* next_pts_xy, uint8_t* status,
                  float* err, int win_size, int max_level, int max_iters, double epsilon);
/* number of pyramid levels calcOpticalFlowPyrLK would use for this geometry
 * (max_level + 1 unless a level would not be larger than the window); -1 on bad arguments */
int orbx_lk_pyramid_levels(int width, int height, int win_size, int max_level);

/* ---- next row: relative pose -------------------------------
 * Replaces the reference's get_pose,
 *   cv::findEssentialMat(pts1, pts2, K, cv::RANSAC, 0.999, 1.0, mask);
 *   cv::recoverPose(E, pts1, pts2, K, R, t, mask);
 * (both calls in src/feature_matching.cpp:185-206 and in src/feature_tracking.cpp:222-242)
 * OpenCV is absent from the image this library was written in: the algorithm keeps OpenCV 4.x's structure
 * (Nistér five-point RANSAC, Sampson error, RANSACUpdateNumIters, recoverPose's four candidates and
 * distanceThresh 50) and fixes every choice OpenCV leaves to its RNG or to LAPACK;
 * parity with OpenCV is unpinned.  K: row-major double[9] (fx = K[0], fy = K[4], cx = K[2], cy = K[5]).
 * Conventions: x2 = R x1 + t, |t| = 1; E has unit Frobenius norm.  Degenerate input (n < 5, no model, a
 * solver failure) returns ORBX_OK with inliers = good = 0, E = 0, R = I, t = 0 and an all-zero mask.
 * inliers: RANSAC inliers of E; good: those that triangulate in front of both cameras (the final mask);
 * iters: RANSAC iterations run.  The samples depend on (seed, iteration) only.
 * ORBX_ERR_INVALID_ARG (nothing is launched, no output is written): K NULL or with a non-finite fx, fy, cx or cy,
 * fx <= 0 or fy <= 0, a non-finite prob (a finite one is clamped to [0, 1]), a threshold that is negative or not
 * finite, max_iters outside [0, ORBX_POSE_MAX_ITERS], n < 0. */
/* An interface limit, not a measurement: a pair in which no model ever gets more than four inliers runs all
 * max_iters iterations inside one kernel launch. */
#define ORBX_POSE_MAX_ITERS 100000
/* get_pose on host arrays: pts*_xy are n float (x, y) pairs (matched keypoints or LK output); mask
 * (n bytes, may be NULL) receives recoverPose's final mask.  src/feature_matching.cpp:185-206,
 * src/feature_tracking.cpp:222-242 */
int orbx_estimate_pose(orbx_ctx* ctx, const float* pts1_xy, const float* pts2_xy, int n, const double* K, double prob,
                       double threshold, int max_iters, uint64_t seed, double* E, double* R, double* t, uint8_t* mask,
                       int32_t* inliers, int32_t* good, int32_t* iters);
/* Device-resident: poses every pair matched by the last orbx_batch_match_consecutive, on the batch's stream,
 * from the matches and both frames' level-0 keypoints (int -> float -> double), in the compact query order
 * orbx_batch_match_fetch returns.  ORBX_ERR_INVALID_ARG if the last batch has not been matched.
 * src/feature_matching.cpp:185-206, src/feature_tracking.cpp:222-242 */
int orbx_batch_pose_consecutive(orbx_ctx* ctx, const double* K, double prob, double threshold, int max_iters,
                                uint64_t seed);
/* results of pairs [first, first + n) of the last orbx_batch_pose_consecutive; E, R: 9 doubles per pair,
 * t: 3; any output may be NULL */
int orbx_batch_pose_fetch(orbx_ctx* ctx, int first, int n, double* E, double* R, double* t, int32_t* inliers,
                          int32_t* good, int32_t* iters);
/* the final mask of one pair, one byte per match in orbx_batch_match_fetch order; *count = match count,
 * ORBX_ERR_CAPACITY if > capacity */
int orbx_batch_pose_mask(orbx_ctx* ctx, int pair, uint8_t* mask, int capacity, int* count);

/* ---- next row: triangulation, relative scale, trajectory ----
 * Replaces the rest of the reference's per-frame VO step,
 *   double scale = get_scale(R, t, pts1, pts2, points_3d);      src/feature_matching.cpp:70, :208-275
 *   T = [R | scale * t]; cur_pose = cur_pose * T.inv();          src/feature_matching.cpp:77-82
 * (src/feature_tracking.cpp:77-93, :244-310; src/feature_tracking_scale.py:127-164).
 * OpenCV is absent from the image this library was written in: cv::triangulatePoints' 4x4 SVD is a fixed-sweep
 * Jacobi iteration (DESIGN.md §9 rank 6 rule 1); parity with OpenCV is unpinned.  A point is valid iff its
 * homogeneous w is not 0 and its three float coordinates are finite; an invalid point is (0, 0, 0) with valid = 0
 * and enters no distance ratio. */
/* cv::triangulatePoints(K [I|0], K [R|t], pts1, pts2) + X/w -> cv::Point3f on host arrays: pts*_xy are n float
 * (x, y) pairs in pixels, K and R row-major double[9], t double[3]; xyz: 3 n floats, valid: n bytes.
 * src/feature_matching.cpp:216-245, src/feature_tracking.cpp:252-281 */
int orbx_triangulate(orbx_ctx* ctx, const float* pts1_xy, const float* pts2_xy, int n, const double* K,
                     const double* R, const double* t, float* xyz, uint8_t* valid);
/* the tail of get_scale on two index-aligned point lists: the upper median (nth_element at size / 2) of
 * |prev[i] - prev[i-1]| / (|cur[i] - cur[i-1]| + 1e-6) over i in [1, min(n_prev, n_cur)), clamped to [0.1, 5];
 * 1.0 when a list is empty or no ratio exists.  A ratio that is not finite (distances that overflow a float) counts
 * as no ratio.  The valid arrays may be NULL (all valid).  ORBX_ERR_UNSUPPORTED
 * beyond 20448 aligned points.  src/feature_matching.cpp:248-274, src/feature_tracking.cpp:284-309 */
int orbx_estimate_scale(orbx_ctx* ctx, const float* prev_xyz, const uint8_t* prev_valid, int n_prev,
                        const float* cur_xyz, const uint8_t* cur_valid, int n_cur, double* scale,
                        int32_t* ratios_used);
/* Device-resident: triangulates every match of every pair posed by the last orbx_batch_pose_consecutive and
 * estimates each pair's scale against its predecessor, on the batch's stream.  The two pairs' points are joined
 * on the shared frame's keypoint index (src/feature_tracking_scale.py:127-164: several queries on one keypoint:
 * the largest query index wins; triplets in ascending index order) and the predecessor's points are moved into
 * the shared frame with X' = R X + t.  Pair 0 has no predecessor: scale 1.0, 0 triplets.  K must be the K the
 * poses were computed with.  ORBX_ERR_INVALID_ARG if the last batch has not been posed (or another batch has
 * been enqueued since, or the match table has been rewritten by any matcher entry since the pose).  src/feature_matching.cpp:208-275 */
int orbx_batch_scale_consecutive(orbx_ctx* ctx, const double* K);
/* results of pairs [first, first + n) of the last orbx_batch_scale_consecutive; any output may be NULL.
 * src/feature_matching.cpp:70 */
int orbx_batch_scale_fetch(orbx_ctx* ctx, int first, int n, double* scale, int32_t* triplets, int32_t* ratios_used);
/* the triangulated points of one pair (the reference's points_3d, src/feature_matching.cpp:237-245), one per match
 * in orbx_batch_match_fetch order; *count = match count, ORBX_ERR_CAPACITY if > capacity */
int orbx_batch_points_fetch(orbx_ctx* ctx, int pair, float* xyz, uint8_t* valid, int capacity, int* count);
/* cur_pose = cur_pose * T.inv() with T = [R | scale * t] for n relative motions (src/feature_matching.cpp:77-82),
 * T^-1 in closed form [R^T | -scale R^T t].  Host only, needs no context.  T0: row-major 4x4; R: 9 n, t: 3 n,
 * scale: n doubles; poses: (n + 1) row-major 4x4, poses[0] = T0. */
int orbx_chain_trajectory(const double* T0, const double* R, const double* t, const double* scale, int n,
                          double* poses);

/* ---- next row: sliding-window bundle adjustment ---------------------
 * Replaces the reference's Ceres solve of one window of poses and landmarks,
 *   ReprojectionError: angle-axis + translation, world -> camera, pinhole      src/with_bundle_adjustment.cpp:27-68
 *   the problem: HuberLoss, pose 0 constant, SPARSE_SCHUR, 200 iterations      src/with_bundle_adjustment.cpp:612-679
 *   write-back only on CONVERGENCE                                             src/with_bundle_adjustment.cpp:683
 * as Levenberg-Marquardt with the Schur complement on the landmarks, one GPU workgroup per window, in binary64.
 * Ceres is absent from the image this library was written in: every choice it leaves to its internals is fixed
 * in DESIGN.md §9 rank 7; parity with Ceres is unpinned.
 * Pose block: 6 doubles, angle-axis (3) then translation (3); point block: 3 doubles, world frame.  A window has
 * 2 .. ORBX_BA_MAX_POSES poses and 1 .. 65536 landmarks (more: ORBX_ERR_UNSUPPORTED); every landmark has at least
 * one observation and every (landmark, pose) at most one.  Observations may come in any order.  The reference's
 * values are huber_delta = 1.0 and max_iters = 200.  ORBX_ERR_INVALID_ARG: an index out of range, a duplicate
 * (landmark, pose), a landmark without observation, a pose count outside [2, 8], huber_delta <= 0, max_iters outside
 * [1, 1000], a non-finite input.  On any error nothing is written. */
#define ORBX_BA_MAX_POSES 8
typedef enum {
  ORBX_BA_CONVERGENCE = 0,    /* a tolerance was reached: the blocks hold the solution */
  ORBX_BA_NO_CONVERGENCE = 1, /* max_iters iterations ran: the blocks are unchanged */
  ORBX_BA_FAILURE = 2,        /* non-finite initial cost, an observation at depth 0 at the start, or a rotation
                                 angle beyond 1e5 rad: the blocks are unchanged */
  ORBX_BA_SKIPPED = 3         /* a window of a landmarks block without landmarks (orbx_bundle_adjust_landmarks_device
                                 only): nothing was read, every other field of the summary is 0 */
} orbx_ba_termination;
typedef struct {
  int32_t termination; /* orbx_ba_termination */
  int32_t iterations;  /* trust-region iterations run */
  int32_t successful_steps;
  int32_t reserved;
  double initial_cost; /* 1/2 sum rho(|r|^2) */
  double final_cost;
} orbx_ba_summary;
/* run_bundle_adjustment's solve of one window on host arrays: K row-major double[9]; poses6: 6 n_poses doubles,
 * points3: 3 n_points doubles, both in / out (rewritten only on convergence); observation k sees landmark
 * obs_point[k] from pose obs_pose[k] at pixel obs_xy[2k], obs_xy[2k + 1].  src/with_bundle_adjustment.cpp:612-720 */
int orbx_bundle_adjust(orbx_ctx* ctx, const double* K, int n_poses, double* poses6, int n_points, double* points3,
                       int n_obs, const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                       double huber_delta, int max_iters, orbx_ba_summary* summary);
/* n_windows independent windows in one launch.  Window w owns poses [pose_offset[w], pose_offset[w + 1]), points
 * [point_offset[w], point_offset[w + 1]) and observations [obs_offset[w], obs_offset[w + 1]); each offset array has
 * n_windows + 1 entries and starts at 0; obs_point / obs_pose index inside the window.  A window's result does not
 * depend on the batch it is in.  summaries: n_windows entries.  src/with_bundle_adjustment.cpp:612-720 */
int orbx_bundle_adjust_batch(orbx_ctx* ctx, const double* K, int n_windows, const int32_t* pose_offset,
                             double* poses6, const int32_t* point_offset, double* points3, const int32_t* obs_offset,
                             const int32_t* obs_point, const int32_t* obs_pose, const double* obs_xy,
                             double huber_delta, int max_iters, orbx_ba_summary* summaries);

/* ---- next row: Shi-Tomasi corners --------------------------------------
 * Replaces
 *   cv::goodFeaturesToTrack(imgs_window[0], keypoints0, 2000, 0.01, 8)    src/with_bundle_adjustment.cpp:586-593
 *   the same call                                                         src/t.cpp:285
 * with the arguments the reference leaves at their defaults fixed: no mask, blockSize 3, gradientSize 3, minimum
 * eigenvalue (no Harris).  OpenCV is absent from the image this library was written in: the algorithm keeps OpenCV
 * 4.x's structure (cornerMinEigenVal, threshold at qualityLevel * max, 3x3 dilate maxima, sort, minimum-distance
 * grid) and fixes every choice OpenCV leaves to its SIMD build (rules 1-6); parity with OpenCV
 * is unpinned.  Corners are (float)x, (float)y pairs in acceptance order (strongest first; equal responses: the larger
 * row-major index first), ASSIGN semantics.
 * Arguments: 8 <= width <= max_width, 8 <= height <= max_height; quality_level finite, in (0, 1]; min_distance finite,
 * >= 0 (below 1: no suppression); anything else is ORBX_ERR_INVALID_ARG.  min_distance above
 * ORBX_GFTT_MAX_MIN_DISTANCE (the cell arithmetic is 32-bit; no frame a context accepts is a quarter as wide) is
 * ORBX_ERR_UNSUPPORTED.  max_corners <= 0: no limit (host entry only).  On any error nothing is written but *count
 * of ORBX_ERR_CAPACITY. */
#define ORBX_GFTT_MAX_MIN_DISTANCE 65536.0
/* cv::cornerMinEigenVal(image, eig, 3, 3) (the response map inside goodFeaturesToTrack,
 * src/with_bundle_adjustment.cpp:592): host image in, eig = height x width floats, tightly packed. */
int orbx_corner_min_eigen_val(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride, float* eig);
/* cv::goodFeaturesToTrack on one host image (src/with_bundle_adjustment.cpp:586-593, src/t.cpp:285).  *count =
 * corners found; if it exceeds `capacity`, ORBX_ERR_CAPACITY is returned, *count is the capacity required and
 * corners_xy is not written.  Runs as a good-features batch of one frame: it replaces the results of the last
 * orbx_good_features_batch_device. */
int orbx_good_features_to_track(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                                int max_corners, double quality_level, double min_distance, float* corners_xy,
                                int capacity, int* count);
/* The same for `n` frames in device memory, asynchronously on the context's stream (or `stream`, a hipStream_t):
 * the frame, stride and alignment rules of orbx_detect_and_compute_batch_device hold unchanged, and
 * max_corners >= 1.  The results go to a block of their OWN -- counts and min(max_corners, (width - 2)(height - 2))
 * corner slots per frame -- so the last ORB batch, its matches, poses and scales stay as they are.
 * src/with_bundle_adjustment.cpp:586-593
 * Workspace: 16 bytes per pixel and frame (response map, candidate pool for EVERY interior pixel, cell grid),
 * allocated at the first good-features call for min(max_batch, frames that fit the limit) frames of max_width x
 * max_height and freed by orbx_destroy; a batch of more frames runs in slices, one after the other on the same
 * stream, with identical results.  A caller's stream is used during the call only: later calls, fetches and
 * orbx_destroy wait for an event recorded behind the batch, so the stream may be destroyed once the call returns. */
int orbx_good_features_batch_device(orbx_ctx* ctx, const void* d_frames, int n, int width, int height, int row_stride,
                                    size_t frame_stride, int max_corners, double quality_level, double min_distance,
                                    void* stream);
/* The bound of that workspace in bytes (default ORBX_GFTT_WORKSPACE_DEFAULT; 0 restores it).  One frame of
 * max_width x max_height is always granted.  Waits for the good-features batch in flight and releases the
 * workspace; the next call allocates the new size.  src/with_bundle_adjustment.cpp:592 */
#define ORBX_GFTT_WORKSPACE_DEFAULT ((size_t)1 << 30)
int orbx_good_features_workspace_limit(orbx_ctx* ctx, size_t bytes);
/* Device-side results of the last good-features batch, for consumers that stay on the GPU (valid until the next
 * good-features call; written on the batch's stream). */
typedef struct {
  const int32_t* counts;   /* [n] */
  const float* corners_xy; /* [n][slot_capacity][2]; the first counts[f] of frame f are valid */
  int32_t slot_capacity;
  int32_t n;
} orbx_good_features_view;
int orbx_good_features_results_device(orbx_ctx* ctx, orbx_good_features_view* view);
/* Waits for the last good-features batch and copies frames [first, first + n): counts (n entries) and
 * corners_xy (n x slot_capacity x 2 floats, the view's stride; may be NULL).  src/with_bundle_adjustment.cpp:586-593 */
int orbx_good_features_fetch(orbx_ctx* ctx, int first, int n, int32_t* counts, float* corners_xy);

/* ---- next row: Lucas-Kanade over frame windows ---------------------------
 * Replaces
 *   trackPointsAcrossWindow: the points of a window's first frame followed frame by frame through the window, a
 *   track ending with the first pair that loses it                         src/with_bundle_adjustment.cpp:464-499
 *   track_optical_flow over a stream (windows of two frames)               src/feature_tracking.cpp:166-193
 * for n_windows windows of window_len consecutive frames each in ONE tracking launch per slice.  Every pair is
 * computed exactly as orbx_lk_track computes it (one text of the arithmetic in the kernels), and the point that
 * leaves a pair enters the next one with the same float bits.
 * Result layout (a block of its OWN; slot_capacity slots per window):
 *   tracks_xy[w][slot][k]  the point in frame window_first[w] + k; entry 0 is the input point (tracks[i][0])
 *   seen[w][slot]          frames the point was observed in, 1 .. window_len for a live slot
 *   err[w][slot][k - 1]    the error orbx_lk_track reports for the pair (k - 1, k)
 * Everything past `seen`, and every slot at or beyond counts[w], is written as 0: whole arrays compare equal.
 * A counts[w] above slot_capacity is clamped.
 * Arguments: the frame, stride and alignment rules of orbx_detect_and_compute_batch_device hold unchanged, with
 * 8 <= width <= max_width, 8 <= height <= max_height and 2 <= n_frames <= max_batch; win_size, max_level, max_iters,
 * epsilon as orbx_lk_track; window_len >= 2, n_windows >= 1, slot_capacity >= 1; window_first[w] >= 0 and
 * window_first[w] + window_len <= n_frames (windows may overlap and come in any order).  Anything else is
 * ORBX_ERR_INVALID_ARG: nothing is written, the previous windows result stays fetchable and the context usable.
 * The frames are read IN PLACE (level 0 of the pyramids is the caller's memory; it must stay unchanged until the call
 * has finished on the device); d_points_xy / d_counts may be the view of orbx_good_features_results_device.
 * Asynchronous on the context's stream (or `stream`, a hipStream_t).  A caller's stream is used during the call only:
 * later calls, fetches and orbx_destroy wait for an event recorded behind the batch.  The last ORB batch with its
 * matches, poses and scales, the good-features block and the state of orbx_lk_track (its cached pyramids and the
 * prev == NULL continuation) stay as they are.
 * Workspace: per frame of a slice the pyramid levels 1 .. top (bytes w_l * h_l, each level rounded up to 256) and
 * the int16 derivative pairs of the levels 0 .. top (4 * w_l * h_l, rounded likewise) -- with 4 levels
 * (1/3 - 1/192) + 4 * (4/3 - 1/192) = 5.64 bytes per pixel, 2.63 MB for a 1241 x 376 frame.  It is allocated on demand
 * for min(n_frames, max(frames that fit the limit, window_len)) frames and freed by orbx_destroy.  When the frames of
 * all windows do not fit, the windows run in slices of whole consecutive windows, one after the other on the same
 * stream, with identical results (a slice covers the frames from its lowest to its highest one). */
int orbx_lk_track_windows_device(orbx_ctx* ctx, const void* d_frames, int n_frames, int width, int height,
                                 int row_stride, size_t frame_stride,
                                 const int32_t* window_first /* host, [n_windows] */, int n_windows, int window_len,
                                 const float* d_points_xy /* device, [n_windows][slot_capacity][2] */,
                                 const int32_t* d_counts /* device, [n_windows]; NULL: every slot is a point */,
                                 int slot_capacity, int win_size, int max_level, int max_iters, double epsilon,
                                 void* stream);
/* Device-side results of the last windows call (valid until the next one; written on its stream).
 * src/with_bundle_adjustment.cpp:464-499 */
typedef struct {
  const float* tracks_xy; /* [n_windows][slot_capacity][window_len][2] */
  const int32_t* seen;    /* [n_windows][slot_capacity] */
  const float* err;       /* [n_windows][slot_capacity][window_len - 1] */
  int32_t slot_capacity, window_len, n_windows;
} orbx_lk_windows_view;
int orbx_lk_windows_results_device(orbx_ctx* ctx, orbx_lk_windows_view* view);
/* Waits for the last windows call and copies windows [first, first + n) in the view's layout; each of the three
 * arrays may be NULL.  src/with_bundle_adjustment.cpp:464-499 */
int orbx_lk_windows_fetch(orbx_ctx* ctx, int first, int n, float* tracks_xy, int32_t* seen, float* err);
/* The bound of the windows workspace in bytes (default ORBX_LK_WORKSPACE_DEFAULT; 0 restores it).  The frames of one
 * window are always granted.  Waits for the windows call in flight and releases the workspace; the next call
 * allocates the new size.  src/with_bundle_adjustment.cpp:464-499 */
#define ORBX_LK_WORKSPACE_DEFAULT ((size_t)1 << 30)
int orbx_lk_workspace_limit(orbx_ctx* ctx, size_t bytes);
/* Host convenience: ONE window of n_frames host frames (frame i at frames + i * frame_stride) and n host points in,
 * tracks_xy (n x n_frames x 2 floats), seen (n) and err (n x (n_frames - 1), may be NULL) out.  Synchronous; runs as
 * a windows batch of one window and replaces the last windows result.  n == 0: nothing is done.  The frames are staged
 * in a buffer of the entry's own, so n_frames is bounded by 65535, not by max_batch; every other rule is that of
 * orbx_lk_track_windows_device.
 * src/with_bundle_adjustment.cpp:464-499, src/feature_tracking.cpp:166-193 */
int orbx_lk_track_window(orbx_ctx* ctx, const uint8_t* frames, int n_frames, int width, int height, int row_stride,
                         size_t frame_stride, const float* pts_xy, int n, float* tracks_xy, int32_t* seen, float* err,
                         int win_size, int max_level, int max_iters, double epsilon);

/* ---- next row: landmarks of tracked windows, bundle-adjusted on the device ----------
 * Replaces
 *   buildLandmarksFromFirstTwoFramesAndTracks: baseline gate, P0 / P1 from the first two poses, linear
 *   triangulation of every track seen at least twice, "simple depth check"    src/with_bundle_adjustment.cpp:502-575
 *   the Ceres solve of the window built from them                              src/with_bundle_adjustment.cpp:612-720
 * for n_windows windows per call, from the tracks block of orbx_lk_track_windows_device to the solved poses without
 * a host round trip beyond the window poses.  Rules: the poses are BA's own blocks (angle-axis
 * then translation, world -> camera); the gate is 0.1 <= |t0 - t1| <= 100; the DLT runs in WORLD coordinates on the
 * first two pixels of a track widened to double, the point stays in binary64; a landmark is kept iff its slot has
 * seen >= 2, the homogeneous point is finite after the division and its world z is > 0.  Kept landmarks stand in
 * ascending slot order, each with the observations k = 0 .. seen - 1 of its slot in ascending k (`seen` outside
 * [0, window_len] is clamped); slot_of_point names the slot.  A window that is not ORBX_LM_OK owns no landmark and
 * no observation.  OpenCV is absent from the image this library was written in: parity with
 * cv::triangulatePoints / cv::SVD is unpinned. */
typedef enum {
  ORBX_LM_OK = 0,
  ORBX_LM_BASELINE = 1, /* |t0 - t1| outside [0.1, 100]                       src/with_bundle_adjustment.cpp:515-516 */
  ORBX_LM_EMPTY = 2,    /* the gate passed and no landmark was kept */
  ORBX_LM_BAD_POSE = 3  /* the rotation angle of pose 0 or 1 is beyond 1e5 rad */
} orbx_lm_status;
/* Builds the landmarks block of n_windows windows, asynchronously on the context's stream (or `stream`, a
 * hipStream_t).  d_tracks_xy / d_seen: device memory in the layout of orbx_lk_windows_view -- they may BE that view;
 * a call on another stream than the last windows call's waits for that call's event.  poses6: HOST,
 * n_windows x window_len x 6 doubles; K: host, row-major double[9].  ORBX_ERR_INVALID_ARG: window_len outside
 * [2, ORBX_BA_MAX_POSES], n_windows < 1, slot_capacity < 1, a NULL pointer, a non-finite K or pose.
 * ORBX_ERR_UNSUPPORTED: slot_capacity > 65536, or n_windows x (slot_capacity + 1) or n_windows x slot_capacity x
 * window_len beyond 32-bit offsets.  On any refusal nothing is written and the previous block stays fetchable.
 * The block is the entry's OWN, sized for every slot kept (57 + 17 window_len bytes per slot, scratch included): ORB
 * results, matches, poses, scales, the good-features block, the LK blocks and the state of orbx_bundle_adjust_batch
 * stay as they are.  A caller's stream is used during the call only: later calls, fetches and orbx_destroy wait for
 * an event recorded behind the call.  src/with_bundle_adjustment.cpp:502-575 */
int orbx_landmarks_build_device(orbx_ctx* ctx, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                                int n_windows, int slot_capacity, int window_len, const double* poses6, void* stream);
/* Device-side view of the last landmarks block (valid until the next build; written on its stream): exactly the
 * arrays k_ba_lm reads.  src/with_bundle_adjustment.cpp:502-575 */
typedef struct {
  const int32_t* status;        /* [n_windows] orbx_lm_status */
  const int32_t* pose_offset;   /* [n_windows + 1], w * window_len */
  const int32_t* point_offset;  /* [n_windows + 1] */
  const int32_t* obs_offset;    /* [n_windows + 1] */
  const double* points3;        /* [point_offset[n_windows]][3], world frame */
  const int32_t* rows;          /* window w: its landmarks + 1 row starts into its observations, at point_offset[w] + w */
  const uint8_t* obs_pose;      /* [obs_offset[n_windows]] */
  const double* obs_xy;         /* [obs_offset[n_windows]][2] */
  const int32_t* slot_of_point; /* [point_offset[n_windows]] */
  int32_t slot_capacity, window_len, n_windows;
} orbx_landmarks_view;
int orbx_landmarks_results_device(orbx_ctx* ctx, orbx_landmarks_view* view);
/* Waits for the last build and copies windows [first, first + n) in the format of orbx_bundle_adjust_batch's
 * arguments: status (n), pose_offset / point_offset / obs_offset (n + 1 each, starting at 0), points3,
 * slot_of_point, and the observations as obs_point / obs_pose (int32 indices inside the window) and obs_xy.  Every
 * array may be NULL.  *n_points / *n_obs = landmarks and observations of those windows; if one exceeds its capacity,
 * ORBX_ERR_CAPACITY is returned, the two counts are the capacities required and nothing else is written.
 * src/with_bundle_adjustment.cpp:502-575 */
int orbx_landmarks_fetch(orbx_ctx* ctx, int first, int n, int32_t* status, int32_t* pose_offset, int32_t* point_offset,
                         int32_t* obs_offset, double* points3, int32_t* slot_of_point, int point_capacity,
                         int32_t* obs_point, int32_t* obs_pose, double* obs_xy, int obs_capacity, int* n_points,
                         int* n_obs);
/* Solves every window of the last landmarks block as orbx_bundle_adjust_batch solves it (the same kernel, the same
 * bits), asynchronously on the context's stream (or `stream`), with the K of the build.  huber_delta and max_iters
 * as orbx_bundle_adjust_batch; without a landmarks block: ORBX_ERR_INVALID_ARG.  The solve works on copies of the
 * poses and points: the block stays as built, and a second solve starts from the same blocks.  A window that is not
 * ORBX_LM_OK reports ORBX_BA_SKIPPED and keeps its poses.  src/with_bundle_adjustment.cpp:612-720 */
int orbx_bundle_adjust_landmarks_device(orbx_ctx* ctx, double huber_delta, int max_iters, void* stream);
/* Waits for the last solve and copies windows [first, first + n): poses6 (n x window_len x 6), summaries (n) and the
 * points (in the order of the block; *count of them; ORBX_ERR_CAPACITY if > capacity, then *count is the capacity
 * required and nothing else is written).  Each array may be NULL.  src/with_bundle_adjustment.cpp:612-720 */
int orbx_bundle_adjust_landmarks_fetch(orbx_ctx* ctx, int first, int n, double* poses6, orbx_ba_summary* summaries,
                                       double* points3, int capacity, int* count);
/* Host convenience: ONE window of host tracks (n_slots x window_len x 2 floats), seen (n_slots) and poses6
 * (window_len x 6, in / out: rewritten only on convergence) through both stages as a batch of one; synchronous;
 * replaces the last landmarks block.  *lm_status: the window's orbx_lm_status; points3 / slot_of_point: the refined
 * landmarks and their slots, *count of them (capacity rule as above; both may be NULL).
 * src/with_bundle_adjustment.cpp:502-575, src/with_bundle_adjustment.cpp:612-720 */
int orbx_bundle_adjust_tracks(orbx_ctx* ctx, const double* K, const float* tracks_xy, const int32_t* seen, int n_slots,
                              int window_len, double* poses6, double huber_delta, int max_iters, int32_t* lm_status,
                              orbx_ba_summary* summary, double* points3, int32_t* slot_of_point, int capacity,
                              int* count);

/* ---- next row: pose and scale of tracked frame pairs, from LK windows ------------
 * Replaces the host side of the reference's tracking loop between the tracker and the trajectory:
 *   the "remove lost tracks" compaction of track_optical_flow                  src/feature_tracking.cpp:166-193
 *   get_pose on the surviving point lists                                      src/feature_tracking.cpp:222-242
 *   get_scale on them                                                          src/feature_tracking.cpp:244-310
 *   the same three steps in the bundle-adjustment executable                   src/with_bundle_adjustment.cpp:180-203
 * for every consecutive frame pair of n_windows tracked windows per call, from the tracks block of
 * orbx_lk_track_windows_device, with no host round trip.  Window w of window_len = L frames owns L - 1 pairs; the
 * global pair index is p = w * (L - 1) + k, pair k being frames k and k + 1 of the window.  Rules (DESIGN.md §9
 * rank 11): the list of pair k is the slots with seen >= k + 2 in ascending slot order (`seen` outside [0, L] is
 * clamped), point 1 = tracks_xy[w][slot][k], point 2 = tracks_xy[w][slot][k + 1]; the pose is rank 5 unchanged (the
 * same kernel, normalisation and (seed, iteration) sampling for every pair, the degenerate rule for n < 5); the
 * points are rank 6 rule 1 with the pair's own R, t; the scale of pair k >= 1 is rank 6 rules 3 / 4 against pair
 * k - 1 OF THE SAME WINDOW, the two lists joined on the slot (so triplets == n), triplets in ascending slot order;
 * pair 0 of every window reports scale 1.0, 0 triplets, 0 ratios.  The join on the slot is exact where the
 * reference aligns its two point lists by list position.  Overlapping windows of three frames
 * (window_first[i] = i) give a stream its per-frame scales (src/feature_tracking_scale.py:127-164). */
typedef struct {
  double E[9], R[9], t[3];
  int32_t inliers, good, iters, pad;
} orbx_tracks_pose_result;
typedef struct {
  double scale;
  int32_t triplets, ratios_used;
} orbx_tracks_scale_result;
/* Poses, triangulates and scales every pair of n_windows windows, asynchronously on the context's stream (or
 * `stream`, a hipStream_t).  d_tracks_xy / d_seen: device memory in the layout of orbx_lk_windows_view -- they may BE
 * that view; a call on another stream than the last windows call's waits for that call's event.  K, prob, threshold,
 * max_iters, seed: as orbx_batch_pose_consecutive.  ORBX_ERR_INVALID_ARG: the argument rules of
 * orbx_batch_pose_consecutive for K / prob / threshold / max_iters, any non-finite entry of K, a NULL pointer, n_windows < 1,
 * slot_capacity < 1, window_len < 2.  ORBX_ERR_UNSUPPORTED: slot_capacity above 10224 (the join holds 16 bytes per
 * slot in LDS), or n_windows x (window_len - 1) x slot_capacity beyond 32-bit offsets.  On any refusal nothing is
 * launched or written, the previous block stays fetchable and the context usable.  The block is the entry's OWN
 * (204 + 50 slot_capacity bytes per pair, scratch included): the ORB batch's matches, poses and scales, the
 * good-features block, both LK states, the landmarks block and the state of orbx_bundle_adjust_batch stay as they
 * are.  A caller's stream is used during the call only: later calls, fetches and orbx_destroy wait for an event
 * recorded behind the call.  src/feature_tracking.cpp:166-193, src/feature_tracking.cpp:222-242,
 * src/feature_tracking.cpp:244-310, src/with_bundle_adjustment.cpp:180-203 */
int orbx_tracks_pose_device(orbx_ctx* ctx, const double* K, const float* d_tracks_xy, const int32_t* d_seen,
                            int n_windows, int slot_capacity, int window_len, double prob, double threshold,
                            int max_iters, uint64_t seed, void* stream);
/* Device-side view of the last tracks-pose block (valid until the next call; written on its stream).  Every row past
 * n[p] is 0.  src/feature_tracking.cpp:222-242, src/feature_tracking.cpp:244-310 */
typedef struct {
  const orbx_tracks_pose_result* pose;   /* [n_pairs] */
  const int32_t* n;                      /* [n_pairs] correspondences of the pair */
  const orbx_tracks_scale_result* scale; /* [n_pairs] */
  const int32_t* slot_of;                /* [n_pairs][slot_capacity] the slot of each list position */
  const uint8_t* mask;                   /* [n_pairs][slot_capacity] recoverPose's final mask */
  const float* xyz;                      /* [n_pairs][slot_capacity][3] */
  const uint8_t* valid;                  /* [n_pairs][slot_capacity] */
  int32_t slot_capacity, window_len, n_windows, n_pairs;
} orbx_tracks_pose_view;
int orbx_tracks_pose_results_device(orbx_ctx* ctx, orbx_tracks_pose_view* view);
/* Waits for the last call and copies pairs [first_pair, first_pair + n): E, R 9 doubles per pair, t 3; counts = the
 * pairs' list lengths; any output may be NULL.  src/feature_tracking.cpp:66-93,
 * src/with_bundle_adjustment.cpp:180-203 */
int orbx_tracks_pose_fetch(orbx_ctx* ctx, int first_pair, int n, double* E, double* R, double* t, int32_t* inliers,
                           int32_t* good, int32_t* iters, int32_t* counts, double* scale, int32_t* triplets,
                           int32_t* ratios_used);
/* One pair's lists, one entry per surviving slot in ascending slot order: the slot, recoverPose's final mask, the
 * triangulated point and its valid byte; each array may be NULL.  *count = the pair's list length, ORBX_ERR_CAPACITY
 * if > capacity (nothing else is written).  src/feature_tracking.cpp:182-192, src/feature_tracking.cpp:252-281 */
int orbx_tracks_pose_pair_fetch(orbx_ctx* ctx, int pair, int32_t* slot_of, uint8_t* mask, float* xyz, uint8_t* valid,
                                int capacity, int* count);
/* Host convenience: ONE window of host tracks (n_slots x window_len x 2 floats) and seen (n_slots) as a batch of one;
 * synchronous; replaces the last tracks-pose block, whose lists orbx_tracks_pose_pair_fetch then delivers.  The
 * outputs hold window_len - 1 pairs each and may be NULL.  src/feature_tracking.cpp:166-193,
 * src/feature_tracking.cpp:222-242, src/feature_tracking.cpp:244-310, src/with_bundle_adjustment.cpp:180-203 */
int orbx_tracks_pose(orbx_ctx* ctx, const double* K, const float* tracks_xy, const int32_t* seen, int n_slots,
                     int window_len, double prob, double threshold, int max_iters, uint64_t seed, double* E, double* R,
                     double* t, int32_t* inliers, int32_t* good, int32_t* iters, int32_t* counts, double* scale,
                     int32_t* triplets, int32_t* ratios_used);

/* ---- next row: masked Shi-Tomasi detection that tops up tracked points ----
 * Replaces, for a tracker whose windows chain on the device,
 *   the fresh cv::goodFeaturesToTrack that is the BA flavour's only source of points when it has no observations
 *                                                                          src/with_bundle_adjustment.cpp:586-593
 *   the re-detection the streaming flavour falls back to when fewer than 150 tracks survive (there: ORB plus the
 *   matcher, which stays out)                                              src/feature_tracking.cpp:68-71
 * with what KLT front-ends call goodFeaturesToTrack(img, n_max - n_alive, q, d, mask): the live tracks are carried,
 * new corners are appended, and no new corner is closer than min_distance to a carried point.  Rules (DESIGN.md §9
 * rank 12, A-F; tests/gftt_topup_ref.py restates them, results are bit-identical):
 *   seeds    slot s of frame f is live iff d_seed_seen == NULL or d_seed_seen[f][s] >= seen_min, and usable iff both
 *            floats are finite, 0 <= x <= width - 1 and 0 <= y <= height - 1 (float compares); others are dropped
 *   carry    the usable seeds of a frame, float bits unchanged, in ascending slot order, at most max_corners of them:
 *            carried[f] points at the front of the frame's output, origin = their seed slot
 *   blocked  (min_distance >= 1) an integer pixel (X, Y) with fadd(fmul(dx, dx), fmul(dy, dy)) < (float)(d * d) for
 *            some carried seed, dx = (float)X - sx, dy = (float)Y - sy; for the mask entry: a mask byte of 0
 *   detect   rules 1-6 of rank 8 with the maximum of rule 2 taken over the pixels that are not blocked (OpenCV's
 *            minMaxLoc with a mask) and blocked pixels no candidates (their values still count in a neighbour's 3x3
 *            maximum); at most max_corners - carried[f] new corners follow the carried points, origin -1
 * counts[f] = carried[f] + new corners; slots at or beyond counts[f] are 0 with origin -1: whole arrays compare equal.
 * min_distance above ORBX_GFTT_TOPUP_MAX_MIN_DISTANCE is ORBX_ERR_UNSUPPORTED (the work per seed is (2R + 2)^2 pixels,
 * R = ceil(min_distance)). */
#define ORBX_GFTT_TOPUP_MAX_MIN_DISTANCE 64.0
/* The top-up of `n` frames in device memory (src/with_bundle_adjustment.cpp:586-593, src/feature_tracking.cpp:68-71),
 * asynchronously on the context's stream (or `stream`).  Frame, stride, alignment and stream rules are those of
 * orbx_good_features_batch_device; quality_level and min_distance are checked as there, plus the bound above.
 * max_corners >= 1, seed_capacity >= 1; d_seed_xy is 4-byte aligned, slot s of frame f at
 * d_seed_xy + f * seed_frame_stride + s * seed_point_stride (strides in floats; seed_point_stride >= 2,
 * seed_frame_stride >= (seed_capacity - 1) * seed_point_stride + 2); d_seed_seen is [n][seed_capacity] or NULL.  A
 * d_seed_xy inside the top-up's own result block is ORBX_ERR_INVALID_ARG.  On any error nothing is written, the
 * previous top-up result stays fetchable and the context usable.
 * With the view of orbx_lk_windows_results_device: d_seed_xy = tracks_xy + 2 * (window_len - 1), seed_point_stride =
 * 2 * window_len, seed_frame_stride = 2 * window_len * slot_capacity, d_seed_seen = seen, seen_min = window_len, and
 * d_frames / frame_stride picking each window's last frame; points_xy and counts of the result go into the next
 * orbx_lk_track_windows_device, origin joins its slots to the previous window's.  The plain good-features view is
 * an equally valid seed source.
 * The results go to a block of their OWN (slot_capacity = max_corners): the ORB batch, the plain good-features
 * block, the LK windows block and orbx_lk_track's state stay as they are.  Workspace: the good-features workspace
 * (its size and the slicing of the plain entries unchanged) plus one bit per pixel -- 4 * ceil(width / 32) * height
 * bytes per frame of a slice --, allocated beside it for the same number of frames at the first top-up or masked call
 * and freed with it; results do not depend on the slicing. */
int orbx_good_features_topup_device(orbx_ctx* ctx, const void* d_frames, int n, int width, int height, int row_stride,
                                    size_t frame_stride, const float* d_seed_xy, size_t seed_point_stride,
                                    size_t seed_frame_stride, const int32_t* d_seed_seen, int seen_min,
                                    int seed_capacity, int max_corners, double quality_level, double min_distance,
                                    void* stream);
/* Device-side view of the last top-up's results (src/with_bundle_adjustment.cpp:586-593), valid until the next
 * top-up or masked call; written on that call's stream. */
typedef struct {
  const int32_t* counts;   /* [n] */
  const int32_t* carried;  /* [n] */
  const float* points_xy;  /* [n][slot_capacity][2] */
  const int32_t* origin;   /* [n][slot_capacity] */
  int32_t slot_capacity;
  int32_t n;
} orbx_good_features_topup_view;
/* Fills the view; ORBX_ERR_INVALID_ARG before any top-up.  src/with_bundle_adjustment.cpp:586-593 */
int orbx_good_features_topup_results_device(orbx_ctx* ctx, orbx_good_features_topup_view* view);
/* Waits for the last top-up and copies frames [first, first + n): counts and carried (n entries), points_xy
 * (n x slot_capacity x 2 floats) and origin (n x slot_capacity); all but counts may be NULL.
 * src/with_bundle_adjustment.cpp:586-593 */
int orbx_good_features_topup_fetch(orbx_ctx* ctx, int first, int n, int32_t* counts, int32_t* carried,
                                   float* points_xy, int32_t* origin);
/* The top-up of one host image from n_seeds host points (n_seeds >= 0; every seed is live), synchronous
 * (src/feature_tracking.cpp:68-71).  *count = carried + new points, *carried = points carried; if *count exceeds
 * `capacity`, ORBX_ERR_CAPACITY is returned, *count is the capacity required and nothing else is written.  Runs as
 * a top-up of one frame: it replaces the results of the last top-up. */
int orbx_good_features_topup(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                             const float* seeds_xy, int n_seeds, int max_corners, double quality_level,
                             double min_distance, float* points_xy, int32_t* origin, int capacity, int* count,
                             int* carried);
/* cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance, mask) on one host image
 * (src/with_bundle_adjustment.cpp:586-593 with the argument the reference leaves empty): a pixel whose mask byte is 0
 * is no corner and does not count for the maximum that qualityLevel scales; mask_stride >= width.  max_corners <= 0:
 * no limit.  *count and ORBX_ERR_CAPACITY as orbx_good_features_to_track.  Runs as a top-up of one frame without
 * seeds: it replaces the results of the last top-up, and leaves the plain good-features block alone. */
int orbx_good_features_to_track_masked(orbx_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                                       const uint8_t* mask, int mask_stride, int max_corners, double quality_level,
                                       double min_distance, float* corners_xy, int capacity, int* count);

/* ---- next row: the forward-backward check of Lucas-Kanade over frame windows ------------
 * What every KLT front end built on cv::calcOpticalFlowPyrLK puts behind the tracker, and the reference's
 * trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499) and track_optical_flow
 * (src/feature_tracking.cpp:166-193) leave out: a point that slid along an edge or jumped to a look-alike patch keeps
 * status 1.  Here every pair of a window is tracked twice in the one tracking launch, with the arithmetic of
 * orbx_lk_track both times.  For the slot's point p entering pair k (frames window_first[w] + k - 1 and + k):
 *   1. forward   (q, status, e) = the pair as orbx_lk_track_windows_device tracks it; status 0 ends the track, reason 1
 *   2. backward  (r, status) = q tracked from frame k back into frame k - 1, starting at q itself (no initial flow),
 *                same parameters; status 0 ends the track, reason 2
 *   3. distance  dx = r.x - p.x, dy = r.y - p.y in float; d2 = (double)dx * dx + (double)dy * dy, the products exact,
 *                the sum rounded once; the pair passes iff d2 <= (double)fb_threshold * (double)fb_threshold.  A NaN
 *                d2 fails.  Failing ends the track, reason 3
 *   4. on a pass tracks[k] = q, err[k - 1] = e, fb_d2[k - 1] = (float)d2, and q enters pair k + 1 with the same bits
 * tracks_xy, seen and err go into the block of orbx_lk_track_windows_device in its layout: after this call
 * orbx_lk_windows_results_device and orbx_lk_windows_fetch return them, and the landmarks build, the tracks pose and
 * the top-up read the view as they read any other.  Beside them, in a buffer of their own:
 *   fb_d2[w][slot][k - 1]  the squared distance of every pair that passed (the first seen - 1 entries), 0 elsewhere
 *   lost[w][slot]          0 for a track alive through the window and for the slots at or beyond counts[w], else the
 *                          reason the track ended, 1 / 2 / 3
 * fb_threshold: NaN or < 0 is ORBX_ERR_INVALID_ARG (nothing is written, the previous result stays fetchable); 0 (only
 * points that return exactly) and +inf (only the two status tests) are legal.  Every other argument rule, the slices
 * under the workspace limit, the stream ordering and the workspace are those of orbx_lk_track_windows_device: the
 * backward pass reads the pyramids and derivative maps that call builds for every frame of a slice anyway. */
int orbx_lk_track_windows_fb_device(orbx_ctx* ctx, const void* d_frames, int n_frames, int width, int height,
                                    int row_stride, size_t frame_stride,
                                    const int32_t* window_first /* host, [n_windows] */, int n_windows, int window_len,
                                    const float* d_points_xy /* device, [n_windows][slot_capacity][2] */,
                                    const int32_t* d_counts /* device, [n_windows]; NULL: every slot is a point */,
                                    int slot_capacity, int win_size, int max_level, int max_iters, double epsilon,
                                    float fb_threshold, void* stream);
/* Device-side view of what the check added to the last windows call (valid until the next one; written on its
 * stream).  src/with_bundle_adjustment.cpp:464-499 */
typedef struct {
  const float* fb_d2;  /* [n_windows][slot_capacity][window_len - 1] */
  const int32_t* lost; /* [n_windows][slot_capacity] */
  int32_t slot_capacity, window_len, n_windows;
} orbx_lk_windows_fb_view;
/* Fills the view; ORBX_ERR_INVALID_ARG when the last windows call had no forward-backward check (or none has run).
 * src/with_bundle_adjustment.cpp:464-499 */
int orbx_lk_windows_fb_results_device(orbx_ctx* ctx, orbx_lk_windows_fb_view* view);
/* Waits for the last windows call and copies windows [first, first + n) in the view's layout; each of the two arrays
 * may be NULL.  ORBX_ERR_INVALID_ARG as above.  src/with_bundle_adjustment.cpp:464-499 */
int orbx_lk_windows_fb_fetch(orbx_ctx* ctx, int first, int n, float* fb_d2, int32_t* lost);
/* Host convenience, the twin of orbx_lk_track_window: ONE window of n_frames host frames and n host points in; beside
 * tracks_xy, seen and err (may be NULL), fb_d2 (n x (n_frames - 1)) and lost (n) out, both may be NULL.  Synchronous;
 * runs as a windows batch of one window with the check and replaces the last windows result.  n == 0: nothing is done.
 * src/with_bundle_adjustment.cpp:464-499, src/feature_tracking.cpp:166-193 */
int orbx_lk_track_window_fb(orbx_ctx* ctx, const uint8_t* frames, int n_frames, int width, int height, int row_stride,
                            size_t frame_stride, const float* pts_xy, int n, float* tracks_xy, int32_t* seen,
                            float* err, int win_size, int max_level, int max_iters, double epsilon, float fb_threshold,
                            float* fb_d2, int32_t* lost);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
