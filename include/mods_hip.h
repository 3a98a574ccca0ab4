/*
 * mods_hip.h — C ABI of libmodsgpu.so, the MI355X (gfx950) implementation of the
 * detect -> describe -> match -> verify hot path of MODS (ducha-aiki/mods-light-zmq).
 *
 * Plain pointers and sizes only.  Every entry point names the reference interface it
 * replaces (file:line relative to the reference root); INTEGRATION.md shows the binding a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - images: row-major fp32, single channel, `stride` in elements (the reference passes
 *     contiguous CV_32FC1 cv::Mat, imagerepresentation.cpp:293-302).
 *   - all functions return 0 on success, a negative MODS_E_* code otherwise; nothing is
 *     computed on the CPU when the GPU is missing (MODS_E_NODEVICE).
 *   - `*_dev` variants take device pointers (HBM resident inputs/outputs); the others take
 *     host pointers and stage through the context's pinned buffers.
 */
#ifndef MODS_HIP_H
#define MODS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MODS_OK 0
#define MODS_E_NODEVICE (-1)   /* no HIP device / extension unusable: never falls back to CPU */
#define MODS_E_ARG (-2)
#define MODS_E_CAPACITY (-3)   /* an output or internal list overflowed its capacity */
#define MODS_E_HIP (-4)        /* a HIP runtime call failed; see mods_last_error() */

typedef struct mods_ctx mods_ctx;

/* [HessianAffine] keys of the .ini (io_mods.cpp:167-207) = PyramidParams + AffineShapeParams
 * (detectors/structures.hpp:114-150, detectors/affinedetectors/affine.h:26-68). */
typedef struct mods_hessaff_params {
  int numberOfScales;          /* 3 */
  float initialSigma;          /* 1.6 */
  float threshold;             /* 5.33 */
  float edgeEigenValueRatio;   /* 10; PyramidParams keeps a double: a value no float holds (7.3) reaches the edge test as (double)(float)7.3 */
  int border;                  /* 5 */
  int maxIterations;           /* max_iter = 16 */
  float convergenceThreshold;  /* 0.05 */
  int smmWindowSize;           /* 19 */
  int doBaumberg;              /* 1 */
  /* keypoint selection, AffineDetector::prepareKeysForExport (scale-space-detector.hpp:126-198); in every mode but FixedTh the
   * detector's thresholds are 0 (pyramid.h:58-59): every 3x3x3 extremum is localised and adapted, then the sorted list is cut */
  int mode;                    /* [HessianAffine] mode: MODS_DET_* (FixedTh) */
  float relativeThreshold;     /* RelativeTh: keep |response| > relativeThreshold * max|response| */
  int regionsNumber;           /* FixedRegNumber: the strongest regionsNumber; NotLessThanRegions: at least that many */
  float relativeRegionsNumber; /* RelativeRegNumber: the strongest floor(relativeRegionsNumber * n) */
  /* which response the scale space is searched in: the [HessianAffine] / [DoG] / [HarrisAffine] sections of the .ini fill the
   * same parameter set and differ in DetectorType (io_mods.cpp:167-169, 208-210, 260-262).  ScaleSpaceDetector::Response,
   * pyramid.cpp:126-163; final threshold = threshold^2 for Hessian, threshold otherwise (pyramid.h:55-56); point types
   * pyramid.cpp:65-124 */
  int detectorType;            /* MODS_DET_HESSIAN */
  int iiDoGMode;               /* DoG only: illumination-invariant rescale of the response (pyramid.cpp:172-194) */
  int sampleFromImage;         /* AffineShapeParams::sampleFromImage (affine.h:47, io_mods.cpp:184): findAffineShape samples the input
                                * image at pixel distance 1 instead of the blur level below the detection level
                                * (scale-space-detector.hpp:47-55); dense (stride == w) input only */
  /* detectorType = MODS_DET_MSER: the [MSER] section (io_mods.cpp:101-123) = extrema::ExtremaParams
   * (detectors/mser/extrema/extremaParams.h:56-89); mode, relativeThreshold, regionsNumber, relativeRegionsNumber above are
   * shared (regionsNumber of a view is scaled by 2 * zoom / tilt, extrema.cpp:201-202), everything else above is unused.
   * Replaces DetectMSERs (detectors/mser/extrema/extrema.cpp:196-295) behind DetectAffineRegions<> (imagerepresentation.cpp:780-783):
   * MSER+ regions first (sub_type 21), then MSER- (20), response = the stability margin; in every mode but FixedTh the margin
   * bound is 1 and the list is sorted by margin and cut (prepareKeysForExport, extrema.cpp:31-90). */
  double mserMaxArea;          /* max_area = 0.01 (0.05 in config_affori_classic.ini): largest region as a fraction of the image */
  double mserMinMargin;        /* min_margin = 10 (8 in the shipped .ini): the stability bound of FixedTh */
  int mserMinSize;             /* min_size = 30 pixels */
  int affBmbrgMethod;          /* [HessianAffine] affBmbrgMethod (io_mods.cpp:193; AffineBaumbergMethod, affine.h:21-24): 0 = second moment
                                * matrix, 1 = the Hessian form of the iteration (affine.cpp:92-128: 3x3 samples at s * 0.5, SVD of the
                                * Hessian); HessianAffine / DoG / HarrisAffine */
} mods_hessaff_params;
enum { MODS_DET_FIXED_TH = 0, MODS_DET_RELATIVE_TH, MODS_DET_FIXED_REG_NUMBER, MODS_DET_RELATIVE_REG_NUMBER,
       MODS_DET_NOT_LESS_THAN_REGIONS };   /* detection_mode_t, detectors/structures.hpp:10-14 */
enum { MODS_DET_HESSIAN = 0, MODS_DET_DOG = 1, MODS_DET_HARRIS = 2, MODS_DET_MSER = 3 };   /* detector_type, detectors/structures.hpp:16-19 */

/* AffineKeypoint (detectors/structures.hpp:185-195) + provenance of the pyramid hit. */
typedef struct mods_affkey {
  double x, y, s, a11, a12, a21, a22, response;
  int sub_type;                /* Hessian: 0 dark, 1 bright, 2 saddle; DoG: 10 dark, 11 bright; Harris: 30 dark, 31 bright (pyramid.h:33-40);
                                * MSER: 21 MSER+, 20 MSER- (extrema.cpp:261, 286) */
  int octave, level, r0, c0;   /* NMS cell that produced the point (MSER: threshold, polarity, seed row, seed column) */
  int pad;
} mods_affkey;

/* pyramid localisation result before affine adaptation (pyramid.cpp:281-403) */
typedef struct mods_candidate {
  int octave, level, r0, c0, r, c;
  float x, y, s, pixelDistance, response;
  int type;
} mods_candidate;

/* AffineRegion subset that travels through orientation/description/matching
 * (detectors/structures.hpp:214-229): det_kp == reproj_kp for the identity view. */
typedef struct mods_region {
  double x, y, s, a11, a12, a21, a22, response;
  int sub_type;
  int id, parent;
  int pad;
  uint8_t desc[128];           /* RootSIFT, integer valued 0..255 (siftdesc.cpp:199-222) */
} mods_region;

/* TentativeCorrespExt subset (matching/matching.hpp:39-51) */
typedef struct mods_tentative {
  int q, t;                    /* first / second: indices into the query and train lists */
  int t_bad, t_2nd;            /* secondbad / secondbadby2ndcl */
  float d1, d2, d2nd;          /* squared L2 distances */
  float pad;
  double ratio;                /* sqrt(d1/d2) */
} mods_tentative;

/* ---- context ------------------------------------------------------------------------ */
const char *mods_last_error(void);
int mods_device_count(void);
/* One context = one GPU, one stream set, one pool of HBM scratch sized for images up to
 * max_w x max_h and `batch` images per call. */
int mods_ctx_create(int device, int max_w, int max_h, int batch, mods_ctx **out);
/* flags bit 0: non-blocking stream (no implicit ordering after the default stream: inputs must be complete
 * when a call is made); lets several contexts overlap on one GPU */
int mods_ctx_create_ex(int device, int max_w, int max_h, int batch, int flags, mods_ctx **out);
void mods_ctx_destroy(mods_ctx *ctx);
int mods_ctx_sync(mods_ctx *ctx);
void *mods_ctx_stream(mods_ctx *ctx);            /* hipStream_t the kernels run on */

/* per-kernel HIP-event timing (bench.py roofline leg).  When enabled every launch of the
 * named stage is bracketed by events on the context's stream. */
enum { MODS_STAGE_BLUR = 0, MODS_STAGE_RESPONSE, MODS_STAGE_RESIZE, MODS_STAGE_NMS, MODS_STAGE_LOCALIZE,
       MODS_STAGE_BAUMBERG, MODS_STAGE_SORT, MODS_STAGE_ORIENT, MODS_STAGE_DESCRIBE, MODS_STAGE_MATCH,
       MODS_STAGE_RANSAC_SCORE, MODS_STAGE_SYNTH,
       MODS_STAGE_BLUR_SMALL,   /* blur launches of the small planes (the 16-row tile instantiation); MODS_STAGE_BLUR: 32-row tiles */
       MODS_STAGE_PYRAMID,      /* the whole scale space of a batch in ONE scope on the context's stream: every blur, response and
                                 * resize launch of every octave + NMS + compaction (the small octaves run on a second stream
                                 * inside it, so the per-stage sums above overlap and add up to more than this) */
       MODS_STAGE_MATCH_NN1,    /* the matrix-core kernel of the search alone (match_nn1_kernel, i8 MFMA), inside MODS_STAGE_MATCH */
       MODS_STAGE_EXTRACT,      /* measurement-region extraction alone (classify .. column pass + resampling), inside MODS_STAGE_DESCRIBE */
       MODS_STAGE_SIFT,         /* the SIFT kernels alone, inside MODS_STAGE_DESCRIBE */
       MODS_STAGE_GUIDED,       /* a guided search (mods_match_guided[_reps]): pack, both gate sweeps, accept, compaction and emit */
       MODS_STAGE_MATCH_MUTUAL, /* the mutual check of a search alone (mods_ctx_match_mutual: list + sweep), inside MODS_STAGE_MATCH */
       MODS_STAGE_OVERLAP,      /* an overlap search (mods_match_overlap[_reps]): pack, the sweep, accept, compaction and emit */
       MODS_STAGE_OVERLAP_AREA, /* an area-overlap search (mods_match_overlap_area[_reps]): pack, both gate sweeps, the lattice walk,
                                 * accept, compaction and emit - in two scopes, the host reads the length of the pair list between them */
       MODS_STAGE_LOCAL_AFFINE, /* the local affine consistency filter (mods_filter_local_affine, mods_ctx_local_affine): prep, both sweeps,
                                   keep and compaction */
       MODS_STAGE_REPROJECT_H,  /* the post-pass of a homography view (reproject_regions_h_kernel): reprojection, tests and compaction */
       MODS_STAGE_SPATIAL_SELECT, /* the spatial selection of a count mode's cut (mods_ctx_spatial_selection): radius, ranking and
                                     compaction, behind MODS_STAGE_SORT and outside it */
       MODS_STAGE_KNN,          /* a k-nearest-neighbour search (mods_match_knn[_dev|_reps]): pack, sweep and merge */
       MODS_STAGE_KNN_SWEEP,    /* the matrix-core kernel of that search alone (knn_sweep_kernel, i8 MFMA), inside MODS_STAGE_KNN */
       MODS_STAGE_DISTRACTOR,   /* the distractor-database veto of a search (mods_ctx_distractor_db): gather, sweep, fold and the ratio pass */
       MODS_STAGE_DISTRACTOR_SWEEP, /* the matrix-core kernel of that veto alone (descdb_sweep_kernel, i8 MFMA), inside MODS_STAGE_DISTRACTOR */
       MODS_STAGE_REFINE,       /* the least-squares refinement of a correspondence list (mods_refine_matches[_dev]): its one kernel */
       MODS_STAGE_PROPAGATE,    /* a match propagation (mods_propagate_matches[_dev]): every launch of the call - the LSM launches of the
                                   seeds and of each round, mark, propose, list and gate-and-append */
       MODS_STAGE_COUNT };
int mods_ctx_timing_enable(mods_ctx *ctx, int stage_mask);
/* on != 0: mods_detect_describe_dev (and what is built on it: the pair entry points, the pipeline's workers) records the ~70
   launches of a call into a hipGraph the second time it sees the same arguments (image pointer, sizes, parameters) and replays
   it from then on - one submission and one completion for the host instead of one per launch.  The results are the same
   launches' results.  Only calls whose scale space forks onto the context's side stream (images x batch of 4 megapixels or more,
   pyramid streams = 2) are recorded; others stay eager (a linear recording faults on replay with the ROCm 7.0.2 runtime unless
   DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 is set before the runtime starts; csrc/capi.hip: dd_run).  Off by default for a context.
   The pair pipeline used it for its workers' contexts during round 5 and does so only with MODS_PIPELINE_STREAMS=2 now: with this
   runtime a graph launch with branches - like the side stream itself - keeps the HIP runtime's own thread spinning for its
   duration (tools/ubench/rt_thread_probe.hip), a core per process that the pipeline's one-stream workers do not cost.
   mods_ctx_graph_replays: calls served by a replay so far. */
int mods_ctx_graphs(mods_ctx *ctx, int on);
long mods_ctx_graph_replays(const mods_ctx *ctx);
/* detect + describe calls of the context so far whose orientation and description had the batch's 8-bit images to sample from
   (mods_detect_describe_dev_u8 with packed rows; mods_orient_describe_u8; the pair pipeline's batches of 8-bit pairs, warm-up
   included) */
long mods_ctx_u8_source_calls(const mods_ctx *ctx);
/* which kernels sample from the 8-bit images in such calls: bit 0 orient_kernel, 1 extract_small_kernel, 2 big_fused_kernel,
   3 big_sample_kernel; bits 4 - 7: the same four sample from the library's own copy of those images in 16-byte column strips, which
   the conversion launch of the call then makes (it goes before bits 0 - 3); mask < 0 (the default): the library's measured choice
   (orient, extract_small and big_fused from the strips, big_sample from fp32).  Every choice gives the same regions; the tests use
   it to run the forms the default leaves out. */
int mods_ctx_u8_kernels(mods_ctx *ctx, int mask);
/* The strip layout, for the tests.  _layout: the layout's width limit and, for a w x h image, strips per image, bytes per strip
   and bytes per image (no device needed); _strip_of: the strip of the columns 0 .. n - 1; _offsets: the byte offset of every
   pixel pair's first pixel, out[h - 1][w - 1]; _fetch: the strip copy of a packed 8-bit host batch as the library makes it on
   the device, the batch staged src_offset (0 .. 15) bytes into the staging area. */
long mods_ctx_u8_strip_calls(const mods_ctx *ctx);          /* calls so far that had the strip copy as well */
int mods_u8_strips_layout(int w, int h, unsigned *max_width, unsigned *n_strips, unsigned *pitch, size_t *image_bytes);
void mods_u8_strips_strip_of(unsigned n, unsigned *out);
int mods_u8_strips_offsets(int w, int h, unsigned *out);
int mods_u8_strips_fetch(mods_ctx *ctx, const unsigned char *img_u8_host, int n_img, int w, int h, int src_offset, unsigned char *out);
/* Streams the Hessian scale space of a large batch is built on: 2 (default) = the octaves from the third on, and their non-maximum
   suppression, run on a side stream next to the large octaves' last level and NMS; 1 = everything on the context's stream (what
   per-launch timing wants).  The planes and the candidates are the same either way. */
int mods_ctx_pyramid_streams(mods_ctx *ctx, int n);
/* sums since the last reset; resolves pending events (synchronises the stream) */
int mods_ctx_timing_read(mods_ctx *ctx, int stage, double *total_ms, int *launches, double *bytes);
int mods_ctx_timing_reset(mods_ctx *ctx);

/* ---- B2: detector --------------------------------------------------------------------
 * Replaces  int DetectAffineKeypoints(cv::Mat &input, vector<AffineKeypoint> &out,
 *           ScaleSpaceDetectorParams, ScalePyramid&, double tilt, double zoom)
 * (detectors/affinedetectors/scale-space-detector.cpp:13-32) followed by the
 * s*=sqrt|det A| / rectifyTransformation loop of DetectAffineRegions<>
 * (synth-detection.hpp:79-112).  Output sorted by |response| descending, cut as par->mode says. */
int mods_detect_hessian_affine(mods_ctx *ctx, const float *img, int w, int h, int stride,
                               const mods_hessaff_params *par, mods_affkey *out, int max_out, int *n_out);
/* batch of `n_img` same-size device-resident images; out[i*max_out ...], n_out[i] */
int mods_detect_hessian_affine_dev(mods_ctx *ctx, const float *img_dev, int n_img, int w, int h, int stride,
                                   const mods_hessaff_params *par, mods_affkey *out_host, int max_out,
                                   int *n_out_host);

/* Introspection used by the parity tests (no reference counterpart): planes of the last
 * pyramid built by the context. kind 0 = blur, 1 = response. */
int mods_pyramid_octaves(mods_ctx *ctx);
int mods_pyramid_dims(mods_ctx *ctx, int octave, int *w, int *h);
int mods_pyramid_plane(mods_ctx *ctx, int img, int octave, int level, int kind, float *dst_host);
int mods_pyramid_candidates(mods_ctx *ctx, int img, mods_candidate *out, int max_out, int *n_out);
/* raw 3x3x3 NMS hits of the last detection, before localisation, in list (arbitrary) order: out4[4*i ..] = (octave, level, r0, c0)
 * of the first min(count, capacity of the context's hit list) records; *n_out = the device's count, which exceeds that capacity
 * after a detection that ended in MODS_E_CAPACITY "NMS hit list overflow".  MODS_E_CAPACITY here: max_out too small. */
int mods_pyramid_nms_hits(mods_ctx *ctx, int img, int *out4, int max_out, int *n_out);

/* single primitives (parity tests / building blocks; references: helpers.cpp:717-731,
 * pyramid.cpp:196-254, pyramid.cpp:476, helpers.cpp:551-626) */
int mods_gauss_blur(mods_ctx *ctx, const float *src, int w, int h, float sigma, float *dst);
int mods_hessian_response(mods_ctx *ctx, const float *src, int w, int h, float norm, float *dst);
int mods_resize_half(mods_ctx *ctx, const float *src, int w, int h, float *dst, int *dw, int *dh);

/* ---- a doubled first octave (PyramidParams::upscaleInputImage, structures.hpp:116-117; pyramid.cpp:504-509) -----------------
 * Lowe's "octave -1" for HessianAffine, DoG and HarrisAffine: the scale space starts at the doubled image, at pixel distance 0.5,
 * and the input is assumed to carry a blur of 1.0 instead of 0.5.  The reference's doubleImage (helpers.cpp:733-765) cannot be a
 * contract - it indexes with the byte step as an element offset, skips no column at a row's end, leaves the last row and column
 * unwritten, and no .ini key ever sets the switch - so the contract is this library's own (that function's evident intent),
 * restated in tests/upscale_ref.py and held to the bit; parity with the reference is unpinned.
 *
 * double_image(I), I of h x w fp32, is D of 2h x 2w.  With r' = min(r + 1, h - 1), c' = min(c + 1, w - 1), a = I[r, c],
 * b = I[r, c'], c_ = I[r', c], d = I[r', c'], every operation in fp32 with one rounding and in this order:
 *     D[2r,     2c    ] = a                      D[2r,     2c + 1] = 0.5f * (a + b)
 *     D[2r + 1, 2c    ] = 0.5f * (a + c_)        D[2r + 1, 2c + 1] = 0.25f * (((a + b) + c_) + d)
 *
 * With the switch on, octave 0 is D (2w x 2h, pixelDistance 0.5; mods_pyramid_dims(ctx, 0) reports it) and the later octaves
 * follow from it by the usual rule, so octave 1 has the input's size but is decimated from level numberOfScales of octave 0.  The
 * initial blur runs only if initialSigma > 1.0, with sigma = sqrtf(initialSigma^2 - 1.0f); otherwise level 0 is D itself.  Level
 * sigmas and everything behind the planes are unchanged: keys and regions are in image coordinates, mods_affkey.octave counts
 * from the doubled octave, sampleFromImage still samples the input image at pixel distance 1.  A call whose doubled image would
 * have 2^25 pixels or more (4 w h >= 2^25) is MODS_E_ARG, before anything is allocated.  MSER ignores the switch; mods_multi has
 * none.  A context that never turns it on allocates nothing for it.
 *
 * mode: 0 off (default), 1 on, 2 on with the first level made in two launches (double, then blur: what mode 1's single launch,
 * which doubles in the blur's window loader, is tested against; the planes of the two are equal to the bit).  Changing the mode
 * is a change of device state: no recorded launch chain (mods_ctx_graphs) is replayed across it.  The view workers of a step
 * loop take their owner's mode.  mods_pipeline_upscale_input: every worker's context, before the first submit (later: MODS_E_ARG).
 * mods_upscale2x: double_image of one host image, dst holds 2w x 2h floats. */
int mods_ctx_upscale_input(mods_ctx *ctx, int mode);
int mods_ctx_upscale_input_get(const mods_ctx *ctx, int *mode);
int mods_upscale2x(mods_ctx *ctx, const float *src, int w, int h, float *dst);

/* ---- B3: orientation + description ---------------------------------------------------------
 * [DominantOrientation] and [SIFTDescriptor] keys (io_mods.cpp:731-740, 423-436). */
typedef struct mods_describe_params {
  double ori_mrSize;       /* 5.1962 */
  int ori_patchSize;       /* 32 */
  int ori_maxAngles;       /* 1; > 1: an oriented copy per histogram peak above the threshold, the first maxAngles in bin order
                              (synth-detection.cpp:900-927, 1095-1106); <= 0: no oriented copies (`if (maxAngNum > 0)`, :1086) */
  double ori_threshold;    /* (double)(float)0.8 */
  double desc_mrSize;      /* 5.1962 */
  int desc_patchSize;      /* 41 */
  int photoNorm;           /* 1 */
  int rootSift;            /* 1 = RootSIFT, 0 = SIFT */
  double maxBinValue;      /* 0.2 */
  /* Half descriptors (imagerepresentation.cpp:725-731, 909-943, 970-979; siftdesc.cpp:401-436).  As soon as a step's
   * descriptor list names a "Half*" descriptor the reference estimates the dominant orientation in doHalfSIFT mode
   * (orientation modulo pi: histogram bins i and i + 18 folded after the threshold is taken) for EVERY descriptor of the view. */
  int ori_halfMode;        /* 0 */
  int addUpRight;          /* [DominantOrientation] addUpRight (imagerepresentation.cpp:915-930): the unrotated copy of every region
                              that passes DetectOrientation's border test is described too; those copies come first in the list */
  int halfDesc;            /* 1: also HalfRootSIFT (64 values: orientation bins j and j + 4 of the raw histogram added, then the
                              RootSIFT normalisation) for the same regions, see mods_regions_half_dev */
  int fastExtraction;      /* [SIFTDescriptor] FastPatchExtraction: the fast branch of DescribeRegions (synth-detection.hpp:232-253): one
                              interpolate() of the image at imageToPatchScale = (2*int(mrSize*s)+1)/patchSize (double), no smoothing */
} mods_describe_params;

/* Replaces, for one identity view (H = I), the chain of imagerepresentation.cpp:867-968:
 *   ReprojectRegionsAndRemoveTouchBoundary(dontRemove)  synth-detection.cpp:151-190
 *   DetectOrientation(...)                               synth-detection.cpp:1039-1149
 *   ReprojectRegions(...)                                synth-detection.cpp:631-706
 *   DescribeRegions<SIFTDescriptor>(...)                 synth-detection.hpp:170-263, matching/siftdesc.cpp
 * Input: keypoints as produced by mods_detect_hessian_affine; output: oriented, described
 * regions in input order (dropped ones removed). */
int mods_orient_describe(mods_ctx *ctx, const float *img, int w, int h, int stride, const mods_affkey *keys,
                         int n_keys, const mods_describe_params *par, mods_region *out, int max_out, int *n_out);

/* the same for an 8-bit grey host image (`stride` in bytes): converted exactly to fp32 inside the context, while orientation and
 * description sample the 8-bit image itself in the kernels mods_ctx_u8_kernels selects - the same regions to the bit.  Counts in
 * mods_ctx_u8_source_calls.  MODS_E_ARG, before any device call: a null pointer, stride < w, an image larger than the context,
 * more keypoints than the context's candidate capacity (for which mods_orient_describe, the fp32 twin, answers MODS_E_CAPACITY
 * after it has selected the device: here every refusal is an argument error and comes first). */
int mods_orient_describe_u8(mods_ctx *ctx, const unsigned char *img_u8, int w, int h, int stride, const mods_affkey *keys,
                            int n_keys, const mods_describe_params *par, mods_region *out, int max_out, int *n_out);

/* detect + orient + describe for a batch of device-resident images; regions stay in HBM for the
 * matcher (mods_regions_fetch copies them out).  n_regions_host[i] = regions of image i. */
int mods_detect_describe_dev(mods_ctx *ctx, const float *img_dev, int n_img, int w, int h, int stride,
                             const mods_hessaff_params *det, const mods_describe_params *desc,
                             int *n_detected_host, int *n_regions_host);
/* the same for a batch that is 8-bit grey in HBM ([n_img][h][stride] bytes, the form images have on disk): converted exactly to fp32
 * inside the context for the scale space and the detector, while orientation and description sample the 8-bit images themselves
 * (which kernels do: DESIGN.md section 4, "Sampling from the 8-bit twin") - the same regions to the bit.
 * img_u8_dev must stay unchanged until the call returns. */
int mods_detect_describe_dev_u8(mods_ctx *ctx, const unsigned char *img_u8_dev, int n_img, int w, int h, int stride,
                                const mods_hessaff_params *det, const mods_describe_params *desc,
                                int *n_detected_host, int *n_regions_host);
/* External descriptors (reference: the "ZMQ" descriptor, DescribeWithZmq, imagerepresentation.cpp:21-103, 992-1006).  While
 * a function is set, the describe stage extracts ExtractPatchesColumn's patches (patchSize x patchSize at mrSize, fp32, no
 * photometric normalisation) and hands them to it; the function returns 128 values per patch (0..255, integer valued, as
 * the HardNet daemon delivers them), which become the descriptor bytes.  libmodszmq.so provides mods_zmq_descriptor_hook
 * (user = endpoint string) with this signature. */
typedef int (*mods_descriptor_fn)(void *user, const float *patches, int n, int ps, float *out, size_t out_cap_floats, int *dim);
int mods_ctx_set_external_descriptor(mods_ctx *ctx, mods_descriptor_fn fn, void *user, double mrSize, int patchSize);
/* External affine shape and orientation (reference: [AffineAdaptation] useZMQ=1 with AffNet, [DominantOrientation] useZMQ=1 with
 * OriNet; imagerepresentation.cpp:786-856, 874-900).  While a shape function is set, the describe stage replaces the frame of
 * every detected keypoint (detect with doBaumberg = 0) by the function's (a11, a21, a22) for its ExtractPatchesColumn patch
 * (3 values per patch), rectified "up is up", and drops keypoints by the reference's eigenvalue-ratio and border tests.  While
 * an orientation function is set, the dominant-orientation estimate is replaced by atan2(y, x) of the function's 2 values per
 * patch.  Same callback type as the descriptor (libmodszmq's mods_zmq_descriptor_hook with the daemon's endpoint as user). */
int mods_ctx_set_external_shape(mods_ctx *ctx, mods_descriptor_fn fn, void *user, double mrSize, int patchSize);
int mods_ctx_set_external_orientation(mods_ctx *ctx, mods_descriptor_fn fn, void *user, double mrSize, int patchSize);
/* The same three networks in-process (nets.hip): AffNet, OriNet and HardNet as HIP kernels, fp32 with fp32 accumulation, inference
 * mode, on 32 x 32 patches.  A patch's output is a function of that patch and the weights only (not of the number of patches in
 * the call, their order or the chunking).  Outputs per patch are what the reference's daemons reply: AffNet (a11, a21, a22) with
 * +1 on the first and the last, OriNet (y, x), HardNet 128 values clip(210 * (d + 0.45), 0, 255) truncated to integers.
 * tensors, in network order: per block weight, running_mean, running_var; then the head's weight and bias (AffNet / OriNet) or
 * weight, running_mean, running_var (HardNet); n_floats[i] = elements of tensors[i] (checked against the architecture).
 * A mods_net is immutable after creation and may be used by several contexts and threads at once. */
typedef struct mods_net mods_net;
enum { MODS_NET_AFFNET = 0, MODS_NET_ORINET = 1, MODS_NET_HARDNET = 2 };
int  mods_net_create(int device, int kind, const float *const *tensors, const size_t *n_floats, int n_tensors, mods_net **out);
/* Precision of a network, chosen at creation.  MODS_NET_FP32 is the mode described above and what mods_net_create makes.
 * MODS_NET_BF16 ("bf16 mode") runs the bulk of the arithmetic on the matrix cores with bf16 operands; its outputs differ from the
 * fp32 mode's.  The arithmetic contract, with bf16(x) = the fp32 value x rounded to the nearest bf16, ties to even (inputs finite
 * and normal):
 *   - stage 0 (input normalisation) and stage 1 (conv 1 -> C, K = 9) compute what the fp32 mode computes, with the same arithmetic;
 *   - activations are stored as bf16 on leaving stages 1..6: bf16(relu(acc + bias)); stage 1's output is bf16(the fp32 mode's
 *     stage-1 output) to the bit;
 *   - the weights of stages 2..6 of all three networks and of HardNet's head are the fp32 mode's folded weights rounded once more:
 *     bf16((float)((double)W * inv)), inv = 1.0 / sqrt((double)var + 1e-5); the folded bias stays fp32.  Products are
 *     bf16 x bf16 (exact in fp32), accumulated in fp32 on the matrix cores; the bias is added in fp32 after the last k-step;
 *   - the order of every sum is fixed by the architecture and the kernel's tiling alone: a patch's output does not depend on the
 *     number of patches in the call, on their order or on the chunking;
 *   - the heads of AffNet and OriNet keep their fp32 weights and the fp32 mode's arithmetic on the bf16 activations widened to
 *     fp32 (exact); HardNet's tail behind the head GEMM is unchanged: + bias, L2 normalisation, trunc(clip(210 (y + 0.45))).
 * An unknown precision is MODS_E_ARG (checked with the other arguments, before the device is looked for).  Either kind of network
 * is immutable and shareable, and is taken by mods_net_forward[_dev] and mods_ctx_set_builtin_*. */
enum { MODS_NET_FP32 = 0, MODS_NET_BF16 = 1 };
int  mods_net_create_ex(int device, int kind, const float *const *tensors, const size_t *n_floats, int n_tensors, int precision, mods_net **out);
int  mods_net_precision(const mods_net *net);                 /* MODS_NET_FP32 or MODS_NET_BF16 */
void mods_net_destroy(mods_net *net);
int  mods_net_dim(const mods_net *net);                       /* 3, 2, 128 */
int  mods_net_chunk(void);                                    /* patches per set of launches (a call of more is cut into chunks) */
/* patches: [n][32][32] fp32 in 0..255.  quantise_u8 = 1 first rounds them as the wire to a daemon does (round half to even,
 * clamp to 0..255); 0 feeds the floats.  out: [n][dim].  The _dev form enqueues on hip_stream (a hipStream_t) and does not wait. */
int  mods_net_forward(mods_net *net, const float *patches_host, int n, int quantise_u8, float *out_host);
int  mods_net_forward_dev(mods_net *net, void *hip_stream, const float *patches_dev, int n, int quantise_u8, float *out_dev);
/* A built-in network in the slot of the external shape / orientation / descriptor function (NULL: off): the describe stage feeds
 * it the patch store in HBM, and only its values per patch go to the host, where the per-keypoint arithmetic of the callback
 * path runs unchanged.  Setting a network clears the slot's callback and the other way round; the kind must fit the slot. */
int  mods_ctx_set_builtin_shape(mods_ctx *ctx, mods_net *net, double mrSize, int quantise_u8);
int  mods_ctx_set_builtin_orientation(mods_ctx *ctx, mods_net *net, double mrSize, int quantise_u8);
int  mods_ctx_set_builtin_descriptor(mods_ctx *ctx, mods_net *net, double mrSize, int quantise_u8);
/* self-test hook: one stage of a network alone, host to host, through the launch functions mods_net_forward_dev uses.  stage 0 =
 * the input normalisation ([n][1024] -> [n][1024]; quantise_u8 as above, ignored by the other stages), 1..6 = the convolution
 * blocks ([n][cin][h][h] -> [n][cout][h / stride][h / stride]; channels C, C, 2C, 2C, 4C, 4C with C = 16 or 32 (HardNet), maps of
 * 32, 32, 16, 16, 8, 8 pixels a side at the output), 7 = the head ([n][4C * 64] -> [n][dim]).  1 <= n <= mods_net_chunk().  The
 * device output has one more patch's worth of elements behind it, filled with a sentinel before the launch; *guard_ok = 1 when
 * the stage left them alone.  On a bf16 network the shapes are the same: the host input of stages 2..7 is rounded to bf16 on its way
 * in, the output of stages 1..6 (bf16 on the device, with a bf16 guard) comes back widened to fp32. */
int  mods_test_net_stage(mods_net *net, int stage, const float *in_host, int n, int quantise_u8, float *out_host, int *guard_ok);
/* timing hook: mods_net_forward_dev with a device event in front of every launch; waits for the stream, then stage_ms[0..7] = the
 * time between the events around stage 0..7, summed over the chunks of the call (tools/bench_nets_bf16.py).  It creates, records
 * and destroys 8 events per chunk and one more, and synchronises the stream: not for a stream that is being captured into a graph. */
int  mods_test_net_stage_times(mods_net *net, void *hip_stream, const float *patches_dev, int n, int quantise_u8, float *out_dev, float *stage_ms);
int mods_patches_fetch(mods_ctx *ctx, int img, int ps, float *out, int max_regions, int *n_out);   /* patches of the last describe call */
/* Baumberg work counters of image slot img (bench.py's per-keypoint figures): keypoints that entered the affine-shape iteration and
 * iterations run since mods_baumberg_stats_enable(ctx, 1); one iteration = smmWindowSize^2 bilinear taps (affine.cpp:26-158). */
int mods_baumberg_stats_enable(mods_ctx *ctx, int on);
int mods_baumberg_stats(mods_ctx *ctx, int img, unsigned long long *keypoints, unsigned long long *iterations);
/* ---- detection masks ----------------------------------------------------------------------------
 * Restricts the regions of an image to a per-image mask, as cv::Feature2D::detect(image, mask) does (the reference began
 * mods-with-mask.cpp, which loads <image>_mask.png, and never wired it in).  A mask is an 8-bit image of the ORIGINAL image's size
 * (w x h, row stride `stride` >= w bytes): 0 = no regions here, anything else = allowed.
 * The rule: a point (x, y) in original-image coordinates - the doubles a mods_affkey / mods_region carries - is on the mask iff
 * 0 <= ix < w, 0 <= iy < h and mask[iy * stride + ix] != 0 with ix = (int)floor(x + 0.5), iy = (int)floor(y + 0.5) (pixel centres
 * sit at integer coordinates).  Only the centre counts; the measurement region may overlap masked pixels.
 * mods_detection_mask_test states the rule on the host (1 on the mask, 0 off it or on bad arguments; no device needed).
 *  - HessianAffine, DoG, HarrisAffine, plain images and synthesised views (there the centre is the reprojected one, in the original
 *    frame): an extremum with an off-mask centre is removed after the octave-map rule and before affine adaptation.  It still
 *    claims its octave-map cell (which of two rival extrema survives is what it was without a mask), never reaches Baumberg, a shape
 *    network, orientation or description, and takes no part in the export selection: RelativeTh's maximum, FixedRegNumber,
 *    RelativeRegNumber and NotLessThanRegions see on-mask points only.  In FixedTh mode the key and region lists are therefore the
 *    unmasked call's with the off-mask entries deleted, order kept, every field equal to the bit except the list positions in
 *    id / parent.
 *  - MSER: the keys with an off-mask centre are deleted from the key list MSER exports, before orientation; MSER's own count
 *    modes (prepareKeysForExport) have been applied by then, so they count off-mask regions too.
 *  - Regions that come from the caller are not filtered: mods_orient_describe*, the command line's pre-extracted mode,
 *    mods_imgrep_append_*.
 *  - No mask set: the calls are what they were, launch for launch (the gate kernel is not launched).
 * `image` is the index in the call's image list: the batch entry of mods_detect_*_dev / mods_detect_describe_dev*, 0 / 1 for the
 * first / second image of the view2, pair and ladder entry points (whichever context of the ladder runs a view).
 * mods_ctx_detection_mask copies a host mask into a buffer of the context; _dev borrows the caller's device buffer, which must stay
 * valid while it is set (its bytes are read when a call runs: new contents need no new call here).  A null pointer clears that
 * image's mask, _masks_clear all of them.  A mask whose w x h differs from the image of a call makes that call MODS_E_ARG.
 * _counts: entries of image `image` that reached the gate in the context's last call and entries it kept (-1, -1 when the image
 * had no mask in that call); after a ladder call: the sums over the views of the call, whichever context ran them. */
int mods_ctx_detection_mask(mods_ctx *ctx, int image, const unsigned char *mask_host, int w, int h, int stride);
int mods_ctx_detection_mask_dev(mods_ctx *ctx, int image, const unsigned char *mask_dev, int w, int h, int stride);
int mods_ctx_detection_masks_clear(mods_ctx *ctx);
int mods_ctx_detection_mask_counts(mods_ctx *ctx, int image, int *n_accepted, int *n_kept);
int mods_detection_mask_test(const unsigned char *mask, int w, int h, int stride, double x, double y);
int mods_unoriented_count(mods_ctx *ctx, int img);   /* |"None" region list| of slot img after the last describe call */
int mods_regions_fetch(mods_ctx *ctx, int img, mods_region *out, int max_out, int *n_out);

/* parity-test building blocks: one 32x32 orientation patch / one 41x41 descriptor patch */
int mods_dominant_angle(mods_ctx *ctx, const float *patch, int ps, double th, float *angle, int *found);
/* Self-test of the square root the gradient passes use (csrc/device_util.hpp: fast_sqrtf = the compiler's correctly rounded
 * expansion without its denormal rescue) against sqrtf over all 2^32 operands.  out5: {operands of its stated domain (+0, x >= 2^-96,
 * +infinity, NaN) where it differs (must be 0), operands 0 < x < 2^-96 where it differs (allowed), non-negative operands where the
 * everywhere-exact form differs (must be 0), operands visited (2^32), negative operands where either differs (outside both
 * domains: the callers' operands are sums of squares)}. */
int mods_selftest_fast_sqrt(mods_ctx *ctx, unsigned long long *out5);
int mods_sift_patch(mods_ctx *ctx, const float *patch, int ps, int rootsift, double maxBinValue, uint8_t *out128);

/* ---- view synthesis ---------------------------------------------------------------------------
 * Replaces GenerateSynthImageCorr (synth-detection.cpp:324-518; the caller hands over a grey float image,
 * i.e. the state after the (B+G+R)/3 conversion of :343-354) and the per-view body of
 * ImageRepresentation::SynthDetectDescribeKeypoints (imagerepresentation.cpp:704-1099) for
 * HessianAffine + RootSIFT.  tilt < 0 = vertical tilt, phi in radians, as in ViewSynthParameters. */
typedef struct mods_view_geom {
  int identity;              /* 1: the original image is the view (tilt ~ 1, phi ~ 0, zoom ~ 1) */
  int w_rot, h_rot;          /* size after the rotation */
  int w_new, h_new;          /* size of the view */
  int ksize_x, ksize_y, pad; /* anti-aliasing Gaussian */
  double rotation, tilt, zoom;   /* SynthImage fields: degrees, |tilt|, zoom */
  double sigma_x, sigma_y;
  double H[9];               /* original -> view (SynthImage::H), row-major */
  double warpRot[6], warpTilt[6];   /* the two cv::warpAffine matrices (src -> dst) */
} mods_view_geom;

int mods_view_geometry(int w, int h, double tilt, double phi, double zoom, double initSigma, mods_view_geom *out);
/* src_dev: w x h floats in HBM (row stride `stride` floats); dst_dev: out->w_new x out->h_new, dense.
 * The context must hold the rotated intermediate: w_rot * h_rot <= max_w * max_h * batch
 * (max_w = max_h = ceil(hypot(w, h)) is always enough). */
int mods_synth_view_dev(mods_ctx *ctx, const float *src_dev, int w, int h, int stride, const mods_view_geom *geom, int doBlur,
                        float *dst_dev);
/* synthesise + detect + orient + reproject + describe one view; regions (reproj_kp, original frame, with
 * descriptors) stay in the context: mods_regions_fetch(ctx, 0, ...) or mods_regions_dev(ctx, 0). */
int mods_detect_describe_view_dev(mods_ctx *ctx, const float *src_dev, int w, int h, int stride, double tilt, double phi,
                                  double zoom, double initSigma, int doBlur, const mods_hessaff_params *det,
                                  const mods_describe_params *desc, mods_view_geom *geom_out, int *n_detected, int *n_regions);
/* the same view of TWO images of one size (the two images of a pair share their view schedule) in one chain of launches; the
 * context needs batch >= 2; regions of image i stay in slot i (mods_regions_fetch(ctx, i, ...)), n_detected2 / n_regions2: [2] */
int mods_detect_describe_view2_dev(mods_ctx *ctx, const float *src1_dev, const float *src2_dev, int w, int h, int stride, double tilt,
                                   double phi, double zoom, double initSigma, int doBlur, const mods_hessaff_params *det,
                                   const mods_describe_params *desc, mods_view_geom *geom_out, int *n_detected2, int *n_regions2);
const mods_region *mods_regions_dev(mods_ctx *ctx, int img);     /* device pointer of the region list of image `img` */
/* the same regions with desc[0..63] = HalfRootSIFT, desc[64..127] = 0 (filled when mods_describe_params.halfDesc was set) */
const mods_region *mods_regions_half_dev(mods_ctx *ctx, int img);
int mods_regions_fetch_half(mods_ctx *ctx, int img, mods_region *out, int max_out, int *n_out);
int mods_regions_copy_dev(mods_ctx *ctx, int img, mods_region *dst_dev, int n);   /* D2D copy of its first n entries */
const float *mods_view_pixels_dev(mods_ctx *ctx);                /* pixels of the last synthesised view (w_new x h_new) */
int mods_view_fetch(mods_ctx *ctx, const mods_view_geom *geom, float *dst_host);   /* host copy of those pixels */
/* host-buffer primitives (parity tests): cv::warpAffine(LINEAR, BORDER_CONSTANT cval), M maps src -> dst;
 * cv::GaussianBlur(Size(kx,ky), sx, sy, BORDER_REFLECT_101) */
int mods_warp_affine(mods_ctx *ctx, const float *src, int w, int h, const double *M, int dw, int dh, float cval, float *dst);
int mods_gauss_blur_xy(mods_ctx *ctx, const float *src, int w, int h, int kx, int ky, double sx, double sy, float *dst);

/* ---- homography views ------------------------------------------------------------------------
 * A view through an arbitrary homography, and its regions carried back with a per-region linearisation: GenerateSynthImageByH,
 * ReprojectByHReal, ReprojectRegionsBackReal and linH (synth-detection.cpp:519-629, 1498-1518), which the reference began and
 * never wired in.  The views above are affine only; these entry points are their projective counterparts and share none of
 * their kernels (csrc/view_h.hip).
 *
 * The warp.  H is row-major and maps original -> view; G = adj(H) / det(H) (the closed form used throughout this library);
 * d0 = (H6 cx + H7 cy) + H8 at (cx, cy) = ((w - 1) / 2, (h - 1) / 2).  MODS_E_ARG when det(H) == 0, d0 == 0 or an entry of H is
 * not finite.  For the destination pixel (x, y), every operation in fp64 with one rounding:
 *     W = (G6 x + G7 y) + G8;   unless W d0 > 0 the pixel is cval (it lies on or behind the horizon);
 *     t = 32 / W;  fX = ((G0 x + G1 y) + G2) t;  fY = ((G3 x + G4 y) + G5) t;   a NaN makes the pixel cval;
 *     fX, fY are clamped to [INT_MIN, INT_MAX];  X = (int)rint(fX), Y = (int)rint(fY);
 *     sx = X >> 5, sy = Y >> 5, fx = (X & 31) / 32.f, fy = (Y & 31) / 32.f,
 * and from there what mods_warp_affine does: the weights (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx in fp32, the sum
 * v0 w0 + v1 w1 + v2 w2 + v3 w3 in that order, taps outside the source reading cval.  Nothing is stepped along a row.
 * The contract is shaped after cv::warpPerspective(INTER_LINEAR, BORDER_CONSTANT); parity with OpenCV is unpinned, and the
 * W d0 > 0 rule is a deliberate difference: OpenCV mirrors the far side of the horizon into the image, this warp writes cval.
 *
 * mods_view_geometry_h (host only, no device): H, identity = 0, tilt = zoom = 1, w_rot x h_rot = w x h; w_new / h_new =
 * floor(xmax) / floor(ymax) of the images of the corners (0, 0), (0, h), (w, 0), (w, h), each coordinate truncated to an integer
 * first as the reference's cv::Point does, clipped to clip_w x clip_h (both > 0) and to >= 0; a corner with den d0 <= 0 is
 * MODS_E_ARG.  Blur: sigma_x = sigma_y = initSigma / 4, ksize = floor(8 sigma + 1), made odd, at least 3.
 * mods_warp_perspective: host pointers, dense rows - the warp alone.
 * mods_synth_view_h_dev: the isotropic BORDER_REFLECT_101 blur when doBlur (on a dense copy: w h <= max_w max_h batch), then
 * the warp with cval = 128 into dst_dev (geom->w_new x geom->h_new, dense).
 * mods_detect_describe_view_h_dev: synthesise -> detect -> orient and describe the view as a plain image in its own frame
 * (border tests in the view frame) -> one pass over the finished regions of slot 0 and their HalfRootSIFT twins.  For a region
 * (x, y, A, s): den = (G6 x + G7 y) + G8, dropped unless den d0 > 0; rx = ((G0 x + G1 y) + G2) / den, ry likewise; L = linH(x, y,
 * G); A' = L A; s, the response and the descriptor stay.  Kept iff 0 < rx < w, 0 < ry < h, its measurement box (the affine views'
 * box, (int)(k_sigma s)) does not touch the border of the original, and - when slot 0 has a detection mask, which must be w x h -
 * (rx, ry) is on it by mods_detection_mask_test's rule.  The detector itself runs unmasked here: unlike with the gate of the
 * other entry points, off-mask regions still used detector budget (regionsNumber, the count modes).  The survivors keep their
 * order, id = the new position; slot 0 holds them in the ORIGINAL frame, ready for mods_imgrep_append_ctx[_half].  A view under
 * 16 x 16 yields no regions, one larger than the context is MODS_E_ARG.
 * mods_rematch_under_h_dev: the second stage of a two-stage match.  H: a verified img1 -> img2 homography.  Image 1 is seen
 * through H (clipped to w2 x h2) and its regions join rep1; with both != 0 image 2 is seen through inv(H) (clipped to w1 x h1)
 * and its regions join rep2; then the banks go through exactly what mods_match_verify_reps runs.  par->ransac.useF must name a
 * homography model (0 or 3; mods_match_verify_reps itself has no image size for 3), else MODS_E_ARG.  Detection masks are
 * numbered as in the pair entry points: the mask of image 0 filters the regions of image 1's view, that of image 1 those of
 * image 2's.
 * mods_test_warp_perspective_strided / mods_test_reproject_regions_h: the test seams - the warp of a host image with a row
 * stride, and the post-pass over n host regions (in / out; `half`: their twins or NULL) through slot 0, whose mask applies. */
int mods_view_geometry_h(int w, int h, const double *H, int clip_w, int clip_h, double initSigma, mods_view_geom *out);
int mods_warp_perspective(mods_ctx *ctx, const float *src, int w, int h, const double *H, int dw, int dh, float cval, float *dst);
int mods_synth_view_h_dev(mods_ctx *ctx, const float *src_dev, int w, int h, int stride, const mods_view_geom *geom, int doBlur,
                          float *dst_dev);
int mods_detect_describe_view_h_dev(mods_ctx *ctx, const float *src_dev, int w, int h, int stride, const double *H, int clip_w, int clip_h,
                                    double initSigma, int doBlur, const mods_hessaff_params *det, const mods_describe_params *desc,
                                    mods_view_geom *geom_out, int *n_detected, int *n_regions);
int mods_test_warp_perspective_strided(mods_ctx *ctx, const float *src, int w, int h, int stride, const double *H, int dw, int dh, float cval,
                                       float *dst);
int mods_test_reproject_regions_h(mods_ctx *ctx, const double *H, int ow, int oh, mods_region *regions, mods_region *half, int n, int *n_out);

/* ---- B4: matching ------------------------------------------------------------------------------
 * Replaces  int MatchFlannFGINN(const AffineRegionList &q, const AffineRegionList &t,
 *           TentativeCorrespListExt &out, const MatchPars &par, const int nn = 50)
 * (matching/matching.hpp:261-262, matching.cpp:356-460) for vector_matcher = linear, vector_dist = L2:
 * exact brute-force squared-L2 search (ties: lower train index first), FGINN walk over nn neighbours.
 * ratio = par.currMatchRatio (FGINNThreshold of the iters .ini), contradDist = [Matching] contradDist.
 * Tentatives come out in query order.  u6_out (optional, 6 doubles per tentative) receives the
 * correspondences as LORANSACFiltering lays them out for degensac: x1 y1 1 x2 y2 1; laf_out (optional,
 * 14 doubles per tentative) the two local affine frames x y a11 a12 a21 a22 s used by the LAF checks. */
int mods_match_fginn(mods_ctx *ctx, const mods_region *q, int n_q, const mods_region *t, int n_t, double ratio,
                     double contradDist, int nn, mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out);
/* same, on the HBM-resident region lists of images img_q / img_t left by mods_detect_describe_dev */
/* MatchFLANNDistance (matching/matching.cpp:572-633) with binary_dist = Hamming (io_mods.cpp:365) and an exact index: the
 * nearest train of every query by Hamming distance over the 128 descriptor bytes is a tentative when the distance is at most
 * (int)(float)threshold; d1, d2 = the two smallest distances (ties by train index), ratio = d1 / d2. */
int mods_match_distance(mods_ctx *ctx, const mods_region *q, int n_q, const mods_region *t, int n_t, double threshold,
                        mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out);
int mods_match_dev(mods_ctx *ctx, int img_q, int img_t, double ratio, double contradDist, int nn, mods_tentative *out,
                   double *u6_out, double *laf_out, int max_out, int *n_out);
/* Launch geometry of the first pass of an n_q x n_t FGINN search: out = {query blocks, train splits, 32-row train tiles per split}.
 * Host arithmetic only (no device, no launch); n_q or n_t < 1 or a null out: MODS_E_ARG.  The result of a search does not depend on
 * it; tests use it to know which tile-loop variant a list length reaches. */
int mods_match_grid(int n_q, int n_t, int out[3]);

/* Exact k-nearest-neighbour search (what cv::DescriptorMatcher::knnMatch and FLANN's knnSearch give; the reference calls the
 * latter with nn = 50).  For every query i and K = min(k, n_t), row i of the result holds the K trains with the smallest keys
 * (d, t) in increasing key order: d = the exact integer squared L2 distance over the 128 descriptor bytes (0 .. 8 323 200), t = the
 * train's index in the list it was given in; ties in d go to the lower index, as in mods_match_fginn.  Positions K .. k-1 of a row
 * hold index -1 and distance INT_MAX.  Nothing depends on a summation or visiting order: the result is defined to the bit.  FLANN's
 * own order among equal distances is not pinned against this one.
 * idx_out, d2_out: [n_q][k] ints on the host; either may be null, not both.
 * mods_match_knn       host lists, staged as mods_match_fginn stages them
 * mods_match_knn_dev   the region lists the context holds after mods_detect_describe_dev (img_q == img_t is allowed: the nearest
 *                      train of a region is then itself, or an equal descriptor at a lower index)
 * mods_match_knn_reps  queries [q_begin, q_end) of a bank; rows are relative to q_begin, train indices refer to the full bank
 * Refusals (MODS_E_ARG, before any device call): a null context, list or bank, both outputs null, k < 1 or k > 64, a negative
 * count, q_begin > q_end or a range outside the bank, an image index outside the last described batch; a list longer than the
 * context's capacity: MODS_E_CAPACITY.  n_q == 0: MODS_OK, nothing is written; n_t == 0: MODS_OK, every row is padding.
 * State: the search has buffers of its own, reserved on first use.  It leaves the matcher's "last search" (what
 * mods_match_fetch_internal and the fetch entry points read), the guided and the overlap buffers alone, and it ignores
 * mods_ctx_match_mutual.  Timers: MODS_STAGE_KNN, MODS_STAGE_KNN_SWEEP.
 * mods_match_knn_grid: {query blocks, train splits, 32-row train tiles per split} of the sweep for these sizes (n_q, n_t >= 0) and a
 * forced split count (0: the library's choice; at most 64 splits and never more than the list has tiles; trailing splits of a forced
 * count may be empty).  Host arithmetic only.  mods_ctx_knn_splits sets that forced count for a context (0: the library chooses); a
 * testing knob, the result never depends on it.  A negative count: MODS_E_ARG. */
int mods_match_knn(mods_ctx *ctx, const mods_region *q, int n_q, const mods_region *t, int n_t, int k, int *idx_out, int *d2_out);
int mods_match_knn_dev(mods_ctx *ctx, int img_q, int img_t, int k, int *idx_out, int *d2_out);
int mods_match_knn_grid(int n_q, int n_t, int k, int forced_splits, int out[3]);
int mods_ctx_knn_splits(mods_ctx *ctx, int splits);

/* Replaces  void DuplicateFiltering(TentativeCorrespListExt &in, const double r, const int mode)
 * (matching.cpp:2615-2679).  Host-side, in place on (tent, u6); mode 0 = keep order (MODE_RANDOM),
 * 1 = best FGINN ratio first, 2 = best distance first (configuration.hpp:31-34); equal keys keep
 * list order. */
int mods_duplicate_filter(mods_tentative *tent, double *u6, double *laf, int n, double r, int mode, int *n_out);
/* The same filter on the context's GPU (csrc/dedup.hip: rank count for the order, brute-force near-predecessor lists, fixed-point
 * resolution of the keep / drop rule; the pair entry points run it behind the search when [DuplicateFiltering] doBeforeRANSAC = 1).
 * Host lists in and out as above, laf required; identical result.  *on_device (optional) = 0 when the list was handed to the
 * host filter instead (a correspondence with more than 12 near predecessors, or more than 150 k correspondences).
 * The call stages the list in the context's tentative buffer: it replaces the "last search" that mods_match_fetch_internal and
 * the fetch entry points of the matcher read (run it after those, or search again). */
int mods_duplicate_filter_gpu(mods_ctx *ctx, mods_tentative *tent, double *u6, double *laf, int n, double r, int mode, int *n_out,
                              int *on_device);

/* ---- B1: verification ---------------------------------------------------------------------------
 * The degensac C ABI itself is exported with the reference's exact signatures (degensac/exp_ranH.h:32-36,
 * degensac/Htools.h): exp_ransacHcustom, HDs, HDsSym, HDsSymMax, HDsi, HDsiSym, HDsiSymMax, HDsidx,
 * HDsSymidx, HDsSymidxMax - see include/mods_degensac.h.  Hypotheses are scored on the GPU.
 *
 * [RANSAC] keys (io_mods.cpp:437-455).  errorType: 0 Sampson, 1 SymmMax, 2 SymmSum. */
typedef struct mods_ransac_params {
  double err_threshold;     /* 4.0 px */
  double confidence;        /* 0.99 */
  int max_samples;          /* 1000000 */
  int localOptimization;    /* 1 */
  double LAFCoef;           /* 2 (F branch) */
  double HLAFCoef;          /* 12 */
  int errorType;            /* 0 */
  int doSymmCheck;          /* 1 */
  int useF;                 /* 0: homography (ver_type "Homog"), 1: epipolar geometry (DEGENSAC, ver_type "Epipolar"),
                             * 2: epipolar geometry verified by ORSA (RANSAC_mode_t ORSA; mods_orsa_f),
                             * 3: homography verified by ORSA-H (mods_orsa_h); mods_model_kind() tells H from F */
  /* ver_type 1 of the command line (GR_TRUTH, mods.cpp:290-320): verification against a known homography.
   * groundTruth 0: off; 1: HMatrixFiltering of the tentatives only; 2: doBothRANSACgroundTruth - LORANSACFiltering first, then
   * HMatrixFiltering of its inliers (the verified list), next to HMatrixFiltering of all tentatives for the log. */
  int groundTruth;
  int ransacForStopping;    /* [Matching] RANSACforStopping: in ground-truth mode the step loop stops on the RANSAC inlier count */
  double gtH[9];            /* the homography img1 -> img2, row-major, as the file of argv[Tmin+2] holds it (mods.cpp:92-98) */
} mods_ransac_params;

/* Replaces  int HMatrixFiltering(TentativeCorrespListExt &in, TentativeCorrespListExt &true_corresp, double *H, const int isExtended,
 *           const RANSACPars pars)  (matching/matching.cpp:917-1012): mask[i] = 1 where the error of correspondence i under H
 * (errorType: 0 HDs Sampson, 1 HDsSymMax, otherwise HDsSym; the point of the second image first, as the reference stacks it) is at
 * most (float)(err_threshold^2).  H_rowmajor: img1 -> img2.  Host-side. */
int mods_hmatrix_filter(const double *u6, int n, const double *H_rowmajor, const mods_ransac_params *par, unsigned char *mask, int *n_true);

/* Replaces  int LORANSACFiltering(TentativeCorrespListExt &in, TentativeCorrespListExt &out, double *H,
 *           const RANSACPars pars)  (matching/matching.hpp:267-269, matching.cpp:637-805) for useF = 0.
 * u6: n x 6 correspondences, laf: n x 14 frames (may be NULL: LAF check skipped).  mask[i] = 1 for the
 * correspondences kept after RANSAC + NaiveHCheck + H_LAF_check; H_out row-major img1 -> img2
 * (all -1 when no model).  stats3 (optional) = {samples drawn, LO runs, orientation rejects}. */
int mods_loransac_h(const double *u6, const double *laf, int n, const mods_ransac_params *par, unsigned char *mask,
                    double *H_out, int *n_inliers, int *stats3);
/* The useF = 1 branch of the same function (matching.cpp:711-726, 804-816): exp_ransacFcustom (inlLimit 0,
 * error functions by errorType: 0 FDs/exFDs, otherwise FDsSym/exFDsSym) followed by F_LAF_check
 * (matching.cpp:192-249, bound LAFCoef * err_threshold).  F_out = the matrix as degensac stores it
 * (x2^T F x1 = 0, F_out[3*c + r] = entry (r, c)), as ransac_corresp.H receives it; all -1 when n < 8.
 * stats3 = {samples drawn, LO runs, plane consensus *Ih}. */
int mods_loransac_f(const double *u6, const double *laf, int n, const mods_ransac_params *par, unsigned char *mask,
                    double *F_out, int *n_inliers, int *stats3);
/* Replaces  int ORSAFiltering(TentativeCorrespListExt &in, TentativeCorrespListExt &out, double *F, const RANSACPars pars, int w,
 *           int h)  (matching/matching.cpp:824-914) for useF = 2: orsa() (orsa.cpp:371-678) in mode 2 with t = 10000, seeded as
 * srand(time(NULL)) (mods_ransac_pin_seed / MODS_RANSAC_SEED pin it), hypotheses scored on the GPU (csrc/orsa.hip).  w, h: the
 * image size the reference passes (in the step loop ((w1 + w2) / 2, (h1 + h2) / 2), mods.cpp:347-350).  When log(nfa) < -2 the
 * verified list is the first miniall + 1 tentatives in input order (the reference's own rule), then F_LAF_check (FDs for
 * errorType 0, FDsSym otherwise; bound LAFCoef * err_threshold), cleared below 8; mask[i] = 1 for those.  F_out: the matrix as
 * ransac_corresp.H receives it (the transpose of orsa()'s Fout), all -1 when not significant or n < 8.  log_nfa: orsa()'s
 * return value (10000 when nothing was scored).  index_out (n entries or NULL): the sorted indices of the most meaningful subset,
 * *n_index = miniall of them.  stats3 = {iterations, models scored, rewinds of a block after an optimisation trigger}. */
int mods_orsa_f(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                double *F_out, int *n_inliers, float *log_nfa, int *index_out, int *n_index, int *stats3);
/* the same with the scoring back end chosen: on_device 0 = the host scalar path (matcherrorn + glibc qsort per model, no device
 * needed; the device's oracle); batch = iterations solved and scored per block, wg_keys = key slots a workgroup packs models into
 * (<= 0: MODS_ORSA_BATCH / MODS_ORSA_WG_KEYS or 512 / 1024).  Results do not depend on batch, wg_keys or MODS_RANSAC_THREADS. */
int mods_orsa_f_ex(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                   double *F_out, int *n_inliers, float *log_nfa, int *index_out, int *n_index, int *stats3, int on_device, int batch,
                   int wg_keys);
/* the calling thread's last mods_orsa_f[_ex] call: ms5 = {host 7-point solves, scoring (device round trips or host), scoring
 * kernels (HIP events), replay, whole call}, *launches = scoring launches */
int mods_orsa_last_profile(double *ms5, long *launches);
/* self-test hooks of ORSA's host pieces (no device needed): epipolar() on the 7 points k7 of p1 / p2 (n x 2 floats each) -> F1, F2
 * (row-major), z[3], returns the number of roots; the logcombi tables of n (n + 1 entries each); (float)log10((double)x) as glibc
 * rounds it.  mods_test_orsa_score: the per-model results {nfa bits, first argmin, logalpha bits, NaN flag} of m models F (m x 9
 * row-major) over the normalised points p1 / p2 of an image w x h, through the device kernel (on_device 1) or the host path. */
int mods_test_orsa_epipolar(const float *p1, const float *p2, const int *k7, float *F1, float *F2, float *z);
int mods_test_orsa_tables(int n, float *logcn, float *logc7);
int mods_test_orsa_log10(const float *x, int n, float *out);
int mods_test_orsa_score(const float *p1, const float *p2, int n, int w, int h, const float *F, int m, int on_device, int wg_keys,
                         int *out4);
/* the device's (float)log10((double)x) against glibc's for the float bit patterns [begin, begin + count): the number of
 * mismatches (< 0: MODS_E_*), the first max_list of them in list */
long long mods_test_orsa_log10_sweep(unsigned begin, unsigned count, unsigned *list, int max_list);

/* ORSA-H, useF = 3: a-contrario homography verification after Moisan, Moulon, Monasse, "Automatic Homographic Registration of a
 * Pair of Images, with A Contrario Elimination of Outliers", IPOL 2012.  The reference tree has no such verifier: the contract is
 * this project's own, stated here, restated in numpy in tests/orsa_h_ref.py and pinned to the bit between the device and the host
 * path (parity with the IPOL code unpinned).  Arguments as mods_orsa_f; the model maps image 1 (u6[0..1]) to image 2 (u6[3..4]).
 * n < 8: no model, MODS_OK.
 *  - Normalisation as orsa(): norm = 1 / (float)sqrt(nx ny), points centred by half the size, scaled, stored as float.
 *  - Sampling: 4 raw rand() values of glibc's generator per iteration (seeded as mods_orsa_f: mods_ransac_pin_seed /
 *    MODS_RANSAC_SEED), mapped to 4 distinct indices the way random_p7 maps 7, over the current (nid, id).
 *  - Minimal solve: the 8 x 8 system of the 4 correspondences with h33 = 1, rows (x, y, 1, 0, 0, 0, -ux, -uy | u) and
 *    (0, 0, 0, x, y, 1, -vx, -vy | v), fp64 Gaussian elimination with partial pivoting (the first largest magnitude wins), fixed
 *    operation order, no contraction, rounded to 9 floats.  A zero (or NaN) pivot or a non-finite entry: the model is invalid.
 *  - Error of correspondence i: the squared distance in image 2 between H p1 (after the projective division) and p2, in double
 *    from the float operands, rounded to float; its bits are the sort key.  A NaN error makes the model invalid, +inf is an
 *    ordinary key.  An invalid model scores nfa = 10000, imin = 0.
 *  - NFA over the sorted errors e_i, 0-based 4 <= i < n, in float: la = logalpha0 + (float)log10((double)max(e_i, FLT_MIN)),
 *    nfa = loge0 + la (float)(i - 3) + logcn[i + 1] + logc4[i + 1], logalpha0 = (float)log10(pi) (the normalised image has area 1;
 *    the log of a squared point error enters with multiplier 1), loge0 = (float)log10((double)(n - 4)), logcn[m] = logcombi(m, n),
 *    logc4[m] = logcombi(4, m).  The lowest i among equal values wins.
 *  - Control loop: orsa()'s, t = 10000, maxniter = t - t / 10; one model per iteration; a record below 0 - or the last iteration,
 *    where a record exists - starts the optimisation phase, which samples from the record's subset for t / 10 more iterations.  The
 *    subset is the first imin + 1 indices of the errors sorted stably by (error, index).
 *  - Final refit: one least-squares model (u2h) from the record's subset, rounded to 9 floats, scored like any other; it replaces
 *    the record only where its NFA is lower.
 * When log_nfa < -2: H_out row-major, image 1 to image 2, in pixels (T^-1 h T in double); *thr_px = sqrt(e_imin) / norm, the
 * data-driven inlier threshold in pixels; index_out / *n_index = the subset in sorted order; mask = 1 on the subset, then - laf
 * given and HLAFCoef > 0 - H_LAF_check with bound HLAFCoef * thr_px, cleared below 8.  Otherwise H_out is all -1 and the mask
 * empty.  log_nfa: 10000 when nothing was scored.  stats3 = {iterations, models scored, rewinds}. */
int mods_orsa_h(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                double *H_out, int *n_inliers, float *log_nfa, double *thr_px, int *index_out, int *n_index, int *stats3);
/* the same with the scoring back end chosen, as mods_orsa_f_ex: on_device 0 = the host path (no device needed), which runs the
 * same solver and error function.  Results do not depend on batch, wg_keys or MODS_RANSAC_THREADS.  mods_orsa_last_profile
 * reports these calls too (ms5[0]: the mapping of the samples; the solves run inside the scoring kernel). */
int mods_orsa_h_ex(const double *u6, const double *laf, int n, int w, int h, const mods_ransac_params *par, unsigned char *mask,
                   double *H_out, int *n_inliers, float *log_nfa, double *thr_px, int *index_out, int *n_index, int *stats3,
                   int on_device, int batch, int wg_keys);
/* the refit of the calling thread's last mods_orsa_h[_ex] call: the loop's best NFA, the refit model's (10000: none scored or
 * invalid), and whether it replaced the record */
int mods_orsa_h_last_refit(float *nfa_loop, float *nfa_refit, int *taken);
/* log_nfa and thr_px (0 when not significant) of the calling thread's last mods_orsa_h[_ex] call, for callers that reach it
 * through the pair, pipeline or ladder entry points (the command line's verbose report) */
int mods_orsa_h_last_threshold(double *thr_px, float *log_nfa);
/* self-test hooks: the tables logcn, logc4 of n (n + 1 entries each); the solve and scoring of m samples (samples4: m x 4 distinct
 * indices below n) over the normalised points p1 / p2 (n x 2 floats, image 1 / 2; n >= 5), through the device kernel (on_device 1)
 * or the host path: out4 per model = {nfa bits, first argmin, logalpha bits, invalid flag}, H_out9 = the m solved models */
int mods_test_orsa_h_tables(int n, float *logcn, float *logc4);
int mods_test_orsa_h_score(const float *p1, const float *p2, int n, int w, int h, const int *samples4, int m, int on_device,
                           int wg_keys, int *out4, float *H_out9);
/* the model a value of mods_ransac_params.useF verifies: 0 = homography (useF 0, 3), 1 = fundamental matrix (useF 1, 2),
 * MODS_E_ARG for any other value */
int mods_model_kind(int useF);
/* The verification half of one step of the reference's loop (mods.cpp:278-368), in place on (tent, u6, laf):
 *   par->dup_before_ransac = 1 ([DuplicateFiltering] doBeforeRANSAC): DuplicateFiltering (mods.cpp:283), then LORANSACFiltering;
 *   par->dup_before_ransac = 0: LORANSACFiltering on every tentative, then DuplicateFiltering on the verified list
 *   (mods.cpp:357-368; TrueMatch1st = the size of the de-duplicated list, which also drives the minMatches stop).
 * On return the first *n_verified entries of tent / u6 / laf are the verified correspondences in output order and *n_unique is
 * the size of the list the RANSAC ran on.  H_out, stats3 as mods_loransac_h / _f; ms_dup / ms_ransac (optional): wall clock. */
struct mods_pair_params;
int mods_verify_tentatives(int device, const struct mods_pair_params *par, mods_tentative *tent, double *u6, double *laf, int n,
                           int *n_unique, int *n_verified, double *H_out, int *stats3, double *ms_dup, double *ms_ransac);
/* the same with the three ground-truth counts of mods_ladder_result (gt3, may be NULL; zeros outside ground-truth mode) */
int mods_verify_tentatives_ex(int device, const struct mods_pair_params *par, mods_tentative *tent, double *u6, double *laf, int n,
                              int *n_unique, int *n_verified, double *H_out, int *stats3, int *gt3, double *ms_dup, double *ms_ransac);
/* the same with the image size (w, h) that useF = 2 and 3 (ORSA: mods_orsa_f, mods_orsa_h) need; the two calls above have none and
 * return MODS_E_ARG for them.  mods_match_pair_dev and the pipeline pass their frame size. */
int mods_verify_tentatives_wh(int device, const struct mods_pair_params *par, mods_tentative *tent, double *u6, double *laf, int n,
                              int w, int h, int *n_unique, int *n_verified, double *H_out, int *stats3, int *gt3, double *ms_dup,
                              double *ms_ransac);
/* GPU used by the degensac entry points of the calling thread (default 0). */
int mods_ransac_set_device(int device);
/* The reference seeds with srand(time(NULL)) (exp_ranH.c:823).  seed >= 0 makes every call behave as if
 * time(NULL) returned `seed`; seed < 0 restores the wall clock.  MODS_RANSAC_SEED in the environment
 * has the same effect when no seed is pinned. */
void mods_ransac_pin_seed(long seed);
/* self-test hook: first n values of srand(seed); rand(); ... from the restated glibc generator */
void mods_test_glibc_rand(unsigned seed, int n, int *out);
/* self-test hooks of the fast host forms of the homography LO step (no device needed): the error functions at a given
 * SIMD width (lanes 0 = the scalar HDs / HDsSym / HDsSymMax, 1 / 4 / 8 = vector forms; MODS_E_ARG when the CPU lacks the
 * width), u2h and its moment matrix with the design matrix written out (reference_form 1: lin_hgN + cov_mat,
 * Htools.c:60-132, utools.c:172-185) or folded into 30 ordered sums (0), and inlidxs (rtools.c:155-166; lanes < 0: the list-only
 * form of the wide-threshold sets - count and list, J = 0). */
int mods_test_host_errfn(int type, const double *u6, int len, const double *H, int lanes, double *out);
int mods_test_host_u2h(const double *u6, const int *inl, int n, int reference_form, double *H);
int mods_test_host_cov(const double *u6, const int *inl, int n, int reference_form, double *Cv);
int mods_test_host_inlidxs(const double *err, int len, double th, int lanes, int *inl, unsigned *I, double *J);
/* the operands of HDsSym / HDsSymMax of a model H, as every scored hypothesis record carries them (Htools.c:206-221): Hinv = H
 * transposed as stored, H1 = minv(Hinv) (left as the inversion leaves it when H is singular) */
int mods_test_host_sym_prepare(const double *H, double *Hinv, double *H1);
/* mods_test_host_cov also takes reference_form 2 (the 30 folded sums in scalar code) and 100 + lanes (the sums through the SIMD
 * table of that width).  The checks LORANSACFiltering runs behind the homography (H -> inv(H^T), NaiveHCheck, H_LAF_check;
 * matching.cpp:745-805, 1014-1043, 250-308) over the correspondences with inl[i] != 0: lanes 0 = the scalar statement, 1 / 4 / 8 =
 * lanes-wide; mask[n], H_out[9], returns the number of survivors (< 0: MODS_E_*). */
int mods_test_host_hchecks(const double *u6, const double *laf14, int n, const unsigned char *inl, const double *Hloran,
                           const mods_ransac_params *par, int lanes, unsigned char *mask, double *H_out);
/* the same for the epipolar error functions of the F-matrix path: mode 0 FDs, 1 FDsSym, 2 exFDs, 3 exFDsSym (Ftools.c:94-209) */
int mods_test_host_fds(int mode, const double *u6, int len, const double *F, int lanes, double *p, double *w);
/* self-test hooks of the host-side pieces of the F-matrix path (no device needed; they let the CPU
 * test-suite compare the restated solvers with the reference's own degensac build, oracle/_ref):
 *   seven_point : u7 = 7 correspondences (7 x 6) -> up to 3 matrices in F27, returns their number
 *                 (-1: null space not two-dimensional)           [exp_ranF.c:884-911]
 *   u2f         : least-squares F of n >= 8 correspondences idx[] of u, optional weights w[len]   [Ftools.c:302-405]
 *   checksample : plane-degeneracy test of a 7-point sample      [DegUtils.c:42-82]
 *   inner_h     : homography LO of the degenerate branch, generator seeded with `seed`   [DegUtils.c:699-735]
 *   rfth        : plane-and-parallax search, generator seeded with `seed`, candidates counted on the host  [DegUtils.c:233-444] */
int mods_test_seven_point(const double *u7, double *F27);
void mods_test_u2f(const double *u, const int *idx, int n, const double *w, double *F);
void mods_test_u2f_form(const double *u, const int *idx, int n, const double *w, int reference_form, double *F);   /* 1: matrix written out */
int mods_test_checksample(const double *F, const double *u7, double th, double *H);
unsigned mods_test_inner_h(unsigned seed, double *H, const double *u, unsigned len, double th, unsigned iters, unsigned char *inl);
unsigned mods_test_rfth(unsigned seed, const double *u, const unsigned char *hinl, double th, const double *H, unsigned len, double *F);
/* self-test hook of the host half of the MSER detector (csrc/mser_host.hpp; no device needed): the grey-level growth of one
 * polarity (invert = 1: MSER-) of a w x h 8-bit image - GetExtrema + FastSetOptThresholds4StableRegion (getExtrema.cpp:385-437,
 * optThresh.cpp:73-165).  out5: rows seed_x, seed_y, threshold, margin, area in output order; tree_out (optional): 3 ints per
 * pixel of the (w + 2) x (h + 2) frame = the merge tree the kernels walk (slot at entry, parent slot or 0x7fffffff, merge level).
 * Returns the number of stable thresholds. */
int mods_test_mser_grow(const unsigned char *img8, int w, int h, int min_size, double max_area, double min_margin, int invert,
                        int *out5, int max_out, int *tree_out);
/* self-test hook of the owning buffer type (csrc/buffer.hpp; no device needed): runs it over a memory policy that counts and fails on a
 * chosen allocation.  report (n >= 16): [0] calls made by a reserve below the capacity, [1] frees and [2] allocations of one growth,
 * [3] 1 when a failed growth left get() == nullptr, [4] its capacity(), [5] frees during it, [6] allocations of the reserve that
 * follows, [7] 1 when moves, swap and detach behaved, [8] buffers of a group left non-empty by a failed group reservation (summed
 * over the failing position), [9] 1 when a group reservation succeeded with [10] buffers at their size, [11] frees of a pointer
 * that was not live, [12] allocations alive after every buffer was destroyed, [13] allocations made, [14] frees made, [15] the
 * group's size.  Returns the number of entries filled. */
int mods_test_buffer_growth(int *report, int n);
/* Host threads the degenerate branch of DEGENSAC spreads its independent pieces over (csrc/ransac_pool.hpp): MODS_RANSAC_THREADS, by
 * default the cores this process may use, at most 8; 1 = the one-thread loops.  Results do not depend on it. */
int mods_ransac_host_threads(void);
/* innerH through the host SIMD evaluation of the production path (simd = 0: scalar); *next_rand = the generator's next value after
 * the call; *path = 0 one-thread loop, 1 repetitions side by side on the pool's threads, 2 side by side, then redone by the loop */
unsigned mods_test_inner_h2(unsigned seed, double *H, const double *u, unsigned len, double th, unsigned iters, unsigned char *inl, int simd,
                            int *next_rand, int *path);
/* the same through the host SIMD evaluation of the production path (simd = 0: scalar); *next_rand = the generator's next value
 * after the call, prof10 (optional) = the call's breakdown (10 doubles, ransac_f_host.hpp: g_rfth_prof) */
unsigned mods_test_rfth2(unsigned seed, const double *u, const unsigned char *hinl, double th, const double *H, unsigned len, double *F,
                         int simd, int *next_rand, double *prof10);
/* test seams of the scoring and counting kernels behind exp_ransacHcustom / exp_ransacFcustom (csrc/ransac.hip, ransac_f.hip; they
 * need a device).  Each one works in the calling thread's scoring workspace and goes through the function the control loop itself
 * calls (gpu_score, gpu_score_f, gpu_upload_aux + gpu_count_pairs_begin / _end, gpu_count_models), so whatever that function
 * chooses per launch - the grid, the gain kernel of the round's width, the buffer slot - is chosen here as it is in a run.  A seam
 * leaves the workspace as a scoring round of a run leaves it (device counters zero), so seam calls and whole runs may alternate
 * on one thread.  tests/ransac_score_ref.py restates what they compute.
 *   score_h : one scoring round of n models h (n x 9, column-major as exp_ransacHcustom carries them) over u6 (len x 6), the
 *             records filled as the run fills them (h, then Hinv = h transposed as stored and H1 = minv(Hinv), Htools.c:206-221).
 *             err_type 0 Sampson, 1 symmetric sum, 2 symmetric max; do_sym: count the symmetric check too.  d_out[n][len] = every
 *             error row, J_out[n] = the MSAC scores (the sequential sums of the gains in correspondence order), counts_out[n][2] =
 *             {#(d <= th), #(d1 + d2 <= th_check), 0 without do_sym}, hyp27_out[n][27] (optional) = the records as uploaded.
 *             n <= 16 runs the 16-column gain kernel, as a run's first batch does.
 *   score_f : the same for n matrices f (n x 9, as exp_ransacFcustom carries them); err_type 0 Sampson, 1 symmetric epipolar;
 *             counts_out[n][2] = {#(d <= th), #(symmetric d <= th_check)}.
 *   count_pairs : the plane-and-parallax candidates of rFtH (DegUtils.c:353-382) given as index pairs into the n off-plane
 *             correspondences uN (n x 6) and their plane-transferred form us (n x 6), Ht = H transposed: F = ([e]x Ht)^T made on
 *             the device, counts[j] = #{i < n : FDs(uN_i, F_j) < limit}.  Two blocks (k0, k1 pairs, 1 .. 2048 each, indices < n)
 *             are counted in slots 0 and 1 with both in flight, as rFtH queues them.
 *   count_models : counts[j] = #{i < len : FDs(u6_i, Fs_j) < limit} for k matrices Fs (k x 9), as innerFH's rounds count theirs.
 * MODS_E_ARG for null, empty or out-of-range input, MODS_E_NODEVICE, MODS_E_HIP. */
int mods_test_ransac_score_h(const double *u6, int len, const double *h, int n, int err_type, int do_sym, double th, double th_check,
                             double *d_out, double *J_out, int *counts_out, double *hyp27_out);
int mods_test_ransac_score_f(const double *u6, int len, const double *f, int n, int err_type, int do_sym, double th, double th_check,
                             double *d_out, double *J_out, int *counts_out);
int mods_test_ransac_count_pairs(const double *uN, const double *us, int n, const double *Ht, double limit, const unsigned *pairs0, int k0,
                                 const unsigned *pairs1, int k1, unsigned *counts0, unsigned *counts1);
int mods_test_ransac_count_models(const double *u6, int len, const double *Fs, int k, double limit, unsigned *counts);

/* ---- whole hot path for one image pair ---------------------------------------------------------
 * The step loop body of mods.cpp:202-383 for one step of HessianAffine + RootSIFT on identity views:
 *   SynthDetectDescribeKeypoints x2 (mods.cpp:234-251) -> MatchImgReps (:270) -> DuplicateFiltering
 *   (:283) -> LORANSACFiltering (:325). */
typedef struct mods_pair_params {
  mods_hessaff_params det;
  mods_describe_params desc;
  double fginn_ratio;        /* iters .ini: FGINNThreshold = 0.8 */
  double contradDist;        /* [Matching] contradDist = 10 */
  int nn;                    /* 50 */
  int dup_before_ransac;     /* [DuplicateFiltering] doBeforeRANSAC = 1 */
  double dup_dist;           /* duplicateDist = 2.0 */
  int dup_mode;              /* whichCorrespondenceRemains: random 0, bestFGINN 1, bestDistance 2, biggerRegion 3 */
  mods_ransac_params ransac;
} mods_pair_params;

typedef struct mods_pair_result {
  int n_detected[2];         /* regions per image after affine adaptation */
  int n_described[2];        /* descriptors per image */
  int n_tentatives;          /* after FGINN matching */
  int n_unique;              /* after duplicate filtering */
  int n_inliers;             /* after RANSAC + NaiveHCheck + H_LAF_check */
  int ransac_samples, ransac_lo, ransac_rejects;
  double H[9];               /* row-major img1 -> img2, all -1 when verification failed; with ransac.useF: F as degensac stores it */
  /* wall-clock per stage in ms, the reference's TimeLog buckets (detectors/structures.hpp:33-56) */
  double ms_detect_describe, ms_match, ms_duplicates, ms_ransac;
} mods_pair_result;

/* img_dev: [2][h][stride] fp32 in HBM (image 1, image 2).  matches_out (optional): up to max_matches
 * rows x1 y1 x2 y2 of the verified correspondences (matchings.txt layout, matching.cpp:2610-2611). */
int mods_match_pair_dev(mods_ctx *ctx, const float *img_dev, int w, int h, int stride, const mods_pair_params *par,
                        mods_pair_result *res, double *matches_out, int max_matches);

/* ---- multi-view representation and the MODS step loop ---------------------------------------------------
 * mods_view_schedule   = SetVSPars for one detector (synth-detection.cpp:191-322): views of a step that no
 *                        earlier step produced; `prev`/`n_prev` is the history, extended in place.
 * mods_imgrep          = the accumulated (HessianAffine, RootSIFT) regions of one image,
 *                        ImageRepresentation::AddRegions (imagerepresentation.cpp:637-684); HBM resident.
 * mods_match_reps      = CorrespondenceBank::MatchImgReps, separate-detector branch (correspondencebank.cpp:288-340)
 *                        for a slice of the queries (the slice is what a rank of the multi-GPU path owns).
 * mods_match_ladder_dev= the step loop of mods.cpp:202-383 on one GPU: per step, new views of both images ->
 *                        match all accumulated regions -> duplicate filter -> LO-RANSAC; stops at min_matches. */
typedef struct mods_view_par { double zoom, tilt, phi; } mods_view_par;      /* ViewSynthParameters subset */
typedef struct mods_imgrep mods_imgrep;
typedef struct mods_ladder_step {     /* one [HessianAffine<i>] section of the iterations .ini (io_mods.cpp:457-492) */
  double scale_set[8]; int n_scales;  /* ScaleSet */
  double tilt_set[8]; int n_tilts;    /* TiltSet */
  double phi;                         /* Phi: rotation density in degrees */
  double initSigma;                   /* initSigma */
  int doBlur;                         /* 1 (io_mods.cpp:475) */
  double fginn_ratio;                 /* FGINNThreshold of RootSIFT (0: RootSIFT lists are not matched) */
  int half_orientation;               /* a descriptor of the step is a Half* one: orientation in doHalfSIFT mode for all of them */
  double fginn_ratio_half;            /* FGINNThreshold of HalfRootSIFT; 0: not described / not matched.  [Matching<i>]
                                         SeparateDescriptors = RootSIFT,HalfRootSIFT: both lists are matched and joined,
                                         HalfRootSIFT first (the bank's key order, correspondencebank.cpp:114-148, 288-340) */
  double dist_threshold;              /* DistanceThreshold of RootSIFT / of HalfRootSIFT: > 0 runs MatchFLANNDistance (nearest by */
  double dist_threshold_half;         /* Hamming distance within the threshold, matching.cpp:572-633), whose tentatives REPLACE the
                                         FGINN ones of that descriptor (it clears the list it appends to) */
} mods_ladder_step;
typedef struct mods_ladder_result {
  int steps_done, n_views;            /* steps executed; views synthesised (both images) */
  int n_detected[2], n_described[2];  /* summed over views / accumulated regions per image */
  int n_unoriented[2];                /* detections inside the image, summed over views (log: UnorientedReg) */
  int n_tentatives, n_unique, n_inliers;   /* of the last step */
  int ransac_samples, ransac_lo, ransac_rejects;
  double H[9];
  double ms_detect_describe, ms_match, ms_duplicates, ms_ransac;
  /* ground-truth mode (mods_ransac_params.groundTruth), of the last step: TrueMatch1st of HMatrixFiltering over all unique
   * tentatives, Tentatives1stRANSAC (LORANSAC inliers), TrueMatch1stRANSAC (of those, the ones the ground truth confirms);
   * n_inliers = the verified list that is written out */
  int gt_true, gt_ransac_inliers, gt_true_of_ransac;
} mods_ladder_result;

int mods_view_schedule(const double *scale_set, int n_scales, const double *tilt_set, int n_tilts, double phi_base,
                       mods_view_par *prev, int *n_prev, int prev_cap, mods_view_par *out, int max_out);
int mods_imgrep_create(mods_ctx *ctx, int capacity, mods_imgrep **out);
void mods_imgrep_destroy(mods_imgrep *rep);
int mods_imgrep_clear(mods_imgrep *rep);
int mods_imgrep_count(const mods_imgrep *rep);
const mods_region *mods_imgrep_regions_dev(const mods_imgrep *rep);
int mods_imgrep_append_ctx(mods_imgrep *rep, mods_ctx *ctx, int img);      /* regions the context holds for image slot img */
int mods_imgrep_append_ctx_half(mods_imgrep *rep, mods_ctx *ctx, int img); /* their HalfRootSIFT twins */
int mods_imgrep_append_dev(mods_imgrep *rep, const mods_region *src_dev, int n);
int mods_imgrep_append_host(mods_imgrep *rep, const mods_region *src, int n);
int mods_imgrep_fetch(mods_imgrep *rep, int begin, int count, mods_region *out);
int mods_match_reps(mods_ctx *ctx, const mods_imgrep *q, int q_begin, int q_end, const mods_imgrep *t, double ratio,
                    double contradDist, int nn, mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out);
/* the k nearest trains of the bank's queries [q_begin, q_end): section B4, mods_match_knn */
int mods_match_knn_reps(mods_ctx *ctx, const mods_imgrep *q, int q_begin, int q_end, const mods_imgrep *t, int k, int *idx_out, int *d2_out);
/* img1_dev, img2_dev: dense fp32 images in HBM; the context needs max_w = max_h >= ceil(hypot(w, h)) of the larger image. */
int mods_match_ladder_dev(mods_ctx *ctx, const float *img1_dev, int w1, int h1, const float *img2_dev, int w2, int h2,
                          const mods_ladder_step *steps, int n_steps, int min_matches, const mods_pair_params *par,
                          mods_imgrep *rep1, mods_imgrep *rep2, mods_ladder_result *res, double *matches_out, int max_matches);

/* The same loop with several scale-space detectors per step (the [HessianAffine<i>] / [DoG<i>] / [HarrisAffine<i>] sections of the
 * iterations file next to each other, io_mods.cpp:457-492): steps[step * n_det + d] is detector d's section of that step
 * (n_tilts = n_scales = -1: none), dets[d] its parameter set, reps1[d] / reps2[d] its region banks.  Every detector has its own
 * view history and its own lists; a detector is matched in the steps that bring new views of it, lists that a step does not
 * touch keep their tentatives (fginn_ratio / fginn_ratio_half < 0: not named in [Matching<i>]; 0: named but not searched), and
 * the joint list is the bank's key order: HalfRootSIFT before RootSIFT, detectors in the order given - list them sorted by
 * name (CorrespondenceBank::MatchImgReps / GetCorresponcesVector, correspondencebank.cpp:114-148, 286-340). */
int mods_match_ladder_dets_dev(mods_ctx *ctx, const float *img1_dev, int w1, int h1, const float *img2_dev, int w2, int h2,
                               const mods_ladder_step *steps, const mods_hessaff_params *dets, int n_steps, int n_det, int min_matches,
                               const struct mods_pair_params *par, mods_imgrep **reps1, mods_imgrep **reps2, mods_ladder_result *res,
                               double *matches_out, int max_matches);

/* Grouped matching of a step ([Matching<i>] GroupDetectors / GroupDescriptors, CorrespondenceBank::MatchImgReps,
 * correspondencebank.cpp:245-285): the regions of the named detectors, joined in the order they are named, are searched as ONE
 * query and ONE train list per named descriptor, with the [Matching]-wide thresholds (matchRatio<Descriptor> /
 * matchDistance<Descriptor>, io_mods.cpp:448-452), in every step that names a group - whether or not the step brought new
 * views.  The result is the bank's list of the pseudo-detector "Group"; group_pos = the number of real detectors whose name
 * sorts before "Group" (its place in the joint list). */
typedef struct mods_ladder_group {
  int n_dets, dets[8];                /* GroupDetectors as indices into the detector array, in the order given; 0: no group */
  double fginn_ratio, fginn_ratio_half;        /* matchRatioRootSIFT / matchRatioHalfRootSIFT; < 0: descriptor not in GroupDescriptors */
  double dist_threshold, dist_threshold_half;  /* matchDistanceRootSIFT / matchDistanceHalfRootSIFT (> 0: MatchFLANNDistance replaces) */
} mods_ladder_group;
int mods_match_ladder_groups_dev(mods_ctx *ctx, const float *img1_dev, int w1, int h1, const float *img2_dev, int w2, int h2,
                                 const mods_ladder_step *steps, const mods_hessaff_params *dets, const mods_ladder_group *groups /* [n_steps] or NULL */,
                                 int group_pos, int n_steps, int n_det, int min_matches, const struct mods_pair_params *par,
                                 mods_imgrep **reps1, mods_imgrep **reps2, mods_ladder_result *res, double *matches_out, int max_matches);

/* ---- one hard pair on several GPUs of a node ------------------------------------------------------
 * The views of every step (ImageRepresentation::SynthDetectDescribeKeypoints' views loop, imagerepresentation.cpp:704-1099) are
 * sharded over the devices, largest first; the described regions travel in ONE all-gather per step (RCCL over xGMI, device
 * buffers; the one host process knows all counts, so nothing else is exchanged); every device searches its slice of the query
 * rows against all trains (CorrespondenceBank::MatchImgReps, correspondencebank.cpp:234-343) and the host of device 0 filters
 * duplicates and verifies.  Same result as mods_match_ladder_dev.  devices[]: HIP device ids; a device listed twice makes
 * the exchange use plain device copies (development on a one-GPU box).  The `mods` command line takes MODS_DEVICES=0,1,... */
typedef struct mods_multi mods_multi;
int mods_multi_create(const int *devices, int n, int w, int h, int rep_capacity, mods_multi **out);
void mods_multi_destroy(mods_multi *m);
int mods_multi_uses_rccl(const mods_multi *m);
mods_imgrep *mods_multi_bank(mods_multi *m, int image);   /* regions of image 1 (0) / 2 (1) after a run; owned by m */
mods_imgrep *mods_multi_bank_det(mods_multi *m, int image, int det);   /* the same for detector `det` of a several-detector run */
int mods_match_ladder_multi(mods_multi *m, const float *img1_host, int w1, int h1, const float *img2_host, int w2, int h2,
                            const mods_ladder_step *steps, int n_steps, int min_matches, const mods_pair_params *par,
                            mods_ladder_result *res, double *matches_out, int max_matches);
/* The whole step loop of mods_match_ladder_groups_dev on several GPUs: several detectors per step (steps[step * n_det + det],
 * dets[n_det]), HalfRootSIFT lists (a job's HalfRootSIFT twins travel behind its RootSIFT regions in the same all-gather), the
 * distance matcher, grouped matching (groups[n_steps] or NULL, group_pos).  Same result as on one GPU, field by field. */
int mods_match_ladder_groups_multi(mods_multi *m, const float *img1_host, int w1, int h1, const float *img2_host, int w2, int h2,
                                   const mods_ladder_step *steps, const mods_hessaff_params *dets, const mods_ladder_group *groups /* or NULL */,
                                   int group_pos, int n_steps, int n_det, int min_matches, const struct mods_pair_params *par,
                                   mods_ladder_result *res, double *matches_out, int max_matches);
/* queries [q_begin, q_end) of bank q against bank t with either matcher: distance > 0 runs MatchFLANNDistance (Hamming threshold)
 * instead of the FGINN search; tentative indices refer to the full lists */
int mods_match_reps_any(mods_ctx *ctx, const mods_imgrep *q, int q_begin, int q_end, const mods_imgrep *t, double ratio, double contradDist,
                        int nn, double distance, mods_tentative *out, double *u6_out, double *laf_out, int max_out, int *n_out);
int mods_regions_half_copy_dev(mods_ctx *ctx, int img, mods_region *dst_dev, int n);   /* HalfRootSIFT twins of slot img, D2D */
/* host logic of the sharding (no device needed): owner[i] = device of view job i with area areas[i] */
int mods_multi_assign(const double *areas, int n, int n_dev, int *owner);

/* Pre-extracted mode (mods.cpp:196-229, 288-383): the banks were filled by the caller (mods_imgrep_append_host, e.g. from the
 * k1 / k2 files of an earlier run); one matching + duplicate filtering + verification pass, no detection. */
int mods_match_verify_reps(mods_ctx *ctx, mods_imgrep *rep1, mods_imgrep *rep2, double fginn_ratio, const mods_pair_params *par,
                           mods_ladder_result *res, double *matches_out, int max_matches);
/* The rematch step under a verified H ("homography views" above): img1_dev, img2_dev dense fp32 in HBM; the context must hold
 * both images and both views (max_w max_h >= w1 h1 and >= w2 h2). */
int mods_rematch_under_h_dev(mods_ctx *ctx, const float *img1_dev, int w1, int h1, const float *img2_dev, int w2, int h2, const double *H,
                             int both, double initSigma, int doBlur, const mods_pair_params *par, mods_imgrep *rep1, mods_imgrep *rep2,
                             double fginn_ratio, mods_ladder_result *res, double *matches_out, int max_matches);
/* plain device-memory helpers for callers that do not link a HIP runtime themselves (the mods CLI) */
int mods_host_alloc(size_t bytes, void **out);     /* pinned host memory */
int mods_host_free(void *p);
int mods_dev_alloc(size_t bytes, void **out);
int mods_dev_free(void *p);
/* Both copies are complete when the call returns.  They run on a NON-BLOCKING stream of the calling thread on the device the buffer
 * lives on: they are ordered after nothing else - not after work in flight on a context's stream, on the legacy stream or on an
 * application's own streams.  A buffer that some stream is still writing (or reading, for an upload) has to be waited for first
 * (mods_ctx_sync, or the application's own synchronisation); every entry point of this library that produces a buffer has returned
 * only after its work was complete, unless its comment says otherwise. */
int mods_dev_upload(void *dst_dev, const void *src_host, size_t bytes);
int mods_dev_download(void *dst_host, const void *src_dev, size_t bytes);

/* ---- CLAHE -------------------------------------------------------------------------------------------
 * Replaces the [Matching] doCLAHE branch of mods.cpp:133-189: createCLAHE() with setClipLimit(4) on an 8 x 8 tile grid, applied to
 * the 8-bit grey images before the ImageRepresentation converts them to float.  The arithmetic restates OpenCV's CPU clahe.cpp
 * for CV_8UC1: tile histograms (the image padded with BORDER_REFLECT_101 when the grid does not divide it),
 * clip limit max((int)(clip_limit * tile pixels / 256), 1) (clip_limit <= 0: no clipping), redistribution, LUT, bilinear blend of
 * the four neighbouring tiles' LUTs in float32.  Images are 8-bit only, as OpenCV's CLAHE takes them. */
typedef struct mods_clahe_params { double clip_limit; int tiles_x, tiles_y; } mods_clahe_params;   /* mods.cpp: 4, 8, 8 */
/* n_img images [n_img][h][src_stride] (bytes) in HBM -> [n_img][h][dst_stride] u8 (dst_f32 = 0; may be src itself, same stride) or
 * fp32 (dst_f32 != 0; dst_stride in floats) in HBM.  Tiles in [1, 64] each way; w * h at most the context's max_w * max_h, any
 * n_img.  Runs on the context's stream and is complete on return.  Arguments are checked before any device call (MODS_E_ARG). */
int mods_clahe_dev(mods_ctx *ctx, const unsigned char *src_dev, int n_img, int w, int h, int src_stride,
                   const mods_clahe_params *par, void *dst_dev, int dst_stride, int dst_f32);
/* one contiguous w x h image, host in, host out (dst_host may be src_host) */
int mods_clahe(mods_ctx *ctx, const unsigned char *src_host, int w, int h, const mods_clahe_params *par, unsigned char *dst_host);

/* ---- pair pipeline ----------------------------------------------------------------------------------
 * Throughput form of the same path: `gpu_workers` threads (one context each) run detect/describe/match
 * while `verify_workers` threads run duplicate filtering + LO-RANSAC of earlier pairs (mods.cpp overlaps
 * its two images with OpenMP tasks, mods.cpp:234-251; here the overlap is across pairs).  Results are
 * returned in submission order and are identical to mods_match_pair_dev's.
 * Host cost: ~1.0 ms of process CPU per 1080p pair: the pipeline's threads wait on recorded events with sleeping
 * polls (MODS_SYNC=spin | sleep:<us> changes that), and its workers' contexts keep ONE stream and eager launches
 * (MODS_PIPELINE_STREAMS=2: side stream for the small octaves + hipGraph replay per worker - same results, same rate, one more
 * busy core: the runtime's own thread spins while a dependency between two streams is pending). */
typedef struct mods_pipeline mods_pipeline;
int mods_pipeline_create(int device, int w, int h, const mods_pair_params *par, int gpu_workers, int verify_workers,
                         mods_pipeline **out);
/* pairs_per_batch > 1: a GPU worker takes up to that many queued pairs through detect/describe as one batch of
 * launches (same results; larger launches, fewer of them per pair) */
int mods_pipeline_create_ex(int device, int w, int h, const mods_pair_params *par, int gpu_workers, int verify_workers,
                            int pairs_per_batch, mods_pipeline **out);
/* the same with CLAHE (mods_clahe_params, e.g. {4, 8, 8}) in front of detection: 8-bit submissions (mods_pipeline_submit_host_u8)
 * are equalised on the GPU on their way to fp32, one LUT and one apply launch per batch; fp32 submissions are refused (MODS_E_ARG).
 * clahe = NULL: mods_pipeline_create_ex */
int mods_pipeline_create_clahe(int device, int w, int h, const mods_pair_params *par, int gpu_workers, int verify_workers,
                               int pairs_per_batch, const mods_clahe_params *clahe, mods_pipeline **out);
int mods_pipeline_capacity(const mods_pipeline *p);    /* pairs that may be in flight before submit blocks */
/* HIP-event timing of the workers' contexts (sums over them); enable/read while nothing is in flight */
int mods_pipeline_timing_enable(mods_pipeline *p, int stage_mask);
int mods_pipeline_timing_read(mods_pipeline *p, int stage, double *total_ms, int *launches, double *bytes);
long mods_pipeline_u8_source_calls(mods_pipeline *p);   /* sum of mods_ctx_u8_source_calls over the GPU workers' contexts */
/* mods_ctx_u8_kernels on every GPU worker's context, before the first submit (later: MODS_E_ARG), and the sum of their
   mods_ctx_u8_strip_calls */
int mods_pipeline_u8_kernels(mods_pipeline *p, int mask);   /* on every worker's context; before the first submit */
long mods_pipeline_u8_strip_calls(mods_pipeline *p);
long mods_pipeline_graph_replays(mods_pipeline *p);   /* batches whose detect + describe chain was a graph replay (mods_ctx_graphs) */
/* CPU seconds the GPU workers' / the verify workers' own threads have spent inside their stages since the last reset (thread clocks;
   the RANSAC task pool's helper threads are not in them).  What a pair costs the host: needed to size ranks per node. */
int mods_pipeline_cpu_seconds(mods_pipeline *p, double *gpu_workers_s, double *verify_workers_s, int reset);
int mods_pipeline_submit(mods_pipeline *p, const float *img_dev, long tag);
/* the pair in HOST memory, [2][h][w] fp32 or 8-bit grey (what cv::imread hands to the ImageRepresentation constructor,
 * mods.cpp:111-121, 184-185): uploaded on the worker's stream (asynchronously when the memory is pinned, see
 * mods_host_alloc); the memory must stay valid until the pair's result has been fetched */
int mods_pipeline_submit_host(mods_pipeline *p, const float *img_host, long tag);
int mods_pipeline_submit_host_u8(mods_pipeline *p, const unsigned char *img_host, long tag);
/* the 8-bit pair with its detection masks (see mods_ctx_detection_mask): mask_host = two stacked masks of the images' geometry
 * ([2][h][w] bytes, valid as long as the images), or null for an unmasked pair - a batch may mix both.  The masks are staged and
 * uploaded with the images; the pair's result is what mods_match_pair_dev gives on a context with the same two masks set. */
int mods_pipeline_submit_host_u8_masked(mods_pipeline *p, const unsigned char *img_host, const unsigned char *mask_host, long tag);
int mods_pipeline_next(mods_pipeline *p, mods_pair_result *res, long *tag);
/* the same, and the verified matches of the pair (rows x1 y1 x2 y2, the order of mods_match_pair_dev's matches_out): the first
 * min(res->n_inliers, max_matches) rows are written */
int mods_pipeline_next_matches(mods_pipeline *p, mods_pair_result *res, long *tag, double *matches_out, int max_matches);
void mods_pipeline_destroy(mods_pipeline *p);

/* ---- guided matching under a verified model ----------------------------------------------------------
 * No counterpart in the reference.  After a verification has produced a model (mods_pair_result.H / mods_ladder_result.H), every
 * query region is matched again, but only against the trains that the model allows ("the gate"), which recovers the
 * correspondences the global FGINN test at ratio 0.8 over all trains discards.  csrc/guided.hip.
 *
 * All geometry is fp64, one rounding per operation, in the order written; a sum of three terms is (a*b + c*d) + e; r2 = radius *
 * radius, rho2 = ratio * ratio.  Mij = entry (i, j) of the model: model_type 0, H row-major image 1 -> image 2, Mij = model[3*i + j];
 * model_type 1, F as degensac stores it (x2^T F x1 = 0), Mij = model[3*j + i].
 *   Homography gate.  Hinv = adjugate(H) * (1 / det H), the closed form of cv::invert for 3 x 3.  Per query (x1, y1):
 *     X = (M00*x1 + M01*y1) + M02, Y = (M10*x1 + M11*y1) + M12, W = (M20*x1 + M21*y1) + M22, px = X / W, py = Y / W; per train
 *     (x2, y2): (bx, by) the same with Hinv.  A pair passes when (px-x2)*(px-x2) + (py-y2)*(py-y2) <= r2 and
 *     (bx-x1)*(bx-x1) + (by-y1)*(by-y1) <= r2.  Comparisons with NaN or infinity fail (W = 0 gates nothing).
 *   Epipolar gate.  Per query a = (M00*x1 + M01*y1) + M02, b = (M10*x1 + M11*y1) + M12, c0 = (M20*x1 + M21*y1) + M22,
 *     gq = r2 * (a*a + b*b); per train a' = (M00*x2 + M10*y2) + M20, b' = (M01*x2 + M11*y2) + M21, gt = r2 * (a'*a' + b'*b');
 *     per pair e = (a*x2 + b*y2) + c0: passes when e*e <= gq and e*e <= gt (within `radius` of the epipolar line in both images).
 *   Distance d(q, t) = sum over the 128 descriptor bytes of (dq[i] - dt[i])^2, an exact integer.
 *   Per query: (d1, t1) = the smallest (d, t) over the gated trains (ties: lower train index); (d2, t_bad) = the smallest (d, t)
 *     over the gated trains t != t1 whose centre lies farther than contradDist from t1's: (x2-x2')^2 + (y2-y2')^2 > contradDist^2.
 *     Accepted when (max_dist == 0 or d1 <= max_dist) and (no t_bad, or (double)d1 < rho2 * (double)d2).
 *   one_to_one: of the accepted queries that chose the same train only the one with the smallest (d1, q) stays; the others are
 *     dropped, not re-assigned.
 *   Output in query order: q, t = t1, t_bad (-1: none), t_2nd = -1, d1, d2 (0: none), d2nd = 0, ratio = sqrt((double)d1 /
 *     (double)d2) (0: none); u6 / laf as mods_match_fginn lays them out.  The result does not depend on launch geometry.
 * MODS_E_ARG with a mods_last_error text, before any device call: a null pointer, model_type not 0 or 1, a model entry that is
 * not finite, a homography whose determinant is 0 (or not finite), radius not finite or <= 0, ratio outside (0, 1], contradDist
 * negative or not finite, max_dist < 0, a negative count.  A result longer than max_out: as mods_match_fginn, *n_out = the full
 * length, MODS_E_CAPACITY, and nothing is copied.  The search has buffers of its own: it leaves the matcher's "last search" alone. */
typedef struct mods_guided_params {
  int model_type;        /* 0 homography, 1 fundamental matrix */
  double model[9];       /* as mods_pair_result.H / mods_ladder_result.H deliver it */
  double radius;         /* px */
  double ratio;          /* (0, 1]; 1 = only the strict d1 < d2 test */
  double contradDist;    /* px, [Matching] contradDist */
  int max_dist;          /* squared L2 cap, 0 = none */
  int one_to_one;
} mods_guided_params;
int mods_match_guided(mods_ctx *ctx, const mods_region *q, int n_q, const mods_region *t, int n_t,
                      const mods_guided_params *par, mods_tentative *out, double *u6_out, double *laf_out,
                      int max_out, int *n_out);                       /* host lists, the testing seam */
int mods_match_guided_reps(mods_ctx *ctx, const mods_imgrep *q, const mods_imgrep *t,
                           const mods_guided_params *par, mods_tentative *out, double *u6_out, double *laf_out,
                           int max_out, int *n_out);                  /* HBM-resident banks */

/* ---- ground-truth overlap matching of two region lists -------------------------------------------------
 * Which regions of image 1 have a geometric counterpart in image 2 under a known homography, and how repeatable the detector is on
 * the pair.  The reference reads [OverlapMatching] doOverlapMatch / overlapError (io_mods.cpp:685-687) and prints "Overlap
 * matches with E <" (mods.cpp:522-523); the error is the linearised one of ellipseOverlapH / ellipseOverlapHPrep
 * (matching/matching.hpp:170-253) with linH (synth-detection.cpp:1498) and rectifyAffineTransformationUpIsUp
 * (detectors/helpers.cpp:401), not the area of intersection of Mikolajczyk et al. (that measure: mods_match_overlap_area below).
 * No descriptor takes part.  csrc/overlap.hip.
 *
 * fp64 throughout, one rounding per operation as written; sqrt and / are the correctly rounded ones.  H is row-major, image 1 ->
 * image 2, as mods_ransac_params.gtH holds it; Hi = H[i].  A region is (x, y, s, a11, a12, a21, a22); k = 3.0.
 *   Query record (a region of image 1):
 *     X = (H0*x + H1*y) + H2, Y = (H3*x + H4*y) + H5, den = (H6*x + H7*y) + H8, px = X/den, py = Y/den;
 *     den2 = den*den, n1 = X/den2, n2 = Y/den2;
 *     L11 = H0/den - n1*H6, L12 = H1/den - n1*H7, L21 = H3/den - n2*H6, L22 = H4/den - n2*H7   (linH);
 *     ks = 3.0*s, Bij = ks*aij;
 *     C11 = L11*B11 + L12*B21, C12 = L11*B12 + L12*B22, C21 = L21*B11 + L22*B21, C22 = L21*B12 + L22*B22.
 *   Train record (a region (x2, y2, ...) of image 2):
 *     ks = 3.0*s, Mij = ks*aij, d = 1.0/(M11*M22 - M12*M21), I11 = M22*d, I12 = -(M12*d), I21 = -(M21*d), I22 = M11*d.
 *   Pair (q, t):
 *     dx = px - x2, dy = py - y2, u = I11*dx + I12*dy, v = I21*dx + I22*dy, dist = u*u + v*v;
 *     G11 = I11*C11 + I12*C21, G12 = I11*C12 + I12*C22, G21 = I21*C11 + I22*C21, G22 = I21*C12 + I22*C22;
 *     with oriented == 0, G is first replaced by its up-is-up form, so that an in-plane rotation of the frame does not count:
 *       det = sqrt(fabs(G11*G22 - G12*G21)), r = sqrt(G12*G12 + G11*G11),
 *       (G11, G12, G21, G22) <- (r/det, 0, (G22*G12 + G21*G11)/(r*det), det/r);
 *     diff = 0.5*((((1-G11)*(1-G11) + G12*G12) + G21*G21) + (1-G22)*(1-G22)), E = diff + dist.
 *   This restates ellipseOverlapH with one deliberate difference: the centre offset is mapped once, I*(p - x2), where the
 *   reference maps the two absolute positions and subtracts.  cv::invert / cv::gemm cannot be pinned without OpenCV, so parity
 *   with the reference is UNPINNED (as for CLAHE): the contract is this restatement.
 *   Per query: (E1, t1) = the smallest (E, t) over the trains that take part (ties: the lower train index); accepted when
 *     E1 < max_error (strict).  Every comparison with NaN fails: a singular train frame, den == 0 and non-finite input never match
 *     and never fault.  (diff >= 0, so the shape term may be skipped whenever dist >= max_error; that is not observable.)
 *   one_to_one: of the accepted queries that chose the same train only the one with the smallest (E1, q) stays; the others are
 *     dropped, not re-assigned - the rule of mods_match_guided.
 *   Common area: when w1, h1, w2, h2 are all > 0, a query takes part when 0 < px < w2 and 0 < py < h2, a train when its centre
 *     sent back with Hinv = adjugate(H) * (1 / det H) (as the guided gate does: (bx, by) by the formulas of (px, py)) satisfies
 *     0 < bx < w1 and 0 < by < h1.  With any of the four sizes 0 every region takes part and the two common counts are the list
 *     lengths.
 *   Output in query order; counts: n_q_common / n_t_common = the regions of either list that take part, n_matches = *n_out,
 *     repeatability = (double)n_matches / (double)min(n_q_common, n_t_common), 0 when that minimum is 0.  The customary
 *     repeatability figure is the one with one_to_one = 1 (otherwise several queries may count one train).  The result does not
 *     depend on launch geometry, train splits or the order of atomics.
 * MODS_E_ARG with a mods_last_error text starting "match_overlap: ", before the context is looked at and before any device call: a
 * null pointer (a list may be null when its count is 0, `out` when max_out is 0), a negative count, an H entry that is not finite,
 * det H zero or not finite, max_error not finite or <= 0, oriented or one_to_one other than 0 / 1, a negative image size.  A result
 * longer than max_out: as mods_match_guided, *n_out = the full length, MODS_E_CAPACITY, and nothing is copied (the counts are
 * filled).  The search has buffers of its own: it leaves the matcher's "last search" and the guided buffers alone.
 * mods_ctx_overlap_splits: the number of train splits of the sweep (0 = chosen from the list lengths, the default); a testing knob,
 * the result does not depend on it. */
typedef struct mods_overlap_params {
  double H[9];
  double max_error;      /* [OverlapMatching] overlapError, 0.09 in the reference's configurations */
  int oriented;          /* 1: the frames' orientations count; 0: up-is-up form */
  int one_to_one;
  int w1, h1, w2, h2;    /* image sizes for the common-area test; any 0: no test */
} mods_overlap_params;
typedef struct mods_overlap_match { int q, t; double E, dist, diff; } mods_overlap_match;
typedef struct mods_overlap_counts { int n_q_common, n_t_common, n_matches; double repeatability; } mods_overlap_counts;
int mods_match_overlap(mods_ctx *ctx, const mods_region *q, int n_q, const mods_region *t, int n_t,
                       const mods_overlap_params *par, mods_overlap_match *out, int max_out, int *n_out,
                       mods_overlap_counts *counts);                  /* host lists, the testing seam */
int mods_match_overlap_reps(mods_ctx *ctx, const mods_imgrep *q, const mods_imgrep *t,
                            const mods_overlap_params *par, mods_overlap_match *out, int max_out, int *n_out,
                            mods_overlap_counts *counts);             /* HBM-resident banks */
int mods_ctx_overlap_splits(mods_ctx *ctx, int splits);
/* Launch geometry of the sweep of a search of two region lists: out = {query blocks, train splits, 256-train tiles per split}.
 * search 0: mods_match_guided; 1: mods_match_overlap and mods_match_overlap_area, for which forced_splits is what
 * mods_ctx_overlap_splits was given (the guided search has no such knob and ignores it).  Host arithmetic only (no device, no
 * launch); the lists may be empty.  A null out, another search or a negative number: MODS_E_ARG.  The result of a search does not
 * depend on it, its speed does; tests pin the choice with it. */
int mods_list_search_grid(int search, int n_q, int n_t, int forced_splits, int out[3]);

/* ---- area-overlap matching of two region lists (the repeatability measure of Mikolajczyk et al., IJCV 2005) --------------
 * The same question as mods_match_overlap, scored with the customary measure: eps = 1 - |A n B| / |A u B| of the two ellipses, the
 * pair first rescaled so that the image-1 region has the area of a circle of radius 30, accepted below 0.4, regions assigned one
 * to one greedily by increasing error.  The areas are counted on the integer lattice, so the contract is exact integers.  No
 * counterpart in the reference; VGG's c_eoverlap is not in its tree, so parity with it is UNPINNED: the contract is this
 * restatement.  csrc/overlap_area.hip.
 *
 * The arithmetic regime of the overlap contract above: fp64 throughout, one rounding per operation in the order written; sqrt and /
 * are the correctly rounded ones; every comparison with NaN fails.  min(a, b) is a < b ? a : b, max(a, b) is a > b ? a : b.
 *   Query record: px, py, C11 .. C22 exactly as above (projected centre, C = linH(x) * (3.0*s) * A).
 *   Train record: x2, y2, Mij = (3.0*s)*aij.
 *   Common area: the test and its counts are the rule above, unchanged.
 *   Pair (q, t), set-up:
 *     detC = C11*C22 - C12*C21, f = 30.0 / sqrt(fabs(detC)), Qij = f*Cij, Tij = f*Mij, dx = f*(px - x2), dy = f*(py - y2);
 *     qex = sqrt(Q11*Q11 + Q12*Q12), qey = sqrt(Q21*Q21 + Q22*Q22), tex and tey the same from T;
 *     at = fabs(T11*T22 - T12*T21), g = 0.9*(1.0 - max_error);
 *     x0 = floor(min(dx - qex, -tex)), x1 = ceil(max(dx + qex, tex)), y0 = floor(min(dy - qey, -tey)), y1 = ceil(max(dy + qey, tey)).
 *   The pair is evaluated only when all of these hold:
 *     at >= g*900.0, 900.0 >= g*at, fabs(dx) <= qex + tex, fabs(dy) <= qey + tey,
 *     -x0 <= 256.0, x1 <= 256.0, -y0 <= 256.0, y1 <= 256.0.
 *   The area gate only removes pairs whose analytic error is at least max_error, with 10 % of slack; the box gate removes disjoint
 *   pairs; the cap bounds the work - a normalised ellipse longer than 256 matches nothing.  A pair that is not evaluated never
 *   matches.
 *   Evaluated pair:
 *     dq = 1.0/(Q11*Q22 - Q12*Q21), QI11 = Q22*dq, QI12 = -(Q12*dq), QI21 = -(Q21*dq), QI22 = Q11*dq; TI the same from T.
 *     For every integer lattice point (X, Y), x0 <= X <= x1, y0 <= Y <= y1 (the origin is the train's centre):
 *       a = X - dx, b = Y - dy, u = QI11*a + QI12*b, v = QI21*a + QI22*b, inQ = (u*u + v*v <= 1.0);
 *       u2 = TI11*X + TI12*Y, v2 = TI21*X + TI22*Y, inT = (u2*u2 + v2*v2 <= 1.0).
 *     n_q_px, n_t_px, n_both count inQ, inT and both - plain integers, so no summation order exists.
 *     uni = n_q_px + n_t_px - n_both; with uni == 0 the pair does not match, otherwise E = 1.0 - (double)n_both / (double)uni.
 *     Every lattice point is decided by the expression as written; an implementation may skip points only where it has proved in
 *     the same arithmetic that the expression is false (this one skips none).
 *   Acceptance: E < max_error (strict).
 *   Assignment, one_to_one:
 *     0: per query the smallest (E, t).
 *     1: the rule of mods_match_overlap - of the queries that chose one train the smallest (E, q) stays, the others are dropped.
 *     2: greedy, the customary protocol - all accepted pairs sorted by (E, q, t) and taken in that order when neither region is
 *        used yet.  The device produces the compact list of accepted pairs; the sort and the greedy pass over that short list
 *        run on the host.
 *   Output in query order in every mode; counts and repeatability as mods_overlap_counts above.  The result does not depend on
 *   launch geometry, train splits or the arrival order of atomics.
 * MODS_E_ARG with a mods_last_error text starting "match_overlap_area: ", before the context is looked at and before any device
 * call: the refusals of mods_match_overlap, and max_error outside (0, 1] or one_to_one outside 0 .. 2.  A result longer than
 * max_out: *n_out = the full length, MODS_E_CAPACITY, the counts are filled and nothing is copied.  The search has buffers of its
 * own: it leaves the matcher's "last search", the guided and the linearised overlap buffers alone.  mods_ctx_overlap_splits also
 * sets the train splits of its gate sweeps. */
typedef struct mods_overlap_area_params {
  double H[9];
  double max_error;      /* 0.4 is the customary bound */
  int one_to_one;        /* 0, 1, 2 */
  int w1, h1, w2, h2;    /* image sizes for the common-area test; any 0: no test */
} mods_overlap_area_params;
typedef struct mods_overlap_area_match { int q, t; double E; int n_q_px, n_t_px, n_both, pad; } mods_overlap_area_match;
int mods_match_overlap_area(mods_ctx *ctx, const mods_region *q, int n_q, const mods_region *t, int n_t,
                            const mods_overlap_area_params *par, mods_overlap_area_match *out, int max_out, int *n_out,
                            mods_overlap_counts *counts);             /* host lists, the testing seam */
int mods_match_overlap_area_reps(mods_ctx *ctx, const mods_imgrep *q, const mods_imgrep *t,
                                 const mods_overlap_area_params *par, mods_overlap_area_match *out, int max_out, int *n_out,
                                 mods_overlap_counts *counts);        /* HBM-resident banks */

/* ---- mutual nearest-neighbour check of the FGINN matcher ----------------------------------------------
 * No counterpart in the reference, whose matcher is one-directional: a query's tentative goes to the verification even when its
 * train is much closer to another query.  csrc/mutual.hip.
 *
 * A forward FGINN search has produced its tentative list, as mods_match_fginn specifies.  For a tentative (q, t):
 *   d(a, t) = the exact integer squared L2 distance over the 128 descriptor bytes; d1 = d(q, t); a rival is any query r != q of
 *   the same query list, d_r = d(r, t); centres are the x, y doubles of mods_region.
 *   Mode 0: off (the default), everything is as without this block.
 *   Mode 1, mutual nearest neighbour: the tentative is dropped when some rival has d_r < d1, or d_r == d1 and r < q - q must be the
 *     first query in (d, index) order for train t.
 *   Mode 2, mode 1 plus the ratio test backwards: the tentative is also dropped when some rival with
 *     (xr-xq)*(xr-xq) + (yr-yq)*(yr-yq) > contradDist*contradDist (fp64, as written) fails the forward search's own predicate with
 *     the roles swapped, (double)((float)d1 / (float)d_r) <= ratio*ratio, taken with the search's own ratio and contradDist.  A
 *     quotient that is NaN or infinite fails (d_r == 0): two far-apart queries with the descriptor of t are both dropped in mode 2;
 *     in mode 1 the one with the lower index survives.
 *   Survivors stay in query order, every field of mods_tentative, u6 and laf exactly as the forward search wrote it; nothing is
 *   re-assigned to a second choice.  The result does not depend on launch geometry or on the grouping of searches.
 * Every FGINN search of the context honours the mode: mods_match_fginn, mods_match_dev, mods_match_reps[_any] over the whole query
 * list, mods_match_pair_dev, mods_match_verify_reps, the single-GPU ladder entry points (RootSIFT and HalfRootSIFT lists alike) and a
 * pipeline's grouped searches; n_tentatives in their results is the count after the check, and the "last search" the fetch entry
 * points read is the checked list.  The Hamming distance matcher (mods_match_distance, a ladder step's dist_threshold) is never
 * checked.  The check needs the whole query list: mods_match_reps[_any] with a proper slice (q_begin > 0 or q_end < the bank's
 * count) while the mode is not 0 answer MODS_E_ARG with a mods_last_error text, before any device call.  The multi-GPU ladder
 * (mods_match_ladder_multi) shards the queries and has no switch: its searches are unchecked.
 * mods_ctx_match_mutual: mode 0 / 1 / 2, anything else MODS_E_ARG (checked before ctx).  mods_match_mutual_counts: of the last single
 * search of the context, the length of the forward list and what the check kept (equal when that search was not checked); waits for
 * the context's stream.  mods_pipeline_match_mutual: the mode of every search of the pipeline, before the first submit - later:
 * MODS_E_ARG. */
int mods_ctx_match_mutual(mods_ctx *ctx, int mode);
int mods_match_mutual_counts(mods_ctx *ctx, int *n_forward, int *n_kept);
int mods_pipeline_match_mutual(mods_pipeline *p, int mode);

/* ---- distractor descriptor database of the FGINN ratio test --------------------------------------------
 * MatchFlannFGINNPlusDB (matching/matching.cpp:461-572, field d2byDB of matching.hpp:48), which the reference defines and never
 * calls: the FGINN walk plus a second opinion from a database B of unrelated descriptors.  csrc/distractor.hip; restated in
 * tests/distractor_ref.py.  Off by default: with no database attached every search is what it was, to the bit and to the launch.
 * With d(a, b) the exact integer squared L2 distance over the 128 descriptor bytes, quot(x, y) = (double)((float)x / (float)y)
 * (0/0 is NaN, x/0 is +inf), sq = ratio * ratio in fp64 and M >= 1 rows in B, for every tentative (q, t) of the forward search:
 *   d0 = d(q, t) (field d1), dj = the distance the tentative was emitted with (field d2), dDB = min over the rows b of B of d(q, b);
 *   rDB = quot(d0, dDB), r = quot(d0, dj), r' = (r < rDB) ? rDB : r   (std::max(ratio, ratioDB) of line 547: a NaN rDB leaves r);
 *   the tentative is dropped when !(r' <= sq) - that is rDB > sq; dDB = 0 with d0 > 0 drops it - and otherwise kept with
 *   ratio = sqrt(r') in fp64, every other field, u6 and laf as the forward search wrote them.
 * Survivors stay in query order, nothing is re-assigned.  dDB is a minimum of integers: nothing depends on order, splits or launch
 * geometry.  Parity with FLANN's tie order is unpinned, as for the matcher; nothing else is approximate.
 * The veto is part of the search: the mutual check (independent of it), the local affine filter, duplicate filtering and
 * verification see the vetoed list, n_tentatives and the "last search" fetch entry points report it.  Honoured by every FGINN search
 * of a context: mods_match_fginn, mods_match_dev, mods_match_reps[_any] (slices allowed: the test is per tentative),
 * mods_match_pair_dev, mods_match_verify_reps, mods_rematch_under_h_dev, the single-GPU ladder entry points and a pipeline's grouped
 * searches.  A context holds two slots: one database for whole descriptors (whatever fills `desc`) and one that the ladder's
 * HalfRootSIFT searches take; a search whose kind has no database runs unvetoed.  An empty database (M = 0) equals none.  The Hamming
 * matcher (mods_match_distance), mods_match_knn*, guided and overlap matching ignore the databases; the multi-GPU entry points
 * (mods_multi_*, mods_match_ladder_multi) have no switch: their searches are unvetoed.
 *
 * A mods_descdb is immutable, lives on one device and is shared by any number of contexts, pipelines and threads of that device, as
 * a mods_net is.  It is packed once at creation into what the distance kernels stream (int8 rows v - 128 in 32-row tiles of 4096
 * bytes, accumulator seeds, a parity word per tile; rows past the end zero); no search packs it again.  Capacity: 2^24 rows
 * (MODS_E_CAPACITY beyond).  References: the creator holds one, every context slot it is attached to holds one (released by
 * attaching something else, by null, or by mods_ctx_destroy).  mods_descdb_destroy gives up the creator's reference; the memory
 * is freed when the last reference goes, so destroying a database a live context uses is deferred, never refused.
 *   mods_descdb_create            from n host rows of 128 bytes (n = 0 allowed)
 *   mods_descdb_create_from_reps  from the descriptors of n_reps banks of ctx's device, in order
 *   mods_descdb_min_dist          dDB of n host descriptors (INT_MAX per row for M = 0)
 *   mods_filter_distractor        the veto on a host list, in place: tent/u6/laf of n tentatives whose q index the n_q regions q;
 *                                 d_db_out[n_out] (may be null) = dDB of the survivors
 *   mods_ctx_distractor_db        attaches (or, with null, detaches) the two slots
 *   mods_distractor_counts        of the last single search: the forward list's length (after a mutual check, before the veto) and
 *                                 what the veto kept; equal when that search was not vetoed.  Waits for the stream
 *   mods_distractor_fetch         dDB of that search's survivors, in list order (*n = 0 when it was not vetoed).  A vetoed batch of
 *                                 searches on the same context in between (a pipeline worker's batch of pairs) takes the
 *                                 scratch both calls read: after it they answer as for a search that was not vetoed, until the
 *                                 next single search
 *   mods_pipeline_distractor_db   the whole-descriptor slot of every worker's context, before the first submit (later: MODS_E_ARG)
 *   mods_descdb_grid              {query blocks, database splits, 32-row tiles per split} of the sweep of n_queries queries against m
 *                                 rows with a forced split count (0: the library chooses; trailing splits may be empty).  Host
 *                                 arithmetic only
 *   mods_ctx_descdb_splits        that forced count for a context: a testing knob, the result never depends on it
 * Refusals are MODS_E_ARG with a mods_last_error text, before any device call: null pointers, negative counts, a database of another
 * device, a tentative whose q is outside the list.  Timers: MODS_STAGE_DISTRACTOR, MODS_STAGE_DISTRACTOR_SWEEP. */
typedef struct mods_descdb mods_descdb;
int mods_descdb_create(int device, const uint8_t *desc_host, long n, mods_descdb **out);
int mods_descdb_create_from_reps(mods_ctx *ctx, const struct mods_imgrep *const *reps, int n_reps, mods_descdb **out);
long mods_descdb_count(const mods_descdb *db);
void mods_descdb_destroy(mods_descdb *db);
int mods_descdb_min_dist(mods_ctx *ctx, const mods_descdb *db, const uint8_t *desc_host, int n, int *d2_out);
int mods_filter_distractor(mods_ctx *ctx, const mods_descdb *db, const mods_region *q, int n_q, double ratio, mods_tentative *tent,
                           double *u6, double *laf, int n, int *d_db_out, int *n_out);
int mods_ctx_distractor_db(mods_ctx *ctx, const mods_descdb *full_or_null, const mods_descdb *half_or_null);
int mods_distractor_counts(mods_ctx *ctx, int *n_forward, int *n_kept);
int mods_distractor_fetch(mods_ctx *ctx, int *d_db_out, int max, int *n);
int mods_pipeline_distractor_db(mods_pipeline *p, const mods_descdb *full_or_null);
int mods_descdb_grid(long m, int n_queries, int forced_splits, int out[3]);
int mods_ctx_descdb_splits(mods_ctx *ctx, int splits);

/* ---- local affine consistency of neighbouring tentatives ----------------------------------------------
 * No counterpart in the reference, which uses the local affine frames of a tentative only in the LAF checks on RANSAC's result.
 * A correspondence of two affine-covariant regions predicts where its neighbours land, T = (s2 A2) (s1 A1)^-1; true
 * correspondences on a locally smooth surface confirm each other's predictions, wrong ones are confirmed by nobody (Schmid and
 * Mohr, PAMI 1997; Cavalli et al., AdaLAM, ECCV 2020).  csrc/local_affine.hip; restated in tests/local_affine_ref.py.  Off by default:
 * with it off every entry point launches what it launches without this section.  The defaults come from a CPU prototype on
 * synthetic homography scenes; the radius was then raised from 100 to 160 after graf1 / graf6 (profiles/local_affine_timing.txt): a
 * list must be dense enough for a true tentative to have minSupport true neighbours inside the radius.
 *
 * Input: laf[n][14] = x1 y1 a11 a12 a21 a22 s1 | x2 y2 b11 b12 b21 b22 s2 per tentative, as mods_match_fginn writes it.  All arithmetic
 * is fp64, one IEEE operation per written operation in the written order, no contraction; comparisons are written so that NaN fails.
 *   per tentative i:
 *     m00=s1*a11  m01=s1*a12  m10=s1*a21  m11=s1*a22        n00=s2*b11  n01=s2*b12  n10=s2*b21  n11=s2*b22
 *     det = m00*m11 - m01*m10
 *     i00 = m11/det   i01 = (-m01)/det   i10 = (-m10)/det   i11 = m00/det
 *     t00 = n00*i00 + n01*i10   t01 = n00*i01 + n01*i11   t10 = n10*i00 + n11*i10   t11 = n10*i01 + n11*i11
 *     dT  = t00*t11 - t01*t10
 *     valid_i = t00, t01, t10, t11, dT all finite and dT != 0
 *   per ordered pair (i, j), j != i, with R2=radius*radius, D2=minDist*minDist, A2=absTol*absTol, L2=relTol*relTol:
 *     dx = x1_j - x1_i   dy = y1_j - y1_i   r2 = dx*dx + dy*dy
 *     gx = x2_j - x2_i   gy = y2_j - y2_i   q2 = gx*gx + gy*gy
 *     nb(i,j) = r2 <= R2 && r2 >= D2 && q2 >= D2
 *     mx = t00_i*dx + t01_i*dy   my = t10_i*dx + t11_i*dy
 *     ex = gx - mx   ey = gy - my   e2 = ex*ex + ey*ey   m2 = mx*mx + my*my
 *     ok(i,j) = nb(i,j) && valid_i && e2 <= A2 + L2*m2
 *               && (areaTol == 0 || (valid_j && dT_i*dT_j > 0 && min(|dT_i|,|dT_j|)*areaTol >= max(|dT_i|,|dT_j|)))
 *   per tentative, as int32:
 *     neighbours_i = #{j : nb(i,j)}     support_i = #{j : ok(i,j)}     strong_i = support_i >= minSupport
 *     backed_j     = #{i : strong_i && ok(i,j)}
 *     keep_i = strong_i || (rescue && backed_i > 0) || (keepSparse && neighbours_i < minSupport)
 * Survivors stay in list order; every byte of mods_tentative, u6 and laf stays as it came in.  All outputs are integers and
 * booleans: the result does not depend on launch geometry, on the grouping of lists or on the order of the traversal.
 *
 * MODS_E_ARG with a mods_last_error text starting "local_affine: ", before any device call and before the context is looked at: null
 * parameters; radius not finite or <= 0; minDist, absTol, relTol or areaTol negative or NaN; minDist > radius; 0 < areaTol < 1;
 * minSupport < 1; rescue or keepSparse outside 0 / 1; n < 0; then a null ctx, n_out or (n > 0) list pointer.
 *
 * mods_filter_local_affine: host lists in and out, compacted in place as mods_duplicate_filter_gpu does; keep_out[n] (bytes 0 / 1),
 * neighbours_out[n], support_out[n], backed_out[n] are optional and indexed by input position.  n = 0 succeeds with no launch.  A
 * list of any length: the context's scratch grows to it.  One host wait before the final copy of the survivors.
 * mods_ctx_local_affine: a parameter set switches the filter on for the context, NULL switches it off.  While it is on, the list that
 * goes to the verification is filtered: with doBeforeRANSAC = 1 after DuplicateFiltering - wherever that ran, also where the device
 * filter hands the list to the host filter - otherwise directly after the search; in mods_match_pair_dev, mods_match_verify_reps,
 * the single-GPU ladder entry points (every step) and a pipeline's batches (the lists of a batch in one grouped set of launches),
 * also in ground-truth mode.  n_unique in their results is the count after the filter, n_tentatives is unchanged.
 * mods_verify_tentatives*, which take no context, are untouched; the multi-GPU ladder (mods_match_ladder_multi) has no switch and is
 * unfiltered, as it is unchecked by the mutual check.
 * mods_local_affine_counts: the length of the last list the filter saw on the context and what it kept.
 * mods_pipeline_local_affine: every GPU worker's context, before the first submit - later: MODS_E_ARG.
 * mods_local_affine_grid: the rows of a sweep block and the columns of an LDS tile (for tests at the tile boundaries). */
typedef struct mods_local_affine_params {
  double radius;     /* 160  px in image 1: j is a neighbour of i when minDist^2 <= |x1_j - x1_i|^2 <= radius^2 ...      */
  double minDist;    /* 3    ... and |x2_j - x2_i|^2 >= minDist^2 (several orientations / views of one region don't vote) */
  double absTol;     /* 4    px */
  double relTol;     /* 0.2  of the length of the mapped offset */
  double areaTol;    /* 2    largest ratio of |det T_i|, |det T_j|; 0: no test */
  int minSupport;    /* 3 */
  int rescue;        /* 1: also keep what a strong seed confirms */
  int keepSparse;    /* 1: keep tentatives with fewer than minSupport neighbours (cannot be judged) */
} mods_local_affine_params;
void mods_local_affine_defaults(mods_local_affine_params *par);
int mods_filter_local_affine(mods_ctx *ctx, mods_tentative *tent, double *u6, double *laf, int n, const mods_local_affine_params *par,
                             int *n_out, unsigned char *keep_out, int *neighbours_out, int *support_out, int *backed_out);
int mods_ctx_local_affine(mods_ctx *ctx, const mods_local_affine_params *par_or_null);
int mods_local_affine_counts(mods_ctx *ctx, int *n_in, int *n_kept);
int mods_pipeline_local_affine(mods_pipeline *p, const mods_local_affine_params *par_or_null);
void mods_local_affine_grid(int *rows, int *tile);

/* ---- domain-size pooling of the SIFT descriptor (DSP-SIFT) -------------------------------------------
 * Dong and Soatto, "Domain-size pooling in local descriptors: DSP-SIFT", CVPR 2015.  The reference reads [SIFTDescriptor] numScales /
 * startCoef / endCoef (io_mods.cpp:431-433, siftdesc.h:21-30) and never uses them; this is their contract here (restated in
 * tests/dsp_ref.py).  Off by default; with it off every entry point launches what it launches without this section.
 *   Coefficients   c_k = startCoef + k * ((endCoef - startCoef) / (K - 1)), k = 0 .. K-1, K = numScales; domain k is described at
 *                  mr_k = desc_mrSize * c_k (all in double).
 *   Patches        patch k of a region is what the unpooled extraction makes at desc_mrSize = mr_k: the same size rule and tiers,
 *                  samples outside the image are 0, photometric normalisation per patch when photoNorm is set.
 *   Histograms     h_k[128]: the raw histogram of patch k - before the HalfSIFT fold and before any normalisation.
 *   Pooling        pooled[i] = ((h_0[i] + h_1[i]) + h_2[i]) + ..., in double, in scale order; no division by K (the L2 normalisation
 *                  that follows removes the factor).
 *   Tail           unchanged, on `pooled`: the HalfSIFT fold when halfDesc asks for it, normalise / clip at maxBinValue /
 *                  renormalise, RootSIFT or plain SIFT, quantisation.
 *   Regions        every field of mods_region but the descriptor bytes - count and order included - is that of the unpooled call
 *                  (the border rule does not depend on desc_mrSize).
 * 2 <= numScales <= 8, 0 < startCoef < endCoef <= 4, finite; numScales 0 or 1 switches pooling off (the coefficients are then
 * ignored); anything else is MODS_E_ARG (checked before ctx).  With pooling on, a describe call with fastExtraction = 1, or on a
 * context with an external descriptor or a descriptor network, is MODS_E_ARG before anything is launched; external shape and
 * orientation hooks are compatible.  The pair, ladder, view, image-representation and verify entry points inherit the context's
 * setting; mods_multi does not (its contexts stay unpooled).  A recorded detect + describe graph (mods_ctx_graphs) is never
 * replayed across a change, and with pooling on the chain is issued eagerly.  After a pooled call mods_patches_fetch returns the
 * patches of the last domain.  The accumulators (1 KB per region slot of the batch) are reserved by the first pooled call.
 * mods_pipeline_domain_pooling: every GPU worker's context, before the first submit - later: MODS_E_ARG.
 * mods_test_sift_pooled: the pooled twin of mods_sift_patch - K (1 .. 8) host patches [K][ps][ps] of one region through the
 * accumulate and finish kernels; half != 0: out128 receives the HalfSIFT bytes (64 values, then 64 zeros). */
int mods_ctx_domain_pooling(mods_ctx *ctx, int numScales, double startCoef, double endCoef);
int mods_ctx_domain_pooling_get(const mods_ctx *ctx, int *numScales, double *startCoef, double *endCoef);
int mods_pipeline_domain_pooling(mods_pipeline *p, int numScales, double startCoef, double endCoef);
int mods_test_sift_pooled(mods_ctx *ctx, const float *patches, int K, int ps, int rootsift, int half, int photoNorm, double maxBinValue,
                          uint8_t *out128);

/* ---- spatial selection of a count-limited detector's regions (ANMS) --------------------------------------------
 * Brown, Szeliski and Winder, "Multi-image matching using multi-scale oriented patches", CVPR 2005: adaptive non-maximal
 * suppression.  The count modes (FixedRegNumber, RelativeRegNumber, the scaled regionsNumber of a ladder view) keep a prefix of
 * the list sorted by |response|; with the selection on they keep as many keys, the ones with the largest suppression radius.  No
 * counterpart in the reference: this is the contract (restated in tests/spatial_select_ref.py and held to the bit).  Off by
 * default; with it off every entry point launches what it launches without this section.
 *   Input        one image's exported keys K[0 .. n): |response| descending, ties in processing order - the list a call with the
 *                count unrestricted returns.  The index in that list is the only order used.  keep = min(n, regionsNumber of the
 *                view) for FixedRegNumber, floor((double)relativeRegionsNumber * n) for RelativeRegNumber, clamped to [0, n].
 *   Trivial      keep <= 0 or keep >= n: the result is the prefix cut's.
 *   Radius       xf = (float)K[i].x, yf = (float)K[i].y, a = fabsf((float)K[i].response) (lossless: the fields hold floats),
 *                c = (float)robustness:
 *                  r2[i] = min over j != i with fl32(c * a[j]) > a[i] of fl32(fl32(dx * dx) + fl32(dy * dy)),
 *                  dx = fl32(xf[i] - xf[j]), dy = fl32(yf[i] - yf[j]);  r2[i] = +inf when there is no such j.
 *                Every operation is rounded to fp32 on its own (no fused multiply-add).  0 <= c <= 1, so only a stronger key
 *                suppresses: c = 1 is plain ANMS, c = 0 suppresses nothing; c = 0.9 is the paper's value.
 *   Selection    the keep indices with the largest r2, ties to the smaller index: ascending order of the unique key
 *                ((uint64)~bits(r2) << 32) | i  (non-negative floats order like their bit patterns).
 *   Output       the selected keys in increasing index order - still |response| descending - and key_count = keep.  Orientation,
 *                description and everything behind them see that list.
 * mods_ctx_spatial_selection: mode 0 off, 1 on, 2 on for the calls it covers (below) and silently off for the others (what a
 * configuration with several detectors wants; the command line uses it); another mode, or a robustness outside [0, 1] or NaN, is
 * MODS_E_ARG (checked before ctx).  With mode 1 a detect call whose mode is FixedTh, RelativeTh or NotLessThanRegions, or whose
 * detectorType is MSER (it exports its own list), is MODS_E_ARG before anything is launched, the message naming the key.  Every
 * entry point that detects on the context inherits the setting: mods_detect_hessian_affine[_dev], mods_detect_describe_dev[_u8],
 * the view calls, the pair calls, the ladders of the context (whose views keep their scaled regionsNumber), the pipeline
 * (mods_pipeline_spatial_selection: every worker's context, before the first submit - later: MODS_E_ARG); mods_multi does not
 * (its contexts cut by response).  keep is computed on the device and no launch is sized by it, so a recorded detect + describe
 * graph (mods_ctx_graphs) holds the selection; it is never replayed across a change of the setting.  The launches are timed as
 * MODS_STAGE_SPATIAL_SELECT.
 * mods_test_spatial_select: n_img lists keys_host[n_img][max_n] (n[b] keys each, sorted as above; n_img <= the context's batch)
 * through the launches of a detect call with keep[b] as the count: out_idx[n_img][max_n] receives the selected indices, n_out[b]
 * their number.  The compacted lists are compared with the input keys of those indices; a difference is MODS_E_HIP. */
int mods_ctx_spatial_selection(mods_ctx *ctx, int mode, double robustness);
int mods_ctx_spatial_selection_get(const mods_ctx *ctx, int *mode, double *robustness);
int mods_pipeline_spatial_selection(mods_pipeline *p, int mode, double robustness);
int mods_pipeline_upscale_input(mods_pipeline *p, int mode);   /* mods_ctx_upscale_input of every worker, before the first submit */
int mods_test_spatial_select(mods_ctx *ctx, const mods_affkey *keys_host, int n_img, const int *n, int max_n, const int *keep,
                             double robustness, int *out_idx, int *n_out);

/* ---- match and region images: an RGB canvas in HBM and a tile rasteriser ---------------------------------------
 * The reference draws with OpenCV (DrawRegions / DrawMatches, matching.cpp:1046-1574, called at mods.cpp:452-505); OpenCV's
 * rasterisers are not pinned, so this is a contract of its own, restated in integers and fp64 in tests/draw_ref.py and held to
 * the byte.  A canvas is h x w x 3 bytes, R G B.  A pixel centre is an integer point.  A colour is 0xRRGGBB.
 *
 * Elements.  A draw call takes an ordered list; a later element (or polyline) is drawn over an earlier one; what lies outside the
 * canvas is not written.  All arithmetic below is in 64-bit integers.
 *   DISC  (ax, ay) centre, t radius >= 0: covers (x, y) iff (x-ax)^2 + (y-ay)^2 <= t^2.  Solid.  bx, by, group unused.
 *   LINE  (ax, ay) -> (bx, by), one pixel wide, 8-connected, solid.  The major axis is x when |dx| >= |dy|, else y; the endpoints are
 *         ordered so that the major delta D >= 0 (the image does not depend on the direction given).  D = 0: the single pixel.
 *         Else for each major coordinate m in [a_m, b_m] the pixel with minor coordinate a_n + floor((2 (m - a_m) d_n + D) / (2 D)).
 *   SEG   (ax, ay) -> (bx, by), thickness t (0 .. 255), anti-aliased.  A pixel has 4 x 4 subsamples at offsets -3, -1, 1, 3 eighths of
 *         a pixel from its centre.  In eighths: p = 8 (x, y) + offset, A = 8 a, B = 8 b, h = 4 t, d = B - A, L2 = d.d, w = p - A,
 *         s = w.d.  The subsample is inside iff  w.w <= h^2 when L2 = 0 or s <= 0;  |p - B|^2 <= h^2 when s >= L2;
 *         cross(w, d)^2 <= h^2 L2 otherwise (a capsule with round caps).  A maximal run of consecutive SEG elements with one group
 *         value and one colour is a polyline: c = the subsamples inside any of its capsules (a joint is not blended twice), and
 *         the pixel is blended once, per channel out = (dst (16 - c) + col c + 8) >> 4.
 * Dropping.  An element with a coordinate outside [-32767, 32767] is not drawn, nor is a SEG with |dx| or |dy| > 2047; when one
 * member of a polyline is dropped the whole polyline is.  n_dropped = the elements not drawn for these reasons: never silent.  An
 * unknown kind, a negative t, a SEG thicker than 255 or a DISC radius above 32767 is MODS_E_ARG.
 * The image does not depend on the launch geometry: a workgroup owns a 16 x 16 tile and walks the list in order, no atomics.
 *
 * mods_canvas_draw_regions builds the contours of regions [begin, begin + count) of a bank on the device: for k = 0 .. 21 the point
 *   ( floor((((3.0 s) a11) C[k] + ((3.0 s) a12) S[k]) + x) + dx),  floor((((3.0 s) a21) C[k] + ((3.0 s) a22) S[k]) + y) + dy) )
 * every product and sum rounded once, in that order, in fp64; a floor outside [-32767, 32767] (or NaN) drops the polyline.  A region
 * gives 22 points and 21 SEG of one group (its index in the call).  table = MODS_DRAW_TABLE_REGIONS: C[l] = cos(l pi / 10), S[l] =
 * sin(l pi / 10), l = 0 .. 21 (DrawRegions, matching.cpp:1061-1064); MODS_DRAW_TABLE_MATCHES: the same for l = 0 .. 20 and C[21] =
 * S[21] = 0, so the contour ends with a spoke to the centre (DrawMatches, :1172-1177).  The host computes the tables with libm
 * (l * M_PI / 10 as written) and hands them to the kernel by value.  The bank belongs to the canvas's context.
 * mods_canvas_regions_elems: the element list that call would draw (21 * count elements; a dropped polyline's members have kind
 * MODS_DRAW_NONE and coordinates 0), for tests.
 *
 * mods_draw_matches composes DrawMatches' two images from the verified frames laf14 (n rows x1 y1 a11 a12 a21 a22 s | the same of
 * image 2) and draws them; mods_draw_matches_elems returns the list of image `which` (0, 1) alone (host only).  colour1 = 0x0000ff,
 * colour2 = 0x00ff00, epipolar lines 0x00ffff (the reference's BGR scalars on its BGR images).  (int)v and floor(v) saturate: a value
 * that is NaN or outside [-40000, 40000] becomes 40000, which the drop rule then reports.  Host contours use the MATCHES table and
 * the expression above.  Every polyline has a group of its own.
 *   reproject_to_one_image = 0: out1 = white (w1 + w2 + 20) x max(h1, h2) with image 1 at (0, 0) and image 2 at (w1 + 20, 0); out2 =
 *     white max(w1, w2) x (h1 + h2 + 20) with image 2 at (0, h1 + 20).  With (ox, oy) = image 2's place: unless draw_only_centers,
 *     per match the contour of region 1 (thickness r1) and of region 2 at (ox, oy) (r2), both colour2; then per match DISC((int)x1,
 *     (int)y1, r1 + 2) and DISC((int)((double)ox + x2), (int)((double)oy + y2), r1 + 2) in colour1, with draw_epipolar_lines the two
 *     epipolar LINEs, and the LINE from the second centre to the first in colour2.
 *     Epipolar lines (matching.cpp:156-169, 1514-1559), M = F: for a point pt = (px, py, 1) and a matrix G, l_j = (px G[j] + py G[3 + j])
 *     + G[6 + j], xc = (-l_2) / l_0, b = (-l_2) / l_1, k = (0 - b) / (xc - 0).  (k, b) from (M, centre 2) gives the line of image 1,
 *     from (M transposed, centre 1) that of image 2; line 1 runs (0, (int)b) -> (w1, (int)(k w1 + b)) clipped to image 1's rectangle,
 *     line 2 (ox, (int)b2 + oy) -> (ox + w2, (int)(k2 w2 + b2) + oy) clipped to image 2's.  Clipping: when all four coordinates are
 *     within +-32767 the line's pixels (rule above) inside the rectangle are found; none: no element; else the LINE from the first to
 *     the last of them in major order.  Otherwise the LINE is emitted unclipped and the draw call drops and counts it.
 *   reproject_to_one_image = 1, M = H (image 1 -> image 2), Hinv = the adjugate times the reciprocal of the determinant:
 *       d = H0 (H4 H8 - H5 H7) - H1 (H3 H8 - H5 H6) + H2 (H3 H7 - H4 H6), r = 1 / d,
 *       Hinv = r * [H4 H8 - H5 H7, H2 H7 - H1 H8, H1 H5 - H2 H4 | H5 H6 - H3 H8, H0 H8 - H2 H6, H2 H3 - H0 H5 |
 *                   H3 H7 - H4 H6, H1 H6 - H0 H7, H0 H4 - H1 H3]     (d = 0 or not finite: MODS_E_ARG);
 *     out1 = image 1, out2 = image 2.  For out1 (G = Hinv, own = region 1, other = region 2; out2: G = H, roles swapped): unless
 *     draw_only_centers, per match the own contour in colour1 / r1 and the other's through G in colour2 / r2: with B = [A11 A12 x | A21
 *     A22 y | 0 0 1] (A = (3.0 s) a), P[r][c] = (G[3r] B[0][c] + G[3r+1] B[1][c]) + G[3r+2] B[2][c], X[r] = (P[r][0] C[k] + P[r][1] S[k]) +
 *     P[r][2] * 1.0, the point (floor(X[0] / X[2]), floor(X[1] / X[2])).  Then per match DISC(own centre, r1 + 2, colour1), DISC(((int)xa,
 *     (int)ya), r2, colour2) with xa = ((G0 x + G1 y) + G2) / ((G6 x + G7 y) + G8), ya likewise with G3 G4 G5, of the other centre, and
 *     the LINE from (xa, ya) to the own centre in colour2. */
typedef struct mods_canvas mods_canvas;
enum { MODS_DRAW_NONE = -1, MODS_DRAW_DISC = 0, MODS_DRAW_LINE = 1, MODS_DRAW_SEG = 2 };
enum { MODS_DRAW_TABLE_REGIONS = 0, MODS_DRAW_TABLE_MATCHES = 1 };
typedef struct mods_draw_elem { int kind, ax, ay, bx, by, t; unsigned rgb; int group; } mods_draw_elem;
typedef struct mods_draw_matches_params {
  int draw_only_centers, reproject_to_one_image, draw_epipolar_lines, r1, r2, pad;
  double M[9];               /* row-major: H with reproject_to_one_image, F (as mods_pair_result.H holds it) with draw_epipolar_lines */
} mods_draw_matches_params;
int mods_canvas_create(mods_ctx *ctx, int w, int h, mods_canvas **out);   /* 1 <= w, h <= 16384; contents undefined until filled */
void mods_canvas_destroy(mods_canvas *cv);
int mods_canvas_width(const mods_canvas *cv);
int mods_canvas_height(const mods_canvas *cv);
int mods_canvas_fill(mods_canvas *cv, unsigned rgb);
/* an 8-bit host image of 1 (grey, replicated) or 3 (R G B) channels with its corner at (x0, y0); clipped to the canvas */
int mods_canvas_blit_u8(mods_canvas *cv, const unsigned char *img, int w, int h, int channels, int x0, int y0);
/* an fp32 grey device image as (uint8)rint(min(max(px, 0), 255)), NaN as 0 */
int mods_canvas_blit_f32_dev(mods_canvas *cv, const float *img_dev, int w, int h, int stride, int x0, int y0);
int mods_canvas_blit_canvas(mods_canvas *cv, const mods_canvas *src, int x0, int y0);
int mods_canvas_fetch(mods_canvas *cv, unsigned char *rgb_out);           /* h * w * 3 bytes */
int mods_canvas_draw(mods_canvas *cv, const mods_draw_elem *elems, int n, int *n_dropped);
int mods_canvas_draw_regions(mods_canvas *cv, const mods_imgrep *rep, int begin, int count, int dx, int dy, int thickness, unsigned rgb,
                             int table, int *n_dropped);
int mods_canvas_regions_elems(mods_canvas *cv, const mods_imgrep *rep, int begin, int count, int dx, int dy, int thickness, unsigned rgb,
                              int table, mods_draw_elem *out, int *n_dropped);
int mods_draw_matches_elems(int which, int w1, int h1, int w2, int h2, const double *laf14, int n, const mods_draw_matches_params *par,
                            mods_draw_elem *out, int max_out, int *n_out);
/* src1, src2: the two images as canvases; *out1, *out2: new canvases (the caller destroys them); n_dropped2[i]: of image i */
int mods_draw_matches(mods_ctx *ctx, const mods_canvas *src1, const mods_canvas *src2, const double *laf14, int n,
                      const mods_draw_matches_params *par, mods_canvas **out1, mods_canvas **out2, int *n_dropped2);
/* The frames of the verified correspondences of the context's last mods_match_pair_dev / ladder / mods_match_verify_reps call, in the
 * order of its matches_out: up to max rows x y a11 a12 a21 a22 s of region 1, then of region 2; *n = how many there are */
int mods_ctx_verified_lafs(mods_ctx *ctx, double *laf14, int max, int *n);
int mods_multi_verified_lafs(mods_multi *m, double *laf14, int max, int *n);

/* ---- refinement of correspondences by affine least-squares matching -------------------------------------------
 * Gruen, "Adaptive least squares correlation", 1985; the photometric refinement of Barath et al., "Making affine correspondences
 * work in camera geometry computation", ECCV 2020.  No counterpart in the reference: this is the contract (csrc/refine.hip,
 * restated in tests/lsm_ref.py).  The pixel window of one image is registered onto the other by an iterated Gauss-Newton fit of a
 * translation and a 2 x 2 affinity with gain and offset; it yields a sub-pixel position, a refined frame and a ZNCC score per
 * correspondence.  It never adds or removes a correspondence (mods_propagate_matches below does).  Every operation is fp64 on fp32
 * pixels, no contraction.
 *
 * Input: laf14[n][14] = x1 y1 a11 a12 a21 a22 s1 | x2 y2 b11 b12 b21 b22 s2, as mods_ctx_verified_lafs returns it.  Per row:
 *   Roles      M1 = s1 A1, M2 = s2 A2 (entry by entry), d1 = det M1, d2 = det M2, B0 = M2 M1^-1 (M1^-1 = adj(M1) / d1, entry by entry,
 *              as the local affine filter writes it), dB0 = det B0.  dB0 >= 1: image 1 is the template image (t), image 2 the
 *              search image (s), B = B0.  Otherwise the roles are swapped and B = B0^-1 = adj(B0) / dB0.  So the window is taken at
 *              native resolution where the region is smaller and is magnified into the other image.  BAD_FRAME: one of the 14
 *              values is not finite, d1 == 0, d2 == 0, B0 or dB0 not finite, dB0 <= 0, or sqrt(det B) > max_magnification.
 *   Sampling   bil(I, x, y): x0 = floor(x), fx = x - x0, y0 = floor(y), fy = y - y0; a = I[y0][x0], b = I[y0][x0+1], c = I[y0+1][x0],
 *              d = I[y0+1][x0+1];  value = (a (1-fx) + b fx) (1-fy) + (c (1-fx) + d fx) fy;  gx = (b-a) (1-fy) + (d-c) fy;
 *              gy = (c-a) (1-fx) + (d-b) fx.  A tap with x0 < 0, y0 < 0, x0 > w-2, y0 > h-2 (or a position that is not finite)
 *              rejects the row with status OUTSIDE - in the template, in any iteration or in the final evaluation.
 *   Window     S = (2R+1)^2 offsets u_k = (ux, uy), ux = k mod (2R+1) - R, uy = k div (2R+1) - R, k = 0 .. S-1.
 *   Sums       every sum over the window is taken in one order: lane l = 0 .. 63 adds its terms k = l, l + 64, l + 128, ... in
 *              ascending k to +0.0; then for o = 32, 16, 8, 4, 2, 1 every lane replaces its value by value + value of lane (l xor o).
 *              All 64 lanes end with the same bits.  mean(X) = sum(X) / S.
 *   Template   T_k = bil(I_t, c_t + u_k) (value only), T -= mean(T), Stt = sum(T T).  FLAT when Stt <= 1e-6 S.
 *   Iteration  (c, B) start at (c_s, B).  p_k = (cx + (B00 ux + B01 uy), cy + (B10 ux + B11 uy)); W_k, gx_k, gy_k = bil(I_s, p_k);
 *              columns q_0..5 = gx, gy, gx ux, gx uy, gy ux, gy uy; Wc = W - mean(W), d_j = q_j - mean(q_j);
 *              Swt = sum(Wc T), Sww = sum(Wc Wc); gain a = Swt / Sww; zncc = Swt / sqrt(Sww Stt) (0 when Sww Stt is not > 0);
 *              r = T - a Wc, J_j = a d_j; N_ij = sum(J_i J_j), g_i = sum(J_i r) for i, j < P (P = 6, or 2 with affine = 0);
 *              tr = N_00 + .. + N_(P-1)(P-1) in that order; N_ii += lambda tr; delta = N^-1 g by Cholesky (N = L L^T, lower, column
 *              by column; a pivot that is not > 0 - NaN included - is status FLAT), forward then backward substitution;
 *              cx += delta_0, cy += delta_1, B00 += delta_2, B01 += delta_3, B10 += delta_4, B11 += delta_5.
 *              Converged when sqrt(delta_0^2 + delta_1^2) < eps_shift; max_iter iterations without that: MAXITER, values kept.
 *              iterations = the number of updates applied.  zncc_before = the zncc of the first iteration's sums.
 *   End        zncc_after = the zncc at the returned (c, B) (one more sampling).  DIVERGED when not
 *              sqrt((cx-csx)^2 + (cy-csy)^2) <= max_shift, or when q = sqrt(det B / det B_start) is not inside
 *              [1 / max_scale_change, max_scale_change].  Else LOW_ZNCC when not zncc_after >= min_zncc.  Else MAXITER or OK.
 *   Output     OK and MAXITER are accepted: the search side of the row gets the centre c and the frame M' = B M_t stored as
 *              s' = sqrt(|det M'|), A' = M' / s'; the template side is untouched.  Every other row comes back as it went in; only
 *              its status, its iteration count and the zncc values that were computed (others: 0) are written.
 *              u6_out[n][6] = x1 y1 1 x2 y2 1 of laf_out.
 * The result for a row depends only on that row and the two images: not on n, the row's place or the launch geometry.
 *
 * MODS_E_ARG with a mods_last_error text starting "refine_matches: ", before any device call: n < 0; radius outside 1 .. 15;
 * max_iter outside 1 .. 1000; eps_shift, max_shift, lambda not finite or <= 0; max_scale_change, max_magnification not finite or
 * < 1; min_zncc NaN or outside [-1, 1]; affine not 0 / 1; an image smaller than 2 x 2 or a stride below the width; a null context,
 * image or (n > 0) laf14.  par == NULL: the defaults.  Any output may be null.  n == 0: MODS_OK, nothing is launched.
 * The rows are staged in a buffer of the context's own; the matcher's "last search" and the guided / overlap buffers are left
 * alone.  Timer: MODS_STAGE_REFINE.  mods_refine_matches: the same with host images (dense rows of stride floats), uploaded first.
 * mods_refit_model: the least-squares model over all n rows of u6 (x1 y1 1 x2 y2 1) through the host fits of the LO steps -
 * model_type 0: the normalised homography fit (u2h), returned row-major image 1 -> image 2 as mods_pair_result.H holds it, n >= 4;
 * 1: the normalised 8-point fit with rank-2 projection (u2f), as mods_pair_result.H holds F, n >= 8.  No device, no RANSAC.
 * mods_test_lsm_iteration: the first iteration of one row through the kernel: N (6 x 6, symmetric, the damped matrix; entries
 * outside P x P are 0), g[6], the gain a and delta[6]; *status_out = BAD_FRAME / OUTSIDE / FLAT when the row ended before them. */
enum { MODS_LSM_OK = 0, MODS_LSM_MAXITER = 1, MODS_LSM_BAD_FRAME = 2, MODS_LSM_OUTSIDE = 3, MODS_LSM_FLAT = 4, MODS_LSM_DIVERGED = 5,
       MODS_LSM_LOW_ZNCC = 6, MODS_LSM_STATUS_COUNT };
typedef struct mods_lsm_params {
  int radius;                 /* 10    the window is (2 radius + 1)^2; 1 .. 15 */
  int max_iter;               /* 20 */
  double eps_shift;           /* 0.01  px of the search image */
  double max_shift;           /* 3.0   px of the search image */
  double max_scale_change;    /* 1.5 */
  double max_magnification;   /* 8 */
  double min_zncc;            /* 0.8 */
  double lambda;              /* 1e-9  damping, relative to the trace */
  int affine;                 /* 1; 0: translation only */
  int pad;
} mods_lsm_params;
void mods_lsm_defaults(mods_lsm_params *par);
int mods_refine_matches_dev(mods_ctx *ctx, const float *img1_dev, int w1, int h1, int stride1, const float *img2_dev, int w2, int h2,
                            int stride2, const double *laf14, int n, const mods_lsm_params *par, double *laf_out, double *u6_out,
                            int *status_out, int *iters_out, double *zncc_before_out, double *zncc_after_out);
int mods_refine_matches(mods_ctx *ctx, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2,
                        int stride2, const double *laf14, int n, const mods_lsm_params *par, double *laf_out, double *u6_out,
                        int *status_out, int *iters_out, double *zncc_before_out, double *zncc_after_out);
int mods_refit_model(const double *u6, int n, int model_type, double *model_out);
int mods_test_lsm_iteration(mods_ctx *ctx, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2,
                            int stride2, const double *laf14_row, const mods_lsm_params *par, double *N36, double *g6, double *a,
                            double *delta6, int *status_out);

/* ---- quasi-dense matches by propagation from refined correspondences -------------------------------------------
 * Lhuillier and Quan, "Match propagation for image-based modeling and rendering", PAMI 2002; Kannala and Brandt, "Quasi-dense wide
 * baseline matching using match propagation", CVPR 2007 (affine frames).  No counterpart in the reference: this is the contract
 * (csrc/propagate.hip, restated in tests/propagate_ref.py).  A refined correspondence carries a local affine map of image 1 onto
 * image 2; the map predicts where the neighbours of the point land, the least-squares matching above tests every prediction
 * against the pixels, and the accepted ones predict their own neighbours in the next round.  Every operation is fp64 in the order
 * written, no contraction; "LSM" is the contract of mods_refine_matches, row by row, with the parameters par->lsm.
 *
 * Lattice    image 1 is cut into Gx = floor(w1 / cell) by Gy = floor(h1 / cell) cells; cell (gx, gy) has the centre p = ((double)(gx
 *            cell) + (cell - 1) * 0.5, (double)(gy cell) + (cell - 1) * 0.5).  A cell is free, occupied or closed; all start free.
 * Round 0    every seed row goes through LSM unchanged; seed_status[n] = its status.  The seeds with status OK are the first front
 *            (MAXITER does not propagate), in seed order.  A front row's own cell is (floor(x1 / cell), floor(y1 / cell)) of its
 *            round-0 output row; where that lies inside the grid the cell becomes occupied (outside - the partial last column
 *            or row - the row still proposes).  The seeds are not part of the output list.
 * Round r    1 Propose.  Every front row k proposes every cell within `reach` (Chebyshev) of its own cell that is free and inside
 * (1, 2, ..)   the grid.  With (dx, dy) = p - (x1, y1) of row k: d2 = (float)(dx dx + dy dy); among the proposers of a cell the
 *              smallest (d2, k) wins, k = the place of the row in the front (the key: bits of d2 << 32 | k, unsigned 64-bit).
 *            2 List.  The proposed cells in raster order (gy major) become the candidate rows of the round.  With the winner's
 *              output row: M1, M2, d1 and B0 = M2 M1^-1 entry by entry as the LSM "Roles" paragraph writes them, dB = B0_00 B0_11 -
 *              B0_01 B0_10, s = sqrt(dB), q = (x2 + (B0_00 dx + B0_01 dy), y2 + (B0_10 dx + B0_11 dy)) with (dx, dy) as above.
 *              Candidate row = px py 1 0 0 1 1 | qx qy B0_00/s B0_01/s B0_10/s B0_11/s s.
 *            3 Register.  The candidate rows go through LSM.
 *            4 Gate.  A candidate is accepted when its status is OK and it passes the model test on its output row (x1, y1, x2,
 *              y2); a row that fails the test ends with status MODS_PROP_OFF_MODEL.  model_type -1: no test.  Mij as the guided
 *              matching above defines it; thr2 = model_thr model_thr.
 *              0 (H): X = (M00 x1 + M01 y1) + M02, Y, W alike; W must be finite and not 0; ex = X / W - x2, ey = Y / W - y2; passes
 *                when ex ex + ey ey <= thr2.
 *              1 (F): l_i = (Mi0 x1 + Mi1 y1) + Mi2 for i = 0, 1, 2; m0 = (M00 x2 + M10 y2) + M20, m1 = (M01 x2 + M11 y2) + M21;
 *                e = (l0 x2 + l1 y2) + l2; den = ((l0 l0 + l1 l1) + m0 m0) + m1 m1; passes when den != 0 and (e e) / den <= thr2
 *                (Sampson).  A comparison with NaN fails.
 *            5 State.  The cells of the accepted rows become occupied; their output rows, in raster order, are appended to the
 *              output list and are the next front; their own cell is the proposed cell, wherever LSM moved x1.  Every other
 *              proposed cell is closed for good.
 * End        after `rounds` rounds, after a round that proposed nothing, or after a round that was cut: when the list would pass
 *            max_out rows, the accepted rows of that round are taken in raster order up to max_out, *truncated = 1 (else 0) and
 *            no further round runs.
 * Outputs (any may be null): laf_out[max_out][14]; u6_out[max_out][6] = x1 y1 1 x2 y2 1; zncc_out = zncc_after; iters_out = the LSM
 * iterations; round_out; cell_out[max_out][2] = gx gy of the row's own cell; parent_out = the winner in the combined list, 0 ..
 * n - 1 a seed, n + j output row j; *n_out; seed_status[n]; stats[(rounds + 1)][MODS_PROP_STATUS_COUNT] = how many rows of each
 * round (0: the seeds) ended in each status, rows beyond max_out included, rounds that did not run 0; tried_status[Gy][Gx] and
 * tried_iters[Gy][Gx] = the status and the iteration count of the one candidate ever tried at a cell (-1: none).
 * Nothing depends on launch geometry or timing; a repeated call returns the same bytes.
 *
 * MODS_E_ARG with a mods_last_error text starting "propagate_matches: ", before any device call: what mods_refine_matches refuses
 * (for par->lsm, the images, n, laf14); cell outside 2 .. 64, reach outside 1 .. 4, rounds outside 1 .. 64; model_type outside
 * -1 .. 1; with a model, an entry that is not finite or model_thr not finite or <= 0; max_out < 0; an image 1 smaller than one
 * cell.  par == NULL: the defaults.  n == 0: MODS_OK, nothing is launched, *n_out = 0, *truncated = 0, stats and the tried maps are
 * not written.  Grid, rows and images live in buffers of the context's own, grown on demand: the matcher's "last search" and the
 * guided / overlap / k-NN / refine buffers are left alone.  The host waits for the device once per round that runs (for the number
 * of candidates) and once at the end; a buffer that has to grow waits once more (the early rounds of a context's first call), and
 * mods_propagate_matches waits for its image upload.  Timer: MODS_STAGE_PROPAGATE (every launch of the call, the LSM launches included).
 * mods_test_propagate_round: one Propose and List pass.  front_laf[nf][14] = the front's output rows; front_cell[nf][2] = their own
 * cells (null: floor(x1 / cell), floor(y1 / cell)); state[Gy][Gx] = 0 free, 1 occupied, 2 closed (null: all free).  winner_out[Gy][Gx]
 * (-1: not proposed), key_out[Gy][Gx] (all ones: not proposed), cand_cell_out[n_cand] = gy Gx + gx in list order, cand_laf_out[n_cand][14];
 * the last two hold up to Gx Gy rows. */
enum { MODS_PROP_OFF_MODEL = MODS_LSM_STATUS_COUNT, MODS_PROP_STATUS_COUNT };
typedef struct mods_propagate_params {
  int cell;                   /* 4     px of image 1; 2 .. 64 */
  int reach;                  /* 1     cells, Chebyshev; 1 .. 4 */
  int rounds;                 /* 8     1 .. 64 */
  int model_type;             /* -1    -1 none, 0 H, 1 F, as mods_pair_result.H delivers them */
  mods_lsm_params lsm;        /* mods_lsm_defaults with radius 5 */
  double model[9];
  double model_thr;           /* 2.0   px (H) / px of the Sampson distance (F) */
} mods_propagate_params;
void mods_propagate_defaults(mods_propagate_params *par);
int mods_propagate_matches_dev(mods_ctx *ctx, const float *img1_dev, int w1, int h1, int stride1, const float *img2_dev, int w2, int h2,
                               int stride2, const double *laf14, int n, const mods_propagate_params *par, int max_out, double *laf_out,
                               double *u6_out, double *zncc_out, int *iters_out, int *round_out, int *cell_out, int *parent_out,
                               int *n_out, int *truncated, int *seed_status, int *stats, int *tried_status, int *tried_iters);
int mods_propagate_matches(mods_ctx *ctx, const float *img1, int w1, int h1, int stride1, const float *img2, int w2, int h2,
                           int stride2, const double *laf14, int n, const mods_propagate_params *par, int max_out, double *laf_out,
                           double *u6_out, double *zncc_out, int *iters_out, int *round_out, int *cell_out, int *parent_out,
                           int *n_out, int *truncated, int *seed_status, int *stats, int *tried_status, int *tried_iters);
int mods_test_propagate_round(mods_ctx *ctx, int w1, int h1, int cell, int reach, const double *front_laf, const int *front_cell, int nf,
                              const unsigned char *state, int *winner_out, unsigned long long *key_out, int *cand_cell_out,
                              double *cand_laf_out, int *n_cand_out);

#ifdef __cplusplus
}
#endif
#endif /* MODS_HIP_H */
