// mods - command-line front end of the MI355X matcher, argument- and file-compatible with the reference's
// `mods` binary for the part of the system that is in scope (HessianAffine + RootSIFT steps, LO-RANSAC
// homography or DEGENSAC epipolar verification).
//
// Reference behaviour:
//   argv layout        getCLIparam, io_mods.cpp:558-603 (Tmin = 9, io_mods.h:13):
//       mods img1 img2 out1 out2 k1 k2 matchings log [logOnly] [ver_type] [H/F file] [config.ini] [iters.ini]
//            [read_pre_extracted] [match_one_to_many]
//       ver_type 0 = LO-RANSAC homography, 1 = ground-truth homography (the H file is read), 2 = LO-RANSAC epipolar ([RANSAC] aContrario = 1: ORSA-H under 0, ORSA F under 2; 3 is rejected)
//   configuration      the [HessianAffine], [DominantOrientation], [SIFTDescriptor], [Matching], [DuplicateFiltering],
//                      [RANSAC], [TextOutput], [Computing] keys of io_mods.cpp:160-207, 423-455, 605-740 and the
//                      [Iterations] / [HessianAffine<i>] sections of the iterations file (:457-492)
//   step loop          mods.cpp:202-383 (mods_match_ladder_dev)
//   outputs            matchings "x1 y1 x2 y2" (matching.cpp:2596-2613), log line (io_mods.cpp:10-66),
//                      keypoint files (imagerepresentation.cpp:198-204, 1219-1255), H/F file (matching.cpp:2681-2686),
//                      time.log (io_mods.cpp:67-99, mods.cpp:528-540); exit code 0 / 1
// Detectors: HessianAffine, DoG, HarrisAffine (one scale-space detector, three responses) and MSER; ORB / FAST / ... steps of an
// iterations file are skipped with a warning.  Match and region images (out1 / out2, mods.cpp:452-505) are drawn on the GPU when
// [ImageOutput] writeImages / drawDetectedRegions ask for them (mods_draw_matches, mods_canvas_draw_regions).  Pre-extracted input
// (read_pre_extracted = 1) is read from .npz or text keypoint files.  The vector matcher is always the exact (linear) search;
// external (ZMQ) descriptor / AffNet / OriNet daemons are used when the configuration asks for them.
#include "../../include/mods_hip.h"
#include "../../include/mods_zmq.h"
#include "image_io.hpp"
#include "npz_io.hpp"
#include "ini_reader.hpp"
#include <chrono>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>

using modscli::GreyImage;
using modscli::IniReader;

namespace {

const int Tmin = 9;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

bool ends_with(const std::string &s, const std::string &suffix) {
  return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}

struct Config {
  mods_pair_params pair;
  // the scale-space detectors that have views in some step, sorted by name (the reference's maps are keyed by name), their
  // parameter sets, and steps[step * n_det + d] = detector d's section of that step (n_tilts = -1: none)
  std::vector<std::string> det_names;
  std::vector<mods_hessaff_params> det_params;
  std::vector<mods_ladder_step> steps;
  // grouped matching ([Matching<i>] GroupDetectors / GroupDescriptors, correspondencebank.cpp:245-285): one entry per step when
  // any step names a group; group_pos = place of the bank's "Group" entry among the detector names
  std::vector<mods_ladder_group> groups;
  int group_pos = 0;
  int max_steps = 4, min_matches = 15;
  int load_color = 1;
  int do_clahe = 0;                // [Matching] doCLAHE (io_mods.cpp:526): CLAHE on both 8-bit grey images before detection
  // [DetectionMask] (no counterpart in the reference's command line; its author began mods-with-mask.cpp): mask1 / mask2 = an 8-bit
  // image of image 1 / 2's size, 0 = no regions there; useMaskFiles = 1: <image path without extension>_mask.png for an image
  // without a key of its own, where that file exists (mods_ctx_detection_mask)
  std::string mask_fn[2];
  int use_mask_files = 0;
  int mutual_check = 0;            // [Matching] mutualCheck (no counterpart in the reference): mods_ctx_match_mutual
  // [Matching] distractorDB / distractorDBHalf = a.npz[,b.npz...]: keypoint files of this program whose descriptors make the distractor
  // databases of the FGINN searches (mods_ctx_distractor_db; MatchFlannFGINNPlusDB, which the reference never calls); absent: none
  std::string distractor_db, distractor_db_half;
  // [SpatialSelection] doSpatialSelection / robustness (no counterpart in the reference): the FixedRegNumber / RelativeRegNumber steps
  // of the scale-space detectors keep the keys with the largest suppression radius (mods_ctx_spatial_selection, mode 2)
  int spatial = 0;
  double spatial_c = 0.9;
  // [HessianAffine] upscaleInputImage (PyramidParams::upscaleInputImage, structures.hpp:116-117; no .ini key of the reference sets it):
  // the scale-space detectors of the run start at the doubled image (mods_ctx_upscale_input)
  int upscale = 0;
  // [SIFTDescriptor] domainSizePooling (the gate; no counterpart in the reference) with the reference's numScales / startCoef /
  // endCoef (io_mods.cpp:431-433, parsed there and never used): mods_ctx_domain_pooling
  int dsp = 0, dsp_scales = 3;
  double dsp_start = 0.5, dsp_end = 1.5;
  int local_affine = 0;            // [LocalAffineFiltering] doLocalAffineFiltering (no counterpart in the reference): mods_ctx_local_affine
  mods_local_affine_params la_par;
  int verbose = 0, time_log = 1, write_keypoints = 1, write_matches = 1, output_h = 0;
  // [Matching] guidedMatching (no counterpart in the reference): behind the final verification every bank is searched again under
  // the verified model (mods_match_guided_reps) and the de-duplicated result is what the matches file holds
  int guided = 0, guided_max_dist = 0, guided_one_to_one = 1;
  double guided_radius = 0, guided_ratio = 0.9;
  // [Matching] rematchUnderH (no counterpart in the reference's live path; it began GenerateSynthImageByH and never called it):
  // under ver_type 0, once the step loop has verified an H, image 1 is seen through it, detected and described, its regions join
  // bank 1 (2: image 2 through inv(H) joins bank 2 as well) and the banks are matched and verified once more; every output
  // then comes from that pass
  int rematch = 0;
  // [MatchRefinement] doRefinement (no counterpart in the reference): the verified correspondences are refined by affine least-squares
  // matching on the two images (mods_refine_matches_dev), last of all; refitModel = 1: the H / F file then takes the least-squares
  // model of the refined rows (mods_refit_model)
  int refine = 0, refit_model = 1;
  mods_lsm_params lsm_par;
  // [MatchPropagation] doPropagation (no counterpart in the reference): the verified correspondences (the refined ones with
  // [MatchRefinement]) grow into quasi-dense ones by match propagation on the two images (mods_propagate_matches_dev), after
  // everything else; useModel = 1: under the model that goes to the H / F file, within modelThreshold (default: [RANSAC]
  // err_threshold).  `output` receives them; the matches file, the log and every count stay as they are
  int propagate = 0, prop_use_model = 1;
  bool prop_thr_set = false;
  mods_propagate_params prop_par;
  std::string prop_output;
  // [OverlapMatching] doOverlapMatch / overlapError (io_mods.cpp:685-687) and matchOriented (ours): with ver_type 1 every detector's
  // banks go through mods_match_overlap_reps under the ground-truth H and the count is printed as mods.cpp:522-523 does
  int overlap = 0, overlap_oriented = 1;
  double overlap_error = 0.09;
  // overlapMeasure = linear | area and overlapAreaError (ours): with `area` the banks go through mods_match_overlap_area_reps instead -
  // intersection over union of the ellipses, greedy one-to-one assignment, the measure published repeatability figures use
  int overlap_area = 0;
  double overlap_area_error = 0.4;
  // [zmqDescriptor] (io_mods.cpp:395-407): used when a step asks for the "ZMQ" descriptor instead of RootSIFT
  bool use_zmq = false;
  std::string zmq_port = "tcp://localhost:5555";
  double zmq_mr = 3.0 * 1.7320508075688772;
  int zmq_ps = 32;
  // [AffineAdaptation] useZMQ + [AffNet], [DominantOrientation] useZMQ + [OriNet] (io_mods.cpp:124-134, 523-524, 727-736)
  bool aff_zmq = false, ori_zmq = false;
  std::string aff_port = "tcp://localhost:5556", ori_port = "tcp://localhost:5557";
  double aff_mr = 3.0 * 1.7320508075688772, ori_mr = 3.0 * 1.7320508075688772;
  int aff_ps = 32, ori_ps = 32;
  // weights=FILE.npz in [AffNet] / [OriNet] / [zmqDescriptor]: the network runs in-process (mods_net_*), no daemon, no port
  std::string aff_weights, ori_weights, zmq_weights;
  // precision = fp32 | bf16 beside weights=: MODS_NET_FP32 / MODS_NET_BF16; *_named: the key is in the file (verbose then names the mode)
  int aff_prec = MODS_NET_FP32, ori_prec = MODS_NET_FP32, zmq_prec = MODS_NET_FP32;
  bool aff_prec_named = false, ori_prec_named = false, zmq_prec_named = false;
  // [ImageOutput] (io_mods.cpp:647-652).  writeImages absent means 0 here (the reference: 1): a configuration without the section
  // runs as it always did; the other keys keep the reference's defaults
  int write_images = 0, draw_only_centers = 1, draw_reprojected = 1, draw_epipolar = 0, draw_regions = 0;
};

int read_config(const std::string &config_fn, const std::string &iters_fn, int ver_type, Config *cfg) {
  IniReader ini(config_fn);
  if (ini.ParseError() < 0) { std::cerr << "Can't load " << config_fn << std::endl; return 1; }
  IniReader it(iters_fn);
  if (it.ParseError() < 0) { std::cerr << "Can't load  " << iters_fn << std::endl; return 1; }
  mods_pair_params &p = cfg->pair;
  cfg->verbose = (int)ini.GetInteger("TextOutput", "verbose", 0);     // first: the notes below depend on it
  // [HessianAffine] / [DoG] / [HarrisAffine], io_mods.cpp:160-207, 208-244, 260-296: one key set, DetectorType set by the
  // section; defaults = PyramidParams / AffineShapeParams constructors
  auto read_det = [&](const char *sec, int type) {
    mods_hessaff_params d;
    memset(&d, 0, sizeof(d));
    d.detectorType = type;
    d.threshold = (float)ini.GetDouble(sec, "threshold", 16.0 / 3.0);
    d.border = (int)ini.GetInteger(sec, "border", 5);
    d.numberOfScales = (int)ini.GetInteger(sec, "numberOfScales", 3);
    d.initialSigma = (float)ini.GetDouble(sec, "initialSigma", 1.6);
    d.edgeEigenValueRatio = (float)ini.GetDouble(sec, "edgeEigenValueRatio", 10.0);
    d.maxIterations = (int)ini.GetInteger(sec, "max_iter", 16);
    d.smmWindowSize = (int)ini.GetInteger(sec, "smmWindowSize", 19);
    d.convergenceThreshold = (float)ini.GetDouble(sec, "convergenceThreshold", 0.05);
    d.doBaumberg = (int)ini.GetInteger(sec, "doBaumberg", 1);
    d.iiDoGMode = ini.GetBoolean(sec, "iiDoGMode", false) ? 1 : 0;
    d.sampleFromImage = ini.GetBoolean(sec, "sampleFromImage", false) ? 1 : 0;     // io_mods.cpp:184, 222, 275
    // patch_size (io_mods.cpp:187): the side of the normalised patch that normalizeAffine renders for a callback which only
    // records the geometry (scale-space-detector.hpp:56-90): it never reaches a keypoint, here or in the reference
    if (ini.GetInteger(sec, "patch_size", 41) != 41 && cfg->verbose)
      std::cerr << "Note: [" << sec << "] patch_size has no effect on the keypoints (the reference renders that patch and drops it)" << std::endl;
    // keypoint selection, io_mods.cpp:170-173, 194-205 (defaults: PyramidParams, structures.hpp:138-150)
    d.relativeThreshold = (float)ini.GetDouble(sec, "relativeThreshold", -1.0);
    d.relativeRegionsNumber = (float)ini.GetDouble(sec, "relativeRegionsNumber", -1.0);
    d.regionsNumber = (int)ini.GetInteger(sec, "regionsNumber", -1);
    const std::string mode = ini.GetStringVector(sec, "mode")[0];
    d.mode = mode == "RelativeTh" ? MODS_DET_RELATIVE_TH : mode == "FixedRegNumber" ? MODS_DET_FIXED_REG_NUMBER
           : mode == "NotLessThanRegions" ? MODS_DET_NOT_LESS_THAN_REGIONS : mode == "RelativeRegNumber" ? MODS_DET_RELATIVE_REG_NUMBER
           : MODS_DET_FIXED_TH;
    return d;
  };
  // [MSER], GetMSERPars (io_mods.cpp:101-123); defaults = extrema::ExtremaParams (detectors/mser/extrema/extremaParams.h:72-88)
  auto read_mser = [&]() {
    mods_hessaff_params d;
    memset(&d, 0, sizeof(d));
    d.detectorType = MODS_DET_MSER;
    d.relativeThreshold = (float)ini.GetDouble("MSER", "relativeThreshold", -1.0);
    d.relativeRegionsNumber = (float)ini.GetDouble("MSER", "relativeRegionsNumber", -1.0);
    d.regionsNumber = (int)ini.GetInteger("MSER", "regionsNumber", -1);
    d.mserMaxArea = ini.GetDouble("MSER", "max_area", 0.01);
    d.mserMinSize = (int)ini.GetInteger("MSER", "min_size", 30);
    d.mserMinMargin = (double)ini.GetInteger("MSER", "min_margin", 10);     // read as an integer (io_mods.cpp:108)
    const std::string mode = ini.GetStringVector("MSER", "mode")[0];
    d.mode = mode == "RelativeTh" ? MODS_DET_RELATIVE_TH : mode == "FixedRegNumber" ? MODS_DET_FIXED_REG_NUMBER
           : mode == "NotLessThanRegions" ? MODS_DET_NOT_LESS_THAN_REGIONS : mode == "RelativeRegNumber" ? MODS_DET_RELATIVE_REG_NUMBER
           : MODS_DET_FIXED_TH;
    return d;
  };
  p.det = read_det("HessianAffine", MODS_DET_HESSIAN);
  // only this section reads the key (io_mods.cpp:193); AffineBaumbergMethod, affine.h:21-24
  p.det.affBmbrgMethod = (int)ini.GetInteger("HessianAffine", "affBmbrgMethod", 0);
  if (p.det.affBmbrgMethod != 0 && p.det.affBmbrgMethod != 1) { std::cerr << "[HessianAffine] affBmbrgMethod must be 0 (SMM) or 1 (Hessian)" << std::endl; return 1; }
  // [DominantOrientation] :731-740 and [SIFTDescriptor] :423-436
  mods_describe_params &q = p.desc;
  q.ori_mrSize = ini.GetDouble("DominantOrientation", "mrSize", 3.0 * std::sqrt(3.0));
  q.ori_patchSize = (int)ini.GetInteger("DominantOrientation", "patchSize", 32);
  q.ori_maxAngles = (int)ini.GetInteger("DominantOrientation", "maxAngles", 1);
  q.ori_threshold = (double)(float)ini.GetDouble("DominantOrientation", "threshold", 0.8);
  q.addUpRight = ini.GetBoolean("DominantOrientation", "addUpRight", false) ? 1 : 0;      // io_mods.cpp:732
  // (halfSIFTMode and addMirrored of the same section are parsed by the reference and used nowhere: io_mods.cpp:733-734)
  q.desc_mrSize = ini.GetDouble("SIFTDescriptor", "mrSize", 3.0 * std::sqrt(3.0));
  q.desc_patchSize = (int)ini.GetInteger("SIFTDescriptor", "patchSize", 41);
  q.photoNorm = ini.GetBoolean("SIFTDescriptor", "photoNorm", true) ? 1 : 0;
  q.rootSift = 1;
  q.maxBinValue = ini.GetDouble("SIFTDescriptor", "maxBinValue", 0.2);
  q.fastExtraction = ini.GetBoolean("SIFTDescriptor", "FastPatchExtraction", false) ? 1 : 0;
  cfg->dsp = (int)ini.GetInteger("SIFTDescriptor", "domainSizePooling", 0);
  if (cfg->dsp != 0 && cfg->dsp != 1) { std::cerr << "[SIFTDescriptor] domainSizePooling must be 0 or 1" << std::endl; return 1; }
  if (cfg->dsp) {   // (with the gate 0 the three keys are ignored, as the reference ignores them)
    cfg->dsp_scales = (int)ini.GetInteger("SIFTDescriptor", "numScales", 3);
    cfg->dsp_start = ini.GetDouble("SIFTDescriptor", "startCoef", 0.5);
    cfg->dsp_end = ini.GetDouble("SIFTDescriptor", "endCoef", 1.5);
    if (cfg->dsp_scales < 0 || cfg->dsp_scales > 8) { std::cerr << "[SIFTDescriptor] numScales must lie in 2 .. 8 (0 or 1: no pooling) with domainSizePooling = 1, not " << cfg->dsp_scales << std::endl; return 1; }
    if (cfg->dsp_scales < 2) cfg->dsp = 0;          // one domain is the unpooled descriptor (mods_ctx_domain_pooling: off)
    if (cfg->dsp) {
      if (!std::isfinite(cfg->dsp_start) || !(cfg->dsp_start > 0)) { std::cerr << "[SIFTDescriptor] startCoef must be a positive number, not " << cfg->dsp_start << std::endl; return 1; }
      if (!std::isfinite(cfg->dsp_end) || !(cfg->dsp_end > cfg->dsp_start) || cfg->dsp_end > 4) { std::cerr << "[SIFTDescriptor] endCoef must lie in (startCoef, 4], not " << cfg->dsp_end << std::endl; return 1; }
      if (q.fastExtraction) { std::cerr << "[SIFTDescriptor] domainSizePooling = 1 cannot be combined with FastPatchExtraction = 1" << std::endl; return 1; }
    }
  }
  if (ini.GetInteger("SIFTDescriptor", "spatialBins", 4) != 4 || ini.GetInteger("SIFTDescriptor", "orientationBins", 8) != 8) {
    std::cerr << "Only 4x4x8 SIFT is supported" << std::endl;
    return 1;
  }
  // [Matching]
  p.fginn_ratio = 0.8;
  p.contradDist = ini.GetDouble("Matching", "contradDist", 10.0);
  p.nn = 50;
  const std::string vm = ini.GetString("Matching", "vector_matcher", "");
  if (!vm.empty() && vm != "linear") std::cerr << "Note: vector_matcher=" << vm << ": this build always searches exactly (the linear index), the approximate indices of FLANN are not reproduced" << std::endl;
  // [DuplicateFiltering] :665-679
  p.dup_dist = ini.GetDouble("DuplicateFiltering", "duplicateDist", 3.0);
  p.dup_before_ransac = (int)ini.GetDouble("DuplicateFiltering", "doBeforeRANSAC", 1);
  const std::string fm = ini.GetString("DuplicateFiltering", "whichCorrespondenceRemains", "random");
  p.dup_mode = fm == "bestFGINN" ? 1 : fm == "bestDistance" ? 2 : fm == "biggerRegion" ? 3 : 0;
  // [RANSAC] :437-455
  mods_ransac_params &r = p.ransac;
  r.err_threshold = ini.GetDouble("RANSAC", "err_threshold", 2.0);
  r.confidence = ini.GetDouble("RANSAC", "confidence", 0.99);
  r.max_samples = (int)ini.GetInteger("RANSAC", "max_samples", 100000);
  r.localOptimization = (int)ini.GetInteger("RANSAC", "localOptimization", 1);
  r.LAFCoef = (double)ini.GetInteger("RANSAC", "LAFcoef", ini.GetInteger("Matching", "LAFcoef", 0));
  r.HLAFCoef = (double)ini.GetInteger("RANSAC", "HLAFcoef", 10);
  r.doSymmCheck = (int)ini.GetInteger("RANSAC", "doSymmCheck", 0);
  const std::string et = ini.GetStringVector("RANSAC", "ErrorType")[0];
  r.errorType = et == "Sampson" ? 0 : et == "SymmMax" ? 1 : 2;
  // [RANSAC] aContrario = 1 (this project's key): the threshold-free a-contrario verifier of the chosen model, ORSA-H (useF = 3)
  // under ver_type 0 and ORSA F (useF = 2) under ver_type 2; err_threshold then only bounds the LAF check of ORSA F
  const long a_contrario = ini.GetInteger("RANSAC", "aContrario", 0);
  if (a_contrario != 0 && a_contrario != 1) { std::cerr << "[RANSAC] aContrario must be 0 or 1" << std::endl; return 1; }
  r.useF = ver_type == 2 ? (a_contrario ? 2 : 1) : (a_contrario ? 3 : 0);
  // GR_TRUTH (mods.cpp:85-87, 290-320, 381-383; io_mods.cpp:340-341): with doBothRANSACgroundTruth the verified list is the
  // LORANSAC inliers that the ground truth confirms, RANSACforStopping stops the step loop on the RANSAC inlier count
  r.groundTruth = ver_type == 1 ? (ini.GetInteger("Matching", "doBothRANSACgroundTruth", 1) ? 2 : 1) : 0;
  r.ransacForStopping = ini.GetInteger("Matching", "RANSACforStopping", 1) ? 1 : 0;
  cfg->guided = (int)ini.GetInteger("Matching", "guidedMatching", 0);
  cfg->guided_radius = ini.GetDouble("Matching", "guidedRadius", r.err_threshold);
  cfg->guided_ratio = ini.GetDouble("Matching", "guidedRatio", 0.9);
  cfg->guided_max_dist = (int)ini.GetInteger("Matching", "guidedMaxDist", 0);
  cfg->guided_one_to_one = (int)ini.GetInteger("Matching", "guidedOneToOne", 1);
  if (cfg->guided != 0 && cfg->guided != 1) { std::cerr << "[Matching] guidedMatching must be 0 or 1" << std::endl; return 1; }
  cfg->rematch = (int)ini.GetInteger("Matching", "rematchUnderH", 0);
  if (cfg->rematch < 0 || cfg->rematch > 2) { std::cerr << "[Matching] rematchUnderH must be 0, 1 (image 1 through H) or 2 (both images)" << std::endl; return 1; }
  if (!std::isfinite(cfg->guided_radius) || !(cfg->guided_radius > 0)) { std::cerr << "[Matching] guidedRadius must be a positive number of pixels, not " << cfg->guided_radius << std::endl; return 1; }
  if (!(cfg->guided_ratio > 0 && cfg->guided_ratio <= 1)) { std::cerr << "[Matching] guidedRatio must lie in (0, 1], not " << cfg->guided_ratio << std::endl; return 1; }
  if (cfg->guided_max_dist < 0) { std::cerr << "[Matching] guidedMaxDist must not be negative (0 = no cap)" << std::endl; return 1; }
  if (cfg->guided_one_to_one != 0 && cfg->guided_one_to_one != 1) { std::cerr << "[Matching] guidedOneToOne must be 0 or 1" << std::endl; return 1; }
  cfg->overlap = (int)ini.GetInteger("OverlapMatching", "doOverlapMatch", 0);
  cfg->overlap_error = ini.GetDouble("OverlapMatching", "overlapError", 0.09);
  cfg->overlap_oriented = (int)ini.GetInteger("OverlapMatching", "matchOriented", 1);
  if (cfg->overlap != 0 && cfg->overlap != 1) { std::cerr << "[OverlapMatching] doOverlapMatch must be 0 or 1" << std::endl; return 1; }
  if (!std::isfinite(cfg->overlap_error) || !(cfg->overlap_error > 0)) { std::cerr << "[OverlapMatching] overlapError must be a positive number, not " << cfg->overlap_error << std::endl; return 1; }
  if (cfg->overlap_oriented != 0 && cfg->overlap_oriented != 1) { std::cerr << "[OverlapMatching] matchOriented must be 0 or 1" << std::endl; return 1; }
  const std::string om = ini.Has("OverlapMatching", "overlapMeasure") ? ini.GetString("OverlapMatching", "overlapMeasure", "") : std::string("linear");
  if (om != "linear" && om != "area") { std::cerr << "[OverlapMatching] overlapMeasure must be linear or area, not " << om << std::endl; return 1; }
  cfg->overlap_area = om == "area";
  cfg->overlap_area_error = ini.GetDouble("OverlapMatching", "overlapAreaError", 0.4);
  if (!(cfg->overlap_area_error > 0 && cfg->overlap_area_error <= 1)) { std::cerr << "[OverlapMatching] overlapAreaError must lie in (0, 1], not " << cfg->overlap_area_error << std::endl; return 1; }
  // [TextOutput], [Computing]
  cfg->time_log = (int)ini.GetInteger("TextOutput", "timeLog", 0);
  cfg->write_keypoints = (int)ini.GetInteger("TextOutput", "writeKeypoints", 1);
  cfg->write_matches = (int)ini.GetInteger("TextOutput", "writeMatches", 1);
  cfg->output_h = (int)ini.GetInteger("TextOutput", "outputEstimatedHorF", 0);
  if (ini.GetInteger("TextOutput", "outputAllTentatives", 0)) std::cerr << "Warning: outputAllTentatives is not supported, only verified matches are written" << std::endl;
  cfg->load_color = (int)ini.GetInteger("Computing", "LoadColor", 1);
  cfg->write_images = (int)ini.GetInteger("ImageOutput", "writeImages", 0);
  cfg->draw_only_centers = (int)ini.GetInteger("ImageOutput", "drawOnlyCenters", 1);
  cfg->draw_reprojected = (int)ini.GetInteger("ImageOutput", "drawReprojected", 1);
  cfg->draw_epipolar = (int)ini.GetInteger("ImageOutput", "drawEpipolarLines", 0);
  cfg->draw_regions = ini.GetBoolean("ImageOutput", "drawDetectedRegions", false) ? 1 : 0;
  cfg->do_clahe = (int)ini.GetInteger("Matching", "doCLAHE", 0);
  cfg->mask_fn[0] = ini.GetString("DetectionMask", "mask1", "");
  cfg->mask_fn[1] = ini.GetString("DetectionMask", "mask2", "");
  cfg->use_mask_files = (int)ini.GetInteger("DetectionMask", "useMaskFiles", 0);
  cfg->distractor_db = ini.GetString("Matching", "distractorDB", "");
  cfg->distractor_db_half = ini.GetString("Matching", "distractorDBHalf", "");
  cfg->mutual_check = (int)ini.GetInteger("Matching", "mutualCheck", 0);
  if (cfg->mutual_check < 0 || cfg->mutual_check > 2) { std::cerr << "[Matching] mutualCheck must be 0, 1 or 2" << std::endl; return 1; }
  cfg->upscale = (int)ini.GetInteger("HessianAffine", "upscaleInputImage", 0);
  if (cfg->upscale != 0 && cfg->upscale != 1) { std::cerr << "[HessianAffine] upscaleInputImage must be 0 or 1" << std::endl; return 1; }
  for (const char *sec : {"DoG", "HarrisAffine"})     // one switch per context: [HessianAffine]'s value holds for the three detectors
    if (ini.Has(sec, "upscaleInputImage") && (int)ini.GetInteger(sec, "upscaleInputImage", 0) != cfg->upscale)
      std::cerr << "Note: [" << sec << "] upscaleInputImage differs from [HessianAffine]'s, which applies to every scale-space detector of the run ("
                << cfg->upscale << ")" << std::endl;
  cfg->spatial = (int)ini.GetInteger("SpatialSelection", "doSpatialSelection", 0);
  if (cfg->spatial != 0 && cfg->spatial != 1) { std::cerr << "[SpatialSelection] doSpatialSelection must be 0 or 1" << std::endl; return 1; }
  if (cfg->spatial && ini.Has("SpatialSelection", "robustness")) {   // (with the gate 0 the key is ignored)
    std::string r = ini.GetString("SpatialSelection", "robustness", "");
    while (!r.empty() && isspace((unsigned char)r.back())) r.pop_back();
    char *end = nullptr;
    cfg->spatial_c = strtod(r.c_str(), &end);
    if (r.empty() || end != r.c_str() + r.size() || !(cfg->spatial_c >= 0.0 && cfg->spatial_c <= 1.0)) {
      std::cerr << "[SpatialSelection] robustness must be a number in [0, 1], not " << r << std::endl;
      return 1;
    }
  }
  // [LocalAffineFiltering]: the filter of the list that goes to the verification, its parameters under the names of mods_local_affine_params
  // (the library checks them when the filter is switched on)
  {
    const char *sec = "LocalAffineFiltering";
    mods_local_affine_defaults(&cfg->la_par);
    cfg->local_affine = (int)ini.GetInteger(sec, "doLocalAffineFiltering", 0);
    if (cfg->local_affine != 0 && cfg->local_affine != 1) { std::cerr << "[LocalAffineFiltering] doLocalAffineFiltering must be 0 or 1" << std::endl; return 1; }
    mods_local_affine_params &q = cfg->la_par;
    q.radius = ini.GetDouble(sec, "radius", q.radius); q.minDist = ini.GetDouble(sec, "minDist", q.minDist);
    q.absTol = ini.GetDouble(sec, "absTol", q.absTol); q.relTol = ini.GetDouble(sec, "relTol", q.relTol);
    q.areaTol = ini.GetDouble(sec, "areaTol", q.areaTol); q.minSupport = (int)ini.GetInteger(sec, "minSupport", q.minSupport);
    q.rescue = (int)ini.GetInteger(sec, "rescue", q.rescue); q.keepSparse = (int)ini.GetInteger(sec, "keepSparse", q.keepSparse);
  }
  // [MatchRefinement]: the keys under the .ini's spelling; a value outside its range is an error here
  {
    const char *sec = "MatchRefinement";
    mods_lsm_defaults(&cfg->lsm_par);
    mods_lsm_params &q = cfg->lsm_par;
    const long on = ini.GetInteger(sec, "doRefinement", 0), refit = ini.GetInteger(sec, "refitModel", 1);
    const long radius = ini.GetInteger(sec, "radius", q.radius), max_iter = ini.GetInteger(sec, "maxIter", q.max_iter), affine = ini.GetInteger(sec, "affine", q.affine);
    q.min_zncc = ini.GetDouble(sec, "minZNCC", q.min_zncc); q.max_shift = ini.GetDouble(sec, "maxShift", q.max_shift);
    if (on != 0 && on != 1) { std::cerr << "[MatchRefinement] doRefinement must be 0 or 1" << std::endl; return 1; }
    if (refit != 0 && refit != 1) { std::cerr << "[MatchRefinement] refitModel must be 0 or 1" << std::endl; return 1; }
    if (radius < 1 || radius > 15) { std::cerr << "[MatchRefinement] radius must be 1 .. 15" << std::endl; return 1; }
    if (max_iter < 1 || max_iter > 1000) { std::cerr << "[MatchRefinement] maxIter must be 1 .. 1000" << std::endl; return 1; }
    if (affine != 0 && affine != 1) { std::cerr << "[MatchRefinement] affine must be 0 or 1" << std::endl; return 1; }
    if (!(q.min_zncc >= -1 && q.min_zncc <= 1)) { std::cerr << "[MatchRefinement] minZNCC must be -1 .. 1" << std::endl; return 1; }
    if (!std::isfinite(q.max_shift) || !(q.max_shift > 0)) { std::cerr << "[MatchRefinement] maxShift must be finite and > 0" << std::endl; return 1; }
    cfg->refine = (int)on; cfg->refit_model = (int)refit;
    q.radius = (int)radius; q.max_iter = (int)max_iter; q.affine = (int)affine;
  }
  // [MatchPropagation]: as above
  {
    const char *sec = "MatchPropagation";
    mods_propagate_defaults(&cfg->prop_par);
    mods_propagate_params &q = cfg->prop_par;
    const long on = ini.GetInteger(sec, "doPropagation", 0), use_model = ini.GetInteger(sec, "useModel", 1);
    const long cell = ini.GetInteger(sec, "cell", q.cell), reach = ini.GetInteger(sec, "reach", q.reach), rounds = ini.GetInteger(sec, "rounds", q.rounds);
    const long radius = ini.GetInteger(sec, "radius", q.lsm.radius);
    q.lsm.min_zncc = ini.GetDouble(sec, "minZNCC", q.lsm.min_zncc); q.lsm.max_shift = ini.GetDouble(sec, "maxShift", q.lsm.max_shift);
    cfg->prop_thr_set = ini.Has(sec, "modelThreshold");
    q.model_thr = ini.GetDouble(sec, "modelThreshold", q.model_thr);
    cfg->prop_output = ini.GetString(sec, "output", "");
    if (on != 0 && on != 1) { std::cerr << "[MatchPropagation] doPropagation must be 0 or 1" << std::endl; return 1; }
    if (use_model != 0 && use_model != 1) { std::cerr << "[MatchPropagation] useModel must be 0 or 1" << std::endl; return 1; }
    if (cell < 2 || cell > 64) { std::cerr << "[MatchPropagation] cell must be 2 .. 64" << std::endl; return 1; }
    if (reach < 1 || reach > 4) { std::cerr << "[MatchPropagation] reach must be 1 .. 4" << std::endl; return 1; }
    if (rounds < 1 || rounds > 64) { std::cerr << "[MatchPropagation] rounds must be 1 .. 64" << std::endl; return 1; }
    if (radius < 1 || radius > 15) { std::cerr << "[MatchPropagation] radius must be 1 .. 15" << std::endl; return 1; }
    if (!(q.lsm.min_zncc >= -1 && q.lsm.min_zncc <= 1)) { std::cerr << "[MatchPropagation] minZNCC must be -1 .. 1" << std::endl; return 1; }
    if (!std::isfinite(q.lsm.max_shift) || !(q.lsm.max_shift > 0)) { std::cerr << "[MatchPropagation] maxShift must be finite and > 0" << std::endl; return 1; }
    if (!std::isfinite(q.model_thr) || !(q.model_thr > 0)) { std::cerr << "[MatchPropagation] modelThreshold must be finite and > 0" << std::endl; return 1; }
    if (on && cfg->prop_output.empty()) { std::cerr << "[MatchPropagation] doPropagation = 1 needs output = FILE" << std::endl; return 1; }
    cfg->propagate = (int)on; cfg->prop_use_model = (int)use_model;
    q.cell = (int)cell; q.reach = (int)reach; q.rounds = (int)rounds; q.lsm.radius = (int)radius;
  }
  if (ini.Has("zmqDescriptor", "port")) cfg->zmq_port = ini.GetString("zmqDescriptor", "port", "");
  cfg->zmq_mr = ini.GetDouble("zmqDescriptor", "mrSize", cfg->zmq_mr);
  cfg->zmq_ps = (int)ini.GetInteger("zmqDescriptor", "patchSize", cfg->zmq_ps);
  cfg->aff_zmq = ini.GetBoolean("AffineAdaptation", "useZMQ", false);
  if (ini.Has("AffNet", "port")) cfg->aff_port = ini.GetString("AffNet", "port", "");
  cfg->aff_mr = ini.GetDouble("AffNet", "mrSize", cfg->aff_mr);
  cfg->aff_ps = (int)ini.GetInteger("AffNet", "patchSize", cfg->aff_ps);
  cfg->ori_zmq = ini.GetBoolean("DominantOrientation", "useZMQ", false);
  if (ini.Has("OriNet", "port")) cfg->ori_port = ini.GetString("OriNet", "port", "");
  cfg->ori_mr = ini.GetDouble("OriNet", "mrSize", cfg->ori_mr);
  cfg->ori_ps = (int)ini.GetInteger("OriNet", "patchSize", cfg->ori_ps);
  cfg->aff_weights = ini.GetString("AffNet", "weights", "");
  cfg->ori_weights = ini.GetString("OriNet", "weights", "");
  cfg->zmq_weights = ini.GetString("zmqDescriptor", "weights", "");
  // precision of an in-process network; any value but fp32 / bf16 ends the run here, before an image is opened
  auto read_precision = [&](const char *sec, const std::string &weights, int *prec, bool *named) {
    if (!ini.Has(sec, "precision")) return true;
    std::string v = ini.GetString(sec, "precision", "fp32");
    while (!v.empty() && (isspace((unsigned char)v.back()) || v.back() == ';')) v.pop_back();
    if (v == "fp32") *prec = MODS_NET_FP32;
    else if (v == "bf16") *prec = MODS_NET_BF16;
    else { std::cerr << "mods: [" << sec << "] precision = " << v << ": fp32 or bf16 expected" << std::endl; return false; }
    *named = true;
    if (weights.empty()) std::cerr << "Note: [" << sec << "] precision has no effect without weights= (it is the arithmetic of the in-process network)" << std::endl;
    return true;
  };
  if (!read_precision("AffNet", cfg->aff_weights, &cfg->aff_prec, &cfg->aff_prec_named) ||
      !read_precision("OriNet", cfg->ori_weights, &cfg->ori_prec, &cfg->ori_prec_named) ||
      !read_precision("zmqDescriptor", cfg->zmq_weights, &cfg->zmq_prec, &cfg->zmq_prec_named)) return 1;
  // iterations file :457-492
  cfg->max_steps = (int)it.GetInteger("Iterations", "Steps", 4);
  cfg->min_matches = (int)it.GetInteger("Iterations", "minMatches", 15);
  static const char *other_detectors[] = {"ORB", "FAST", "ReadAffs", "STAR", "BRISK", "SURF", "SIFT", "TILDE", "FOCI"};
  // the detectors of this build, in name order (the order of the reference's region / correspondence maps)
  static const struct { const char *name; int type; } ss_detectors[] = {{"DoG", MODS_DET_DOG}, {"HarrisAffine", MODS_DET_HARRIS}, {"HessianAffine", MODS_DET_HESSIAN},
                                                                        {"MSER", MODS_DET_MSER}};
  const int kDets = 4;
  std::vector<mods_ladder_step> all[4];
  for (int i = 0; i < cfg->max_steps; i++) {
    for (const char *od : other_detectors)
      if (it.Has(od + std::to_string(i), "TiltSet") || it.Has(od + std::to_string(i), "ScaleSet"))
        std::cerr << "Warning: step " << i << ": detector " << od << " is outside this build, its views are skipped" << std::endl;
    // [Matching<i>] SeparateDetectors (io_mods.cpp:320): the detectors whose lists MatchImgReps searches in this step.  The
    // reference matches nothing when the key is absent; an absent key means "every detector of the step" here.
    const std::string msec_det = "Matching" + std::to_string(i);
    std::vector<std::string> sep_det;
    const bool have_sep_det = it.Has(msec_det, "SeparateDetectors");
    if (have_sep_det)
      for (std::string name : it.GetStringVector(msec_det, "SeparateDetectors")) {
        name.erase(0, name.find_first_not_of(" \t"));
        name.erase(name.find_last_not_of(" \t") + 1);
        sep_det.push_back(name);
      }
  for (int di = 0; di < kDets; di++) {
    const std::string det_name = ss_detectors[di].name;
    const std::string sec = det_name + std::to_string(i);
    mods_ladder_step st;
    memset(&st, 0, sizeof(st));
    st.phi = it.GetDouble(sec, "Phi", 360);
    st.initSigma = it.GetDouble(sec, "initSigma", 0.5);
    st.doBlur = 1;
    // DSPLevels / minSigma / maxSigma (io_mods.cpp:480-482): SetVSPars stores them in ViewSynthParameters
    // (synth-detection.cpp:244-289) and nothing in the reference reads them again
    if (cfg->verbose && (it.Has(sec, "DSPLevels") || it.Has(sec, "minSigma") || it.Has(sec, "maxSigma")))
      std::cerr << "Note: [" << sec << "] DSPLevels / minSigma / maxSigma are stored and never used by the reference; no effect (domain-size pooling: [SIFTDescriptor] domainSizePooling = 1)" << std::endl;
    st.fginn_ratio = 0.0;
    if (it.Has(sec, "TiltSet") && it.Has(sec, "ScaleSet")) {
      const std::vector<double> tilts = it.GetDoubleVector(sec, "TiltSet"), scales = it.GetDoubleVector(sec, "ScaleSet");
      if (tilts.size() > 8 || scales.size() > 8) { std::cerr << sec << ": at most 8 tilts and 8 scales per step" << std::endl; return 1; }
      st.n_tilts = (int)tilts.size(); st.n_scales = (int)scales.size();
      for (size_t k = 0; k < tilts.size(); k++) st.tilt_set[k] = tilts[k];
      for (size_t k = 0; k < scales.size(); k++) st.scale_set[k] = scales[k];
      const std::vector<std::string> descs = it.GetStringVector(sec, "Descriptors");
      const std::vector<double> fginn = it.GetDoubleVector(sec, "FGINNThreshold");
      // DistanceThreshold, same order: > 0 runs MatchFLANNDistance on that descriptor's lists (correspondencebank.cpp:320-334)
      const std::vector<double> dthr = it.Has(sec, "DistanceThreshold") ? it.GetDoubleVector(sec, "DistanceThreshold") : std::vector<double>();
      bool has_root = false, has_zmq = false;
      double zmq_ratio = 0, zmq_dist = 0;
      for (size_t k = 0; k < descs.size(); k++) {
        std::string name = descs[k];
        name.erase(0, name.find_first_not_of(" \t"));
        name.erase(name.find_last_not_of(" \t") + 1);
        // a "Half*" name anywhere in the list switches the step's orientation estimate to doHalfSIFT mode for every descriptor
        // (imagerepresentation.cpp:725-731)
        if (name.find("Half") != std::string::npos) st.half_orientation = 1;
        if (name == "RootSIFT") { has_root = true; st.fginn_ratio = k < fginn.size() ? fginn[k] : 0.0; st.dist_threshold = k < dthr.size() ? dthr[k] : 0.0; }
        else if (name == "ZMQ") { has_zmq = true; zmq_ratio = k < fginn.size() ? fginn[k] : 0.0; zmq_dist = k < dthr.size() ? dthr[k] : 0.0; }
        else if (name == "HalfRootSIFT") {
          st.dist_threshold_half = k < dthr.size() ? dthr[k] : 0.0;
          // the reference indexes FGINNThreshold by the descriptor's position without a bounds check (synth-detection.cpp:221):
          // a missing entry is read past the end of the vector; it counts as 0 = "not matched" here
          if (k < fginn.size()) st.fginn_ratio_half = fginn[k];
          else std::cerr << "Warning: " << sec << ": no FGINNThreshold for HalfRootSIFT: its lists are not matched" << std::endl;
        }
        else if (!name.empty()) std::cerr << "Warning: " << sec << ": descriptor " << name << " is outside this build" << std::endl;
      }
      if (st.fginn_ratio_half != 0 && !(st.fginn_ratio_half > 0 && st.fginn_ratio_half < 1)) { std::cerr << sec << ": FGINNThreshold of HalfRootSIFT must lie in (0, 1)" << std::endl; return 1; }
      // [Matching<i>] SeparateDescriptors: only the listed descriptors are matched (correspondencebank.cpp:288-299)
      const std::string msec = "Matching" + std::to_string(i);
      if (it.Has(msec, "SeparateDescriptors")) {
        bool root_listed = false, half_listed = false;
        for (std::string name : it.GetStringVector(msec, "SeparateDescriptors")) {
          name.erase(0, name.find_first_not_of(" \t"));
          name.erase(name.find_last_not_of(" \t") + 1);
          root_listed = root_listed || name == "RootSIFT" || name == "ZMQ";
          half_listed = half_listed || name == "HalfRootSIFT";
        }
        if (!half_listed) { st.fginn_ratio_half = st.fginn_ratio_half > 0 ? -1.0 : 0.0; st.dist_threshold_half = 0.0; }   // its list is left alone
        if (!root_listed && has_root) std::cerr << "Warning: " << msec << ": SeparateDescriptors does not list the step's descriptor; it is matched anyway" << std::endl;
      }
      if (has_zmq && !has_root) {      // the daemon's descriptor takes the place of RootSIFT for the whole run
        cfg->use_zmq = true; has_root = true; st.fginn_ratio = zmq_ratio; st.dist_threshold = zmq_dist;
      } else if (has_zmq) std::cerr << "Warning: " << sec << ": RootSIFT and ZMQ in one step: RootSIFT is used" << std::endl;
      if (!has_root) { std::cerr << "Warning: " << sec << " does not ask for RootSIFT; the step is skipped" << std::endl; st.n_tilts = st.n_scales = -1; }
      else if (!(st.fginn_ratio > 0 && st.fginn_ratio < 1) && !(st.dist_threshold > 0)) { std::cerr << sec << ": FGINNThreshold of RootSIFT must lie in (0, 1)" << std::endl; return 1; }
      if (st.dist_threshold < 0 || st.dist_threshold_half < 0) { std::cerr << sec << ": DistanceThreshold must be >= 0" << std::endl; return 1; }
    } else st.n_tilts = st.n_scales = -1;      // no views of this detector in this step
    if (st.n_tilts >= 0 && have_sep_det && std::find(sep_det.begin(), sep_det.end(), det_name) == sep_det.end() &&
        std::find(sep_det.begin(), sep_det.end(), std::string("All")) == sep_det.end()) {
      if (cfg->verbose) std::cerr << sec << ": not in SeparateDetectors of [" << msec_det << "]: described, not matched" << std::endl;
      st.fginn_ratio = -1.0;
      if (st.fginn_ratio_half > 0) st.half_orientation = 1;   // still described in doHalfSIFT mode
      st.fginn_ratio_half = -1.0;
      st.dist_threshold = st.dist_threshold_half = 0.0;
    }
    all[di].push_back(st);
  }
  }
  for (int di = 0; di < kDets; di++) {
    bool any = false;
    for (const mods_ladder_step &st : all[di]) any = any || st.n_tilts >= 0;
    if (!any) continue;
    cfg->det_names.push_back(ss_detectors[di].name);
    cfg->det_params.push_back(di == 2 ? p.det : ss_detectors[di].type == MODS_DET_MSER ? read_mser() : read_det(ss_detectors[di].name, ss_detectors[di].type));
  }
  const int n_det = (int)cfg->det_names.size();
  for (int i = 0; i < cfg->max_steps; i++)
    for (int di = 0, d = 0; di < kDets; di++) {
      if (d < n_det && cfg->det_names[d] == ss_detectors[di].name) { cfg->steps.push_back(all[di][i]); d++; }
    }
  // grouped matching: thresholds are the [Matching]-wide ones (io_mods.cpp:448-452), the detector order is the order named
  auto trimmed = [](std::string name) { name.erase(0, name.find_first_not_of(" \t")); name.erase(name.find_last_not_of(" \t") + 1); return name; };
  bool any_group = false;
  std::vector<mods_ladder_group> groups((size_t)cfg->max_steps);
  for (int i = 0; i < cfg->max_steps; i++) {
    mods_ladder_group &g = groups[i];
    memset(&g, 0, sizeof(g));
    g.fginn_ratio = g.fginn_ratio_half = -1.0;
    const std::string msec = "Matching" + std::to_string(i);
    if (!it.Has(msec, "GroupDetectors") || !it.Has(msec, "GroupDescriptors")) continue;
    for (const std::string &raw : it.GetStringVector(msec, "GroupDetectors")) {
      const std::string name = trimmed(raw);
      if (name.empty()) continue;
      const auto at = std::find(cfg->det_names.begin(), cfg->det_names.end(), name);
      if (at == cfg->det_names.end()) { std::cerr << "Warning: [" << msec << "] GroupDetectors: " << name << " has no views in this build's steps, left out of the group" << std::endl; continue; }
      if (g.n_dets < 8) g.dets[g.n_dets++] = (int)(at - cfg->det_names.begin());
    }
    bool any_desc = false;
    for (const std::string &raw : it.GetStringVector(msec, "GroupDescriptors")) {
      const std::string name = trimmed(raw);
      if (name == "RootSIFT" || (name == "ZMQ" && cfg->use_zmq)) {
        g.fginn_ratio = ini.GetDouble("Matching", "matchRatio" + name, 0.0); g.dist_threshold = ini.GetDouble("Matching", "matchDistance" + name, 0.0); any_desc = true;
      } else if (name == "HalfRootSIFT") {
        g.fginn_ratio_half = ini.GetDouble("Matching", "matchRatioHalfRootSIFT", 0.0); g.dist_threshold_half = ini.GetDouble("Matching", "matchDistanceHalfRootSIFT", 0.0); any_desc = true;
      } else if (!name.empty()) std::cerr << "Warning: [" << msec << "] GroupDescriptors: " << name << " is outside this build" << std::endl;
    }
    if (!any_desc || g.n_dets == 0) { g.n_dets = 0; continue; }
    if ((g.fginn_ratio > 0 && !(g.fginn_ratio < 1)) || (g.fginn_ratio_half > 0 && !(g.fginn_ratio_half < 1))) { std::cerr << "[Matching] matchRatio* must lie in (0, 1)" << std::endl; return 1; }
    any_group = true;
  }
  if (cfg->mutual_check && cfg->verbose) {
    bool by_distance = false;
    for (const mods_ladder_step &st : cfg->steps) by_distance = by_distance || (st.n_tilts >= 0 && (st.dist_threshold > 0 || st.dist_threshold_half > 0));
    for (const mods_ladder_group &g : groups) by_distance = by_distance || (g.n_dets > 0 && (g.dist_threshold > 0 || g.dist_threshold_half > 0));
    if (by_distance) std::cerr << "Note: [Matching] mutualCheck: lists matched by DistanceThreshold are not checked" << std::endl;
  }
  if (any_group) {
    cfg->groups = groups;
    cfg->group_pos = 0;
    for (const std::string &nm : cfg->det_names) if (nm < std::string("Group")) cfg->group_pos++;
  }
  return 0;
}

int usage() {
  std::cerr << " ************************************************************************** " << std::endl
            << " **** mods: two-view matching with view synthesis, MI355X build        **** " << std::endl
            << " ************************************************************************** " << std::endl
            << "Usage: mods img1 img2 out1 out2 k1 k2 matchings log [logOnly=1] [ver_type=0] [H/F file] [config.ini] [iters.ini]" << std::endl
            << "  img1, img2   PNG or binary PGM/PPM" << std::endl
            << "  out1, out2   match images (PNG), written with logOnly=0 when [ImageOutput] writeImages = 1" << std::endl
            << "  k1, k2       keypoint + descriptor files (text)" << std::endl
            << "  matchings    verified correspondences, x1 y1 x2 y2 per line" << std::endl
            << "  log          one line: time matches tentatives inlier% regions1 regions2 steps" << std::endl
            << "  ver_type     0 LO-RANSAC homography, 1 ground-truth homography (read from the H/F file), 2 LO-RANSAC (DEGENSAC) epipolar geometry" << std::endl;
  return 1;
}

bool load_grey(const std::string &fn, int load_color, GreyImage *img) {
  std::string err;
  if (!modscli::read_image(fn, load_color != 0, img, &err)) { std::cerr << err << std::endl; return false; }
  return true;
}

bool save_canvas(mods_canvas *cv, const std::string &fn) {
  std::vector<unsigned char> rgb((size_t)mods_canvas_width(cv) * mods_canvas_height(cv) * 3);
  if (mods_canvas_fetch(cv, rgb.data())) { std::cerr << "mods: " << fn << ": " << mods_last_error() << std::endl; return false; }
  std::string err;
  if (!modscli::write_png_rgb(fn, rgb.data(), mods_canvas_width(cv), mods_canvas_height(cv), &err)) { std::cerr << err << std::endl; return false; }
  return true;
}

// The images of mods.cpp:452-505 over the decoded 8-bit images.  `regions`: the contours of the accumulated banks (one per described
// region; the reference shows its unoriented list, which is not kept here) go under the matches.  fn1 / fn2 empty: no match images
bool draw_outputs(mods_ctx *ctx, const GreyImage &img1, const GreyImage &img2, const std::vector<mods_imgrep *> &reps1,
                  const std::vector<mods_imgrep *> &reps2, bool regions, int region_thickness, bool with_matches, const std::vector<double> &laf,
                  const mods_draw_matches_params &par, const std::string &fn1, const std::string &fn2, bool verbose) {
  mods_canvas *src[2] = {nullptr, nullptr}, *out[2] = {nullptr, nullptr};
  const GreyImage *img[2] = {&img1, &img2};
  const std::vector<mods_imgrep *> *reps[2] = {&reps1, &reps2};
  bool ok = true;
  int dropped = 0;
  for (int i = 0; i < 2 && ok; i++) {
    ok = !mods_canvas_create(ctx, img[i]->w, img[i]->h, &src[i]) && !mods_canvas_blit_u8(src[i], img[i]->u8.data(), img[i]->w, img[i]->h, img[i]->ch, 0, 0);
    if (regions)
      for (size_t d = 0; d < reps[i]->size() && ok; d++) {
        int nd = 0;
        ok = !mods_canvas_draw_regions(src[i], (*reps[i])[d], 0, mods_imgrep_count((*reps[i])[d]), 0, 0, region_thickness, 0xa0ffffu,
                                       MODS_DRAW_TABLE_REGIONS, &nd);
        dropped += nd;
      }
  }
  if (ok && with_matches) {
    int nd[2] = {0, 0};
    ok = !mods_draw_matches(ctx, src[0], src[1], laf.data(), (int)(laf.size() / 14), &par, &out[0], &out[1], nd);
    dropped += nd[0] + nd[1];
  }
  if (!ok) std::cerr << "mods: drawing: " << mods_last_error() << std::endl;
  if (ok) ok = save_canvas(with_matches ? out[0] : src[0], fn1) && save_canvas(with_matches ? out[1] : src[1], fn2);
  if (ok && dropped && verbose) std::cerr << dropped << " drawing elements outside the coordinate range were left out" << std::endl;
  for (int i = 0; i < 2; i++) { mods_canvas_destroy(src[i]); mods_canvas_destroy(out[i]); }
  return ok;
}

// SaveRegions, imagerepresentation.cpp:1219-1255: the detectors in name order (the region map's key order), one descriptor list each
void write_regions(const std::string &fn, const std::vector<mods_imgrep *> &reps, const std::vector<std::string> &det_names, const char *desc_name) {
  std::ofstream kp(fn);
  if (!kp.is_open()) { std::cerr << "Cannot open file " << fn << " to save keypoints" << std::endl; return; }
  kp << reps.size() << std::endl;
  for (size_t d = 0; d < reps.size(); d++) {
    const int n = mods_imgrep_count(reps[d]);
    std::vector<mods_region> regs((size_t)std::max(n, 1));
    if (n > 0 && mods_imgrep_fetch(reps[d], 0, n, regs.data())) { std::cerr << mods_last_error() << std::endl; return; }
    kp << det_names[d] << " " << 1 << std::endl;
    kp << desc_name << " " << n << std::endl;
    if (n > 0) kp << 128 << std::endl;
    for (int i = 0; i < n; i++) {
      const mods_region &r = regs[i];
      kp << r.x << " " << r.y << " " << r.s << " " << r.a11 << " " << r.a12 << " " << r.a21 << " " << r.a22;
      kp << " " << 128 << " ";
      for (int j = 0; j < 128; j++) kp << (float)r.desc[j] << " ";
      kp << std::endl;
    }
  }
}

// SaveRegionsNPZ, imagerepresentation.cpp:1257-1316: xy, scales, responses, A (reproj_kp, doubles) and descs (uchar)
bool write_regions_npz(const std::string &fn, const std::vector<mods_imgrep *> &reps) {
  int n = 0;
  for (mods_imgrep *rep : reps) n += mods_imgrep_count(rep);
  std::vector<mods_region> regs((size_t)std::max(n, 1));
  for (size_t d = 0, at = 0; d < reps.size(); d++) {      // all detectors, in name order, in one set of arrays (:1257-1316)
    const int nd = mods_imgrep_count(reps[d]);
    if (nd > 0 && mods_imgrep_fetch(reps[d], 0, nd, regs.data() + at)) { std::cerr << mods_last_error() << std::endl; return false; }
    at += (size_t)nd;
  }
  modscli::NpyArray xy, sc, rs, A, ds;
  auto f8 = [&](modscli::NpyArray &a, size_t cols) { a.descr = "<f8"; a.shape = {(size_t)n, cols}; a.data.resize(sizeof(double) * n * cols); };
  f8(xy, 2); f8(sc, 1); f8(rs, 1); f8(A, 4);
  ds.descr = "|u1"; ds.shape = {(size_t)n, 128}; ds.data.resize((size_t)n * 128);
  for (int i = 0; i < n; i++) {
    const mods_region &r = regs[i];
    const double v2[2] = {r.x, r.y}, v4[4] = {r.a11, r.a12, r.a21, r.a22};
    memcpy(&xy.data[sizeof(double) * 2 * i], v2, sizeof(v2));
    memcpy(&sc.data[sizeof(double) * i], &r.s, sizeof(double));
    memcpy(&rs.data[sizeof(double) * i], &r.response, sizeof(double));
    memcpy(&A.data[sizeof(double) * 4 * i], v4, sizeof(v4));
    memcpy(&ds.data[(size_t)128 * i], r.desc, 128);
  }
  std::string err;
  if (!modscli::npz_write(fn, {{"xy", xy}, {"scales", sc}, {"responses", rs}, {"A", A}, {"descs", ds}}, &err)) { std::cerr << err << std::endl; return false; }
  return true;
}

// A built-in network from the arrays `<prefix>.features.N.*` of a weights file written with np.savez (the names of the daemon's
// --weights FILE.npz), in network order; every missing or misshapen array is an error that names it
mods_net *load_net(int device, int kind, int precision, const std::string &prefix, std::string fn) {
  while (!fn.empty() && (isspace((unsigned char)fn.back()) || fn.back() == ';')) fn.pop_back();
  static std::map<std::string, std::map<std::string, modscli::NpyArray>> files;      // one file usually serves all three sections
  if (!files.count(fn)) {
    std::string err;
    std::map<std::string, modscli::NpyArray> z;
    if (!modscli::npz_read(fn, &z, &err)) { std::cerr << "mods: weights file: " << err << " (write it with numpy.savez, not savez_compressed)" << std::endl; return nullptr; }
    files[fn] = std::move(z);
  }
  const std::map<std::string, modscli::NpyArray> &z = files[fn];
  std::vector<std::string> names;
  for (int l = 0; l < 6; l++) {
    names.push_back("features." + std::to_string(3 * l) + ".weight");
    names.push_back("features." + std::to_string(3 * l + 1) + ".running_mean");
    names.push_back("features." + std::to_string(3 * l + 1) + ".running_var");
  }
  names.push_back("features.19.weight");
  if (kind == MODS_NET_HARDNET) { names.push_back("features.20.running_mean"); names.push_back("features.20.running_var"); }
  else names.push_back("features.19.bias");
  std::vector<const float *> ptr;
  std::vector<size_t> cnt;
  std::string missing;
  for (const std::string &nm : names) {
    const auto it = z.find(prefix + "." + nm);
    if (it == z.end()) { missing += (missing.empty() ? "" : ", ") + prefix + "." + nm; continue; }
    if (it->second.descr != "<f4") { std::cerr << "mods: " << fn << ": array " << prefix << "." << nm << " is " << it->second.descr << ", float32 expected" << std::endl; return nullptr; }
    ptr.push_back((const float *)it->second.data.data());
    cnt.push_back(it->second.count());
  }
  if (!missing.empty()) { std::cerr << "mods: " << fn << " has no arrays " << missing << std::endl; return nullptr; }
  mods_net *net = nullptr;
  if (mods_net_create_ex(device, kind, ptr.data(), cnt.data(), (int)ptr.size(), precision, &net)) {
    std::cerr << "mods: " << fn << " (" << prefix << ".*): " << mods_last_error() << std::endl;
    return nullptr;
  }
  return net;
}

// The descriptors of a comma-separated list of keypoint files (member descs, (n, 128) u1, as SaveRegionsNPZ writes it), in the order
// given, for a distractor database; `key` names the configuration key in the messages
bool read_distractor_descs(const std::string &list, const char *key, std::vector<unsigned char> *out) {
  out->clear();
  size_t at = 0;
  while (at <= list.size()) {
    size_t end = list.find(',', at);
    if (end == std::string::npos) end = list.size();
    std::string fn = list.substr(at, end - at);
    at = end + 1;
    while (!fn.empty() && isspace((unsigned char)fn.back())) fn.pop_back();
    while (!fn.empty() && isspace((unsigned char)fn.front())) fn.erase(fn.begin());
    if (fn.empty()) continue;
    std::map<std::string, modscli::NpyArray> z;
    std::string err;
    if (!modscli::npz_read(fn, &z, &err)) { std::cerr << "[Matching] " << key << ": " << fn << ": " << err << std::endl; return false; }
    if (!z.count("descs")) { std::cerr << "[Matching] " << key << ": " << fn << ": no array descs" << std::endl; return false; }
    const modscli::NpyArray &ds = z["descs"];
    if (ds.descr != "|u1" || ds.shape.size() != 2) { std::cerr << "[Matching] " << key << ": " << fn << ": descs must be uint8 (n x 128)" << std::endl; return false; }
    if (ds.shape[1] != 128) {
      std::cerr << "[Matching] " << key << ": " << fn << ": descriptors of dimension " << ds.shape[1] << " (a distractor database holds 128-byte descriptors)" << std::endl;
      return false;
    }
    out->insert(out->end(), (const unsigned char *)ds.data.data(), (const unsigned char *)ds.data.data() + ds.shape[0] * 128);
  }
  return true;
}

// PreLoadRegionsNPZ, imagerepresentation.cpp:1355-1503: xy, scales, responses, descs and either A, angles (degrees) or neither
// (upright circles); det_kp = reproj_kp
bool read_regions_npz(const std::string &fn, std::vector<mods_region> *out) {
  std::map<std::string, modscli::NpyArray> z;
  std::string err;
  if (!modscli::npz_read(fn, &z, &err)) { std::cerr << err << std::endl; return false; }
  for (const char *key : {"xy", "scales", "responses", "descs"})
    if (!z.count(key)) { std::cerr << fn << ": no array " << key << std::endl; return false; }
  const modscli::NpyArray &xy = z["xy"], &sc = z["scales"], &rs = z["responses"], &ds = z["descs"];
  if (xy.descr != "<f8" || sc.descr != "<f8" || rs.descr != "<f8" || ds.descr != "|u1" || xy.shape.empty() || ds.shape.size() != 2) {
    std::cerr << fn << ": xy / scales / responses must be float64 and descs uint8 (n x dim)" << std::endl; return false;
  }
  const size_t n = xy.shape[0];
  if (ds.shape[1] != 128) { std::cerr << fn << ": descriptors of dimension " << ds.shape[1] << " (this build matches 128-byte descriptors)" << std::endl; return false; }
  if (xy.count() != 2 * n || sc.count() != n || rs.count() != n || ds.shape[0] != n) { std::cerr << fn << ": array lengths differ" << std::endl; return false; }
  const double *pxy = (const double *)xy.data.data(), *psc = (const double *)sc.data.data(), *prs = (const double *)rs.data.data();
  const double *pA = nullptr, *pang = nullptr;
  if (z.count("A")) { if (z["A"].descr != "<f8" || z["A"].count() != 4 * n) { std::cerr << fn << ": bad A" << std::endl; return false; } pA = (const double *)z["A"].data.data(); }
  else if (z.count("angles")) { if (z["angles"].descr != "<f8" || z["angles"].count() != n) { std::cerr << fn << ": bad angles" << std::endl; return false; } pang = (const double *)z["angles"].data.data(); }
  out->assign(n, mods_region());
  for (size_t i = 0; i < n; i++) {
    mods_region &r = (*out)[i];
    memset(&r, 0, sizeof(r));
    r.x = pxy[2 * i]; r.y = pxy[2 * i + 1]; r.s = psc[i]; r.response = prs[i];
    if (pA) { r.a11 = pA[4 * i]; r.a12 = pA[4 * i + 1]; r.a21 = pA[4 * i + 2]; r.a22 = pA[4 * i + 3]; }
    else {
      const double angle = pang ? pang[i] * M_PI / 180.0 : 0.0;
      r.a11 = cos(angle); r.a12 = sin(angle); r.a21 = -sin(angle); r.a22 = cos(angle);
    }
    r.id = (int)i; r.parent = -1;
    memcpy(r.desc, &ds.data[(size_t)128 * i], 128);
  }
  return true;
}

// ImageRepresentation::LoadRegions, imagerepresentation.cpp:1317-1354: the text keypoint file.  Header as SaveRegions writes
// it (number of detectors; per detector: name, number of descriptors; per descriptor: name, number of regions, dimension),
// rows as loadAR reads them (:241-253: id img_id img_reproj_id parent_id, det_kp and reproj_kp as "x y a11 a12 a21 a22
// pyramid_scale octave_number s sub_type", dimension, values).  The reference's own SaveRegions writes a different row
// (saveAR, :198-204: "x y s a11 a12 a21 a22 dimension values", the file this program writes too), which its LoadRegions cannot
// read back; both row forms are accepted here, told apart by the number of values on the first row.  The regions of the first
// 128-value descriptor list of the HessianAffine detector (or of the first detector) are returned.
bool read_regions_txt(const std::string &fn, std::vector<mods_region> *out) {
  std::ifstream f(fn);
  if (!f.is_open()) { std::cerr << "Cannot open file " << fn << " to load keypoints" << std::endl; return false; }
  int n_det = 0;
  if (!(f >> n_det) || n_det < 0 || n_det > 64) { std::cerr << fn << ": not a keypoint file" << std::endl; return false; }
  out->clear();
  bool have = false;
  for (int d = 0; d < n_det; d++) {
    std::string det_name;
    int n_desc = 0;
    if (!(f >> det_name >> n_desc) || n_desc < 0 || n_desc > 64) { std::cerr << fn << ": bad detector header" << std::endl; return false; }
    for (int k = 0; k < n_desc; k++) {
      std::string desc_name;
      long n = 0, dim = 0;
      if (!(f >> desc_name >> n) || n < 0 || n > (1 << 24)) { std::cerr << fn << ": bad descriptor header" << std::endl; return false; }
      if (n > 0 && (!(f >> dim) || dim < 0 || dim > 4096)) { std::cerr << fn << ": bad descriptor dimension" << std::endl; return false; }
      std::string rest;
      std::getline(f, rest);
      const bool take = !have && dim == 128 && (det_name == "HessianAffine" || d == 0) && desc_name != "HalfRootSIFT";
      for (long i = 0; i < n; i++) {
        std::string line;
        if (!std::getline(f, line)) { std::cerr << fn << ": truncated (" << desc_name << ", row " << i << ")" << std::endl; return false; }
        if (!take) continue;
        std::istringstream ls(line);
        std::vector<double> v;
        double t;
        while (ls >> t) v.push_back(t);
        mods_region r;
        memset(&r, 0, sizeof(r));
        size_t dpos;
        if (v.size() == (size_t)(8 + dim)) {            // saveAR row
          r.x = v[0]; r.y = v[1]; r.s = v[2]; r.a11 = v[3]; r.a12 = v[4]; r.a21 = v[5]; r.a22 = v[6];
          if ((long)v[7] != dim) { std::cerr << fn << ": row " << i << ": dimension mismatch" << std::endl; return false; }
          dpos = 8; r.id = (int)i; r.parent = -1;
        } else if (v.size() == (size_t)(25 + dim)) {    // loadAR row: reproj_kp is what matching and verification use
          r.id = (int)v[0]; r.parent = (int)v[3];
          const double *kp = &v[14];
          r.x = kp[0]; r.y = kp[1]; r.a11 = kp[2]; r.a12 = kp[3]; r.a21 = kp[4]; r.a22 = kp[5]; r.s = kp[8]; r.sub_type = (int)kp[9];
          if ((long)v[24] != dim) { std::cerr << fn << ": row " << i << ": dimension mismatch" << std::endl; return false; }
          dpos = 25;
        } else { std::cerr << fn << ": row " << i << " of " << desc_name << " has " << v.size() << " values" << std::endl; return false; }
        for (long q = 0; q < 128; q++) {
          const double dv = v[dpos + q];
          r.desc[q] = (uint8_t)(dv <= 0 ? 0 : (dv >= 255 ? 255 : (int)(dv + 0.5)));
        }
        out->push_back(r);
      }
      if (take) have = true;
    }
  }
  if (!have) { std::cerr << fn << ": no 128-value descriptor list" << std::endl; return false; }
  return true;
}

bool read_regions_any(const std::string &fn, std::vector<mods_region> *out) {   // mods.cpp:216-229: .npz or the text format
  return ends_with(fn, ".npz") ? read_regions_npz(fn, out) : read_regions_txt(fn, out);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && std::string(argv[1]) == "--npz-echo") {   // read an .npz keypoint file and write it back (format check, no GPU involved)
    std::map<std::string, modscli::NpyArray> z;
    std::string err;
    if (!modscli::npz_read(argv[2], &z, &err)) { std::cerr << err << std::endl; return 1; }
    std::vector<std::pair<std::string, modscli::NpyArray>> members(z.begin(), z.end());
    if (!modscli::npz_write(argv[3], members, &err)) { std::cerr << err << std::endl; return 1; }
    return 0;
  }
  if (argc < Tmin) return usage();
  const double c_start = now_s();
  const std::string img1_fn = argv[1], img2_fn = argv[2], k1_fn = argv[5], k2_fn = argv[6], match_fn = argv[7], log_fn = argv[8];
  int log_only = 1, ver_type = 0;
  std::string config_fn = "config_iter.ini", iters_fn = "iters.ini";
  if (argc >= Tmin + 1) log_only = atoi(argv[Tmin]);
  if (argc >= Tmin + 2) {
    ver_type = atoi(argv[Tmin + 1]);
    if (ver_type != 0 && ver_type != 1 && ver_type != 2) {
      std::cerr << ver_type << " is wrong correspondence verification type." << std::endl
                << "Try 0 for LO-RANSAC(homography), 1 for ground truth matrix or 2 for LO-RANSAC(epipolar) (3 is not taken: [RANSAC] aContrario = 1 selects ORSA under 0 or 2)" << std::endl;
      return 1;
    }
    if (ver_type == 1 && argc < Tmin + 3) {   // io_mods.cpp:594-599
      std::cerr << "Ground truth homography file is needed for verification type 1" << std::endl;
      return 1;
    }
  }
  if (argc >= Tmin + 4) config_fn = argv[Tmin + 3];
  if (argc >= Tmin + 5) iters_fn = argv[Tmin + 4];
  const bool pre_extracted = argc >= Tmin + 6 && atoi(argv[Tmin + 5]) > 0;   // conf1.read_pre_extracted, io_mods.cpp:602
  // argv[Tmin + 6] = match_one_to_many: parsed by the reference (io_mods.cpp:603) and used nowhere; ignored here too
  Config cfg;
  memset(&cfg.pair, 0, sizeof(cfg.pair));
  if (read_config(config_fn, iters_fn, ver_type, &cfg)) return 1;
  const bool model_is_f = mods_model_kind(cfg.pair.ransac.useF) == 1;   // the verified model: F (useF 1, 2) or H (0, 3)
  if (ver_type == 1) {   // mods.cpp:89-104: the file holds the matrix row by row
    std::ifstream gf(argv[Tmin + 2]);
    double *g = cfg.pair.ransac.gtH;
    if (!gf.is_open() || !(gf >> g[0] >> g[1] >> g[2] >> g[3] >> g[4] >> g[5] >> g[6] >> g[7] >> g[8])) {
      std::cerr << "Cannot open ground truth file " << argv[Tmin + 2] << std::endl;
      return 1;
    }
  }

  GreyImage img1, img2;
  if (!load_grey(img1_fn, cfg.load_color, &img1)) { std::cerr << "Cannot read image " << img1_fn << std::endl; return 1; }
  if (!load_grey(img2_fn, cfg.load_color, &img2)) { std::cerr << "Cannot read image " << img2_fn << std::endl; return 1; }
  if (cfg.verbose) std::cerr << "Image1: " << img1.w << "x" << img1.h << ", Image2: " << img2.w << "x" << img2.h << std::endl;

  // [DetectionMask]: read as grey with the image reader, checked against the image before anything else runs
  std::vector<unsigned char> det_mask[2];
  bool masks_ignored = false;
  {
    const std::string *img_fn[2] = {&img1_fn, &img2_fn};
    const GreyImage *im[2] = {&img1, &img2};
    for (int i = 0; i < 2; i++) {
      std::string fn = cfg.mask_fn[i];
      while (!fn.empty() && isspace((unsigned char)fn.back())) fn.pop_back();
      if (fn.empty() && cfg.use_mask_files) {
        const size_t dot = img_fn[i]->find_last_of('.'), slash = img_fn[i]->find_last_of('/');
        const std::string stem = (dot != std::string::npos && (slash == std::string::npos || dot > slash)) ? img_fn[i]->substr(0, dot) : *img_fn[i];
        if (std::ifstream(stem + "_mask.png").good()) fn = stem + "_mask.png";
      }
      if (fn.empty()) continue;
      if (pre_extracted || getenv("MODS_DEVICES")) { masks_ignored = true; continue; }
      GreyImage m;
      if (!load_grey(fn, 0, &m)) { std::cerr << "Cannot read detection mask " << fn << " ([DetectionMask] mask" << i + 1 << ")" << std::endl; return 1; }
      if (m.w != im[i]->w || m.h != im[i]->h) {
        std::cerr << "Detection mask " << fn << " is " << m.w << "x" << m.h << ", image " << i + 1 << " is " << im[i]->w << "x" << im[i]->h << std::endl;
        return 1;
      }
      det_mask[i].resize(m.px.size());
      for (size_t q = 0; q < m.px.size(); q++) det_mask[i][q] = m.px[q] != 0.0f ? 255 : 0;
      if (cfg.verbose) std::cerr << "Detection mask of image " << i + 1 << ": " << fn << std::endl;
    }
    if (masks_ignored) std::cerr << "Note: [DetectionMask] is ignored in pre-extracted mode and with MODS_DEVICES" << std::endl;
  }

  // [Matching] distractorDB / distractorDBHalf: read and checked before anything else runs
  std::vector<unsigned char> distractor_descs[2];
  {
    const std::string *lists[2] = {&cfg.distractor_db, &cfg.distractor_db_half};
    const char *keys[2] = {"distractorDB", "distractorDBHalf"};
    bool ignored = false;
    for (int s = 0; s < 2; s++) {
      if (lists[s]->find_first_not_of(" \t\r\n,") == std::string::npos) continue;
      if (getenv("MODS_DEVICES")) { ignored = true; continue; }
      if (!read_distractor_descs(*lists[s], keys[s], &distractor_descs[s])) return 1;
      if (cfg.verbose) std::cerr << "[Matching] " << keys[s] << ": " << distractor_descs[s].size() / 128 << " descriptors" << std::endl;
    }
    if (ignored) std::cerr << "Note: [Matching] distractorDB / distractorDBHalf are ignored with MODS_DEVICES (the multi-GPU ladder has no distractor databases)" << std::endl;
  }

  if (mods_device_count() <= 0) { std::cerr << "mods: no MI355X / HIP device available (" << mods_last_error() << "); this build has no CPU path" << std::endl; return 1; }
  const int device = getenv("MODS_DEVICE") ? atoi(getenv("MODS_DEVICE")) : 0;
  const double diag = std::ceil(std::max(std::hypot((double)img1.w, (double)img1.h), std::hypot((double)img2.w, (double)img2.h))) + 2;
  mods_ctx *ctx = nullptr;
  const int n_det = (int)cfg.det_names.size();
  if (n_det == 0) { std::cerr << "The iterations file has no HessianAffine / DoG / HarrisAffine / MSER step with RootSIFT; nothing to do" << std::endl; return 1; }
  const bool hessian_only = n_det == 1 && cfg.det_names[0] == "HessianAffine" && cfg.groups.empty();
  std::vector<mods_imgrep *> reps1((size_t)n_det, nullptr), reps2((size_t)n_det, nullptr);
  void *d1 = nullptr, *d2 = nullptr;
  auto fail = [&](const char *what) { std::cerr << "mods: " << what << ": " << mods_last_error() << std::endl; return 1; };
  // two image slots: the same view of both images goes through one chain of launches when the images have one size.
  // One run of one pair: further contexts for the views of a step (MODS_LADDER_WORKERS) take longer to set up than they save
  setenv("MODS_LADDER_WORKERS", "1", 0);
  if (mods_ctx_create(device, (int)diag, (int)diag, 2, &ctx)) return fail("context");
  for (int i = 0; i < 2; i++)
    if (!det_mask[i].empty() && mods_ctx_detection_mask(ctx, i, det_mask[i].data(), i ? img2.w : img1.w, i ? img2.h : img1.h, i ? img2.w : img1.w))
      return fail("[DetectionMask]");
  if (cfg.mutual_check && mods_ctx_match_mutual(ctx, cfg.mutual_check)) return fail("mutualCheck");
  {
    // the context keeps its references; the creator's go at once
    mods_descdb *dbs[2] = {nullptr, nullptr};
    for (int s = 0; s < 2; s++)
      if (!distractor_descs[s].empty() && mods_descdb_create(device, distractor_descs[s].data(), (long)(distractor_descs[s].size() / 128), &dbs[s]))
        return fail(s ? "distractorDBHalf" : "distractorDB");
    const int drc = (dbs[0] || dbs[1]) ? mods_ctx_distractor_db(ctx, dbs[0], dbs[1]) : 0;
    for (int s = 0; s < 2; s++) { mods_descdb_destroy(dbs[s]); distractor_descs[s] = std::vector<unsigned char>(); }
    if (drc) return fail("distractorDB");
  }
  if (cfg.local_affine && mods_ctx_local_affine(ctx, &cfg.la_par)) return fail("[LocalAffineFiltering]");
  if (cfg.dsp && cfg.use_zmq) { std::cerr << "[SIFTDescriptor] domainSizePooling = 1 pools SIFT histograms: it cannot be combined with the [zmqDescriptor] descriptor" << std::endl; return 1; }
  if (cfg.dsp && mods_ctx_domain_pooling(ctx, cfg.dsp_scales, cfg.dsp_start, cfg.dsp_end)) return fail("domainSizePooling");
  if (cfg.spatial) {
    if (pre_extracted || getenv("MODS_DEVICES")) std::cerr << "Note: [SpatialSelection] is ignored in pre-extracted mode and with MODS_DEVICES" << std::endl;
    else {
      std::string uncovered;
      for (int d = 0; d < n_det; d++) {
        const mods_hessaff_params &dp = cfg.det_params[d];
        if (dp.detectorType == MODS_DET_MSER || (dp.mode != MODS_DET_FIXED_REG_NUMBER && dp.mode != MODS_DET_RELATIVE_REG_NUMBER))
          uncovered += (uncovered.empty() ? "" : ", ") + cfg.det_names[d];
      }
      if (!uncovered.empty() && cfg.verbose)
        std::cerr << "Note: [SpatialSelection] covers the FixedRegNumber / RelativeRegNumber steps of HessianAffine, DoG and HarrisAffine; run as before: "
                  << uncovered << std::endl;
      // mode 2: the calls the selection does not cover run without it
      if (mods_ctx_spatial_selection(ctx, 2, cfg.spatial_c)) return fail("[SpatialSelection]");
      if (cfg.verbose) std::cerr << "Spatial selection (ANMS): robustness " << cfg.spatial_c << std::endl;
    }
  }
  if (cfg.upscale) {
    if (pre_extracted || getenv("MODS_DEVICES")) std::cerr << "Note: [HessianAffine] upscaleInputImage is ignored in pre-extracted mode and with MODS_DEVICES" << std::endl;
    else {
      if (mods_ctx_upscale_input(ctx, 1)) return fail("upscaleInputImage");
      if (cfg.verbose) std::cerr << "Doubled first octave (upscaleInputImage): HessianAffine, DoG and HarrisAffine start at twice the image's size" << std::endl;
    }
  }
  if (cfg.dsp && cfg.verbose) std::cerr << "Domain-size pooling: " << cfg.dsp_scales << " domains, " << cfg.dsp_start << " .. " << cfg.dsp_end << " x mrSize" << std::endl;
  // mods.cpp:133-189: createCLAHE() (8 x 8 tiles), setClipLimit(4), on the 8-bit grey image (convertTo(CV_8UC1) of the colour average,
  // or imread's grey bytes); ImageRepresentation then takes the float of the result.  Before everything else, so that every path
  // below (one GPU, MODS_DEVICES, the ladders) sees the same pixels; the pre-extracted mode has no use for the images
  if (cfg.do_clahe && !pre_extracted) {
    const double t0 = now_s();
    const mods_clahe_params cp = {4.0, 8, 8};
    for (GreyImage *im : {&img1, &img2}) {
      std::vector<unsigned char> u8(im->px.size());
      for (size_t i = 0; i < u8.size(); i++) u8[i] = (unsigned char)std::min(std::max(std::rint(im->px[i]), 0.0f), 255.0f);
      if (mods_clahe(ctx, u8.data(), im->w, im->h, &cp, u8.data())) return fail("CLAHE");
      for (size_t i = 0; i < u8.size(); i++) im->px[i] = (float)u8[i];
    }
    if (cfg.verbose) std::cerr << " CLAHE done in " << now_s() - t0 << " seconds" << std::endl;
  }
  for (int d = 0; d < n_det; d++)
    if (mods_imgrep_create(ctx, 1 << 20, &reps1[d]) || mods_imgrep_create(ctx, 1 << 20, &reps2[d])) return fail("region banks");
  if (mods_dev_alloc(sizeof(float) * img1.px.size(), &d1) || mods_dev_alloc(sizeof(float) * img2.px.size(), &d2)) return fail("device memory");
  if (mods_dev_upload(d1, img1.px.data(), sizeof(float) * img1.px.size()) || mods_dev_upload(d2, img2.px.data(), sizeof(float) * img2.px.size())) return fail("upload");

  // one HessianAffine detector (the MODS_DEVICES path takes this form): steps without views are dropped from the ladder but
  // still count as steps of the loop
  std::vector<mods_ladder_step> steps;
  std::vector<int> step_index;
  if (hessian_only)
    for (size_t i = 0; i < cfg.steps.size(); i++)
      if (cfg.steps[i].n_tilts >= 0) { steps.push_back(cfg.steps[i]); step_index.push_back((int)i); }
  if (cfg.verbose) {
    std::cerr << "Detectors:";
    for (const std::string &nm : cfg.det_names) std::cerr << " " << nm;
    std::cerr << "; " << cfg.steps.size() / n_det << " step(s), minMatches = " << cfg.min_matches << std::endl;
  }
  double first_ratio = 0.8;
  for (const mods_ladder_step &st : cfg.steps) if (st.n_tilts >= 0 && st.fginn_ratio > 0) { first_ratio = st.fginn_ratio; break; }
  // a section with weights= serves its slot in-process: 32 x 32 patches only, rounded to 8 bits as over the wire
  mods_net *net_desc = nullptr, *net_aff = nullptr, *net_ori = nullptr;
  auto builtin = [&](const char *section, const std::string &weights, int ps, int kind, const char *name, const char *prefix, int prec, bool prec_named,
                     mods_net **net) {
    if (ps != 32) { std::cerr << "mods: [" << section << "] weights= runs the network in-process on 32x32 patches; patchSize=" << ps << " is not supported" << std::endl; return false; }
    if (cfg.verbose)
      std::cerr << "[" << section << "]: " << name << " in-process" << (prec_named ? (prec == MODS_NET_BF16 ? " (precision bf16)" : " (precision fp32)") : "")
                << ", weights from " << weights << std::endl;
    *net = load_net(device, kind, prec, prefix, weights);
    return *net != nullptr;
  };
  if (cfg.use_zmq && !cfg.zmq_weights.empty()) {
    if (!builtin("zmqDescriptor", cfg.zmq_weights, cfg.zmq_ps, MODS_NET_HARDNET, "HardNet", "hardnet", cfg.zmq_prec, cfg.zmq_prec_named, &net_desc)) return 1;
    if (mods_ctx_set_builtin_descriptor(ctx, net_desc, cfg.zmq_mr, 1)) return fail("built-in descriptor");
  } else if (cfg.use_zmq) {
    while (!cfg.zmq_port.empty() && isspace((unsigned char)cfg.zmq_port.back())) cfg.zmq_port.pop_back();
    if (cfg.verbose) std::cerr << "Descriptors from the daemon at " << cfg.zmq_port << " (" << cfg.zmq_ps << "x" << cfg.zmq_ps << " patches)" << std::endl;
    if (mods_ctx_set_external_descriptor(ctx, &mods_zmq_descriptor_hook, (void *)cfg.zmq_port.c_str(), cfg.zmq_mr, cfg.zmq_ps)) return fail("external descriptor");
  }
  auto rtrim = [](std::string &t) { while (!t.empty() && isspace((unsigned char)t.back())) t.pop_back(); };
  if (cfg.aff_zmq && cfg.pair.det.doBaumberg) std::cerr << "Warning: [AffineAdaptation] useZMQ=1 with doBaumberg=1 in [HessianAffine]: the Baumberg frames are replaced" << std::endl;
  if (cfg.aff_zmq && !cfg.aff_weights.empty()) {
    if (!builtin("AffNet", cfg.aff_weights, cfg.aff_ps, MODS_NET_AFFNET, "AffNet", "affnet", cfg.aff_prec, cfg.aff_prec_named, &net_aff)) return 1;
    if (mods_ctx_set_builtin_shape(ctx, net_aff, cfg.aff_mr, 1)) return fail("built-in shape");
  } else if (cfg.aff_zmq) {
    rtrim(cfg.aff_port);
    if (cfg.verbose) std::cerr << "Affine shapes from the daemon at " << cfg.aff_port << std::endl;
    if (mods_ctx_set_external_shape(ctx, &mods_zmq_descriptor_hook, (void *)cfg.aff_port.c_str(), cfg.aff_mr, cfg.aff_ps)) return fail("external shape");
  }
  if (cfg.ori_zmq && !cfg.ori_weights.empty()) {
    if (!builtin("OriNet", cfg.ori_weights, cfg.ori_ps, MODS_NET_ORINET, "OriNet", "orinet", cfg.ori_prec, cfg.ori_prec_named, &net_ori)) return 1;
    if (mods_ctx_set_builtin_orientation(ctx, net_ori, cfg.ori_mr, 1)) return fail("built-in orientation");
  } else if (cfg.ori_zmq) {
    rtrim(cfg.ori_port);
    if (cfg.verbose) std::cerr << "Orientations from the daemon at " << cfg.ori_port << std::endl;
    if (mods_ctx_set_external_orientation(ctx, &mods_zmq_descriptor_hook, (void *)cfg.ori_port.c_str(), cfg.ori_mr, cfg.ori_ps)) return fail("external orientation");
  }
  // MODS_DEVICES=0,1,...: several GPUs for one pair (not with the ZMQ daemons: their hooks belong to one context)
  mods_multi *multi = nullptr;
  if (const char *md = getenv("MODS_DEVICES")) {
    std::vector<int> devs;
    for (const char *q = md; *q;) {
      char *e = nullptr;
      const long v = strtol(q, &e, 10);
      if (e == q) break;
      devs.push_back((int)v);
      q = *e == ',' ? e + 1 : e;
    }
    if (pre_extracted || cfg.use_zmq || cfg.aff_zmq || cfg.ori_zmq) std::cerr << "Note: MODS_DEVICES is ignored in pre-extracted mode and with ZMQ daemons" << std::endl;
    else if (!devs.empty()) {
      if (mods_multi_create(devs.data(), (int)devs.size(), std::max(img1.w, img2.w), std::max(img1.h, img2.h), 1 << 20, &multi)) return fail("multi-GPU setup");
      if (cfg.mutual_check) std::cerr << "Note: [Matching] mutualCheck is ignored with MODS_DEVICES (the queries are sharded)" << std::endl;
      if (cfg.local_affine) std::cerr << "Note: [LocalAffineFiltering] is ignored with MODS_DEVICES (the multi-GPU ladder is unfiltered)" << std::endl;
      if (cfg.dsp) std::cerr << "Note: [SIFTDescriptor] domainSizePooling is ignored with MODS_DEVICES (the devices' contexts describe unpooled)" << std::endl;
      if (cfg.verbose) std::cerr << devs.size() << " device(s), exchange over " << (mods_multi_uses_rccl(multi) ? "RCCL" : "device copies") << std::endl;
    }
  }
  mods_ladder_result res;
  std::vector<double> matches((size_t)4 << 20);
  if (pre_extracted) {   // mods.cpp:196-229: one step, the banks come from the keypoint files
    std::vector<mods_region> r1, r2;
    if (!read_regions_any(k1_fn, &r1) || !read_regions_any(k2_fn, &r2)) return 1;
    if (cfg.verbose) std::cerr << "Pre-extracted regions: " << r1.size() << " | " << r2.size() << std::endl;
    if ((!r1.empty() && mods_imgrep_append_host(reps1[0], r1.data(), (int)r1.size())) || (!r2.empty() && mods_imgrep_append_host(reps2[0], r2.data(), (int)r2.size())))
      return fail("region banks");
    if (mods_match_verify_reps(ctx, reps1[0], reps2[0], first_ratio, &cfg.pair, &res, matches.data(), 1 << 20)) return fail("matching");
    res.n_unoriented[0] = (int)r1.size(); res.n_unoriented[1] = (int)r2.size();
  } else if (multi) {   // MODS_DEVICES: the views of every step sharded over several GPUs, one all-gather of the regions per step
    // (every detector, descriptor list and group of the configuration: the step loop of mods_match_ladder_groups_dev)
    if (mods_match_ladder_groups_multi(multi, img1.px.data(), img1.w, img1.h, img2.px.data(), img2.w, img2.h, cfg.steps.data(), cfg.det_params.data(),
                                       cfg.groups.empty() ? nullptr : cfg.groups.data(), cfg.group_pos, (int)cfg.steps.size() / n_det, n_det,
                                       cfg.min_matches, &cfg.pair, &res, matches.data(), 1 << 20))
      return fail("matching");
    for (int d = 0; d < n_det; d++) {      // for the keypoint files; owned by `multi`
      mods_imgrep_destroy(reps1[d]); mods_imgrep_destroy(reps2[d]);
      reps1[d] = mods_multi_bank_det(multi, 0, d); reps2[d] = mods_multi_bank_det(multi, 1, d);
    }
  } else if (hessian_only) {
    if (steps.empty()) { res = mods_ladder_result(); }
    else if (mods_match_ladder_dev(ctx, (const float *)d1, img1.w, img1.h, (const float *)d2, img2.w, img2.h, steps.data(), (int)steps.size(),
                                   cfg.min_matches, &cfg.pair, reps1[0], reps2[0], &res, matches.data(), 1 << 20))
      return fail("matching");
  } else if (mods_match_ladder_groups_dev(ctx, (const float *)d1, img1.w, img1.h, (const float *)d2, img2.w, img2.h, cfg.steps.data(), cfg.det_params.data(),
                                          cfg.groups.empty() ? nullptr : cfg.groups.data(), cfg.group_pos, (int)cfg.steps.size() / n_det, n_det, cfg.min_matches,
                                          &cfg.pair, reps1.data(), reps2.data(), &res, matches.data(), 1 << 20))
    return fail("matching");
  // [Matching] rematchUnderH: the second stage under the H the step loop verified (mods_rematch_under_h_dev); the matches, the H
  // file, the log counts and the images below are that pass's
  int rematch_added[2] = {0, 0}, rematch_before = -1;
  if (cfg.rematch) {
    if (pre_extracted || multi) std::cerr << "Note: [Matching] rematchUnderH is ignored in pre-extracted mode and with MODS_DEVICES" << std::endl;
    else if (ver_type != 0 || cfg.pair.ransac.useF != 0)
      std::cerr << "Note: [Matching] rematchUnderH is ignored unless LO-RANSAC verifies a homography (verification type 0, aContrario = 0)" << std::endl;
    else if (!hessian_only) std::cerr << "Note: [Matching] rematchUnderH is ignored with several detectors or groups (it extends the one HessianAffine bank)" << std::endl;
    else {
      bool have_h = res.n_inliers > 0 && res.steps_done > 0;
      bool all_m1 = true;
      for (int i = 0; i < 9; i++) { if (!std::isfinite(res.H[i])) have_h = false; if (res.H[i] != -1.0) all_m1 = false; }
      if (!have_h || all_m1) { if (cfg.verbose) std::cerr << "Rematch under H: no verified model, skipped" << std::endl; }
      else {
        const mods_ladder_step &last = steps[(size_t)res.steps_done - 1];
        const int n1 = mods_imgrep_count(reps1[0]), n2 = mods_imgrep_count(reps2[0]);
        mods_ladder_result again;
        if (mods_rematch_under_h_dev(ctx, (const float *)d1, img1.w, img1.h, (const float *)d2, img2.w, img2.h, res.H, cfg.rematch == 2, last.initSigma,
                                     last.doBlur, &cfg.pair, reps1[0], reps2[0], first_ratio, &again, matches.data(), 1 << 20))
          return fail("rematchUnderH");
        rematch_added[0] = mods_imgrep_count(reps1[0]) - n1; rematch_added[1] = mods_imgrep_count(reps2[0]) - n2;
        rematch_before = res.n_inliers;
        res.n_described[0] = again.n_described[0]; res.n_described[1] = again.n_described[1];
        res.n_tentatives = again.n_tentatives; res.n_unique = again.n_unique; res.n_inliers = again.n_inliers;
        res.ransac_samples = again.ransac_samples; res.ransac_lo = again.ransac_lo; res.ransac_rejects = again.ransac_rejects;
        for (int i = 0; i < 9; i++) res.H[i] = again.H[i];
        res.ms_match += again.ms_match; res.ms_duplicates += again.ms_duplicates; res.ms_ransac += again.ms_ransac;
      }
    }
  }
  // [Matching] guidedMatching = 1: the banks of every detector, in detector order, searched again under the verified model; the
  // joint list goes through the duplicate filter and replaces the rows of the matches file (the log rows stay the reference's)
  int n_guided = -1, n_guided_unique = 0;
  {
    bool have_model = res.n_inliers > 0;
    for (int i = 0; i < 9 && have_model; i++) if (!std::isfinite(res.H[i])) have_model = false;
    bool all_m1 = true;
    for (int i = 0; i < 9; i++) if (res.H[i] != -1.0) all_m1 = false;
    if (cfg.guided && multi) std::cerr << "Note: guidedMatching is not run with MODS_DEVICES" << std::endl;
    else if (cfg.guided && have_model && !all_m1) {
      mods_guided_params gp;
      memset(&gp, 0, sizeof(gp));
      gp.model_type = model_is_f ? 1 : 0;
      for (int i = 0; i < 9; i++) gp.model[i] = res.H[i];
      gp.radius = cfg.guided_radius; gp.ratio = cfg.guided_ratio; gp.contradDist = cfg.pair.contradDist;
      gp.max_dist = cfg.guided_max_dist; gp.one_to_one = cfg.guided_one_to_one;
      std::vector<mods_tentative> gt;
      std::vector<double> gu, gl;
      for (int d = 0; d < n_det; d++) {
        const int cap = mods_imgrep_count(reps1[d]);
        if (cap <= 0 || mods_imgrep_count(reps2[d]) <= 0) continue;
        const size_t at = gt.size();
        gt.resize(at + cap); gu.resize((at + cap) * 6); gl.resize((at + cap) * 14);
        int m = 0;
        if (mods_match_guided_reps(ctx, reps1[d], reps2[d], &gp, gt.data() + at, gu.data() + at * 6, gl.data() + at * 14, cap, &m)) return fail("guided matching");
        gt.resize(at + m); gu.resize((at + m) * 6); gl.resize((at + m) * 14);
      }
      n_guided = (int)gt.size();
      n_guided_unique = n_guided;
      if (n_guided > 0 && mods_duplicate_filter_gpu(ctx, gt.data(), gu.data(), gl.data(), n_guided, cfg.pair.dup_dist, cfg.pair.dup_mode, &n_guided_unique, nullptr))
        return fail("guided matching: duplicate filter");
      if ((size_t)n_guided_unique * 4 > matches.size()) matches.resize((size_t)n_guided_unique * 4);
      for (int i = 0; i < n_guided_unique; i++) {
        matches[4 * (size_t)i] = gu[6 * (size_t)i]; matches[4 * (size_t)i + 1] = gu[6 * (size_t)i + 1];
        matches[4 * (size_t)i + 2] = gu[6 * (size_t)i + 3]; matches[4 * (size_t)i + 3] = gu[6 * (size_t)i + 4];
      }
    } else if (cfg.guided && cfg.verbose) std::cerr << "Guided matching: no verified model, skipped" << std::endl;
  }
  // [MatchRefinement] doRefinement = 1: the verified list, refined on the two images the run holds on the device; last of all.  The
  // rows of the matches file and the frames of the match images take the refined values (a rejected row stays as it was and
  // stays in the file), the H / F file the refit model; no count changes
  std::vector<double> refined_laf;
  int lsm_status[MODS_LSM_STATUS_COUNT] = {0}, lsm_n = -1;
  double lsm_zncc[2] = {0, 0};
  bool lsm_refit = false;
  if (cfg.refine) {
    if (pre_extracted || multi) std::cerr << "Note: [MatchRefinement] is ignored in pre-extracted mode and with MODS_DEVICES" << std::endl;
    else if (ver_type != 0 && ver_type != 2) std::cerr << "Note: [MatchRefinement] is ignored unless RANSAC or ORSA verifies (verification type 0 or 2)" << std::endl;
    else if (n_guided >= 0) std::cerr << "Note: [MatchRefinement] is ignored with guidedMatching (the matches file holds the guided list, not the verified one)" << std::endl;
    else {
      const int n = std::max(res.n_inliers, 0);
      std::vector<double> laf((size_t)14 * (size_t)std::max(n, 1)), u6((size_t)6 * (size_t)std::max(n, 1)), zb((size_t)std::max(n, 1)), za((size_t)std::max(n, 1));
      std::vector<int> st((size_t)std::max(n, 1));
      int n_laf = 0;
      if (mods_ctx_verified_lafs(ctx, laf.data(), n, &n_laf)) return fail("verified frames");
      if (n_laf != n) { std::cerr << "[MatchRefinement] " << n_laf << " verified frames for " << n << " matches" << std::endl; return 1; }
      refined_laf.resize((size_t)14 * (size_t)n);
      if (mods_refine_matches_dev(ctx, (const float *)d1, img1.w, img1.h, img1.w, (const float *)d2, img2.w, img2.h, img2.w, laf.data(), n, &cfg.lsm_par,
                                  refined_laf.data(), u6.data(), st.data(), nullptr, zb.data(), za.data()))
        return fail("[MatchRefinement]");
      lsm_n = n;
      int n_z = 0;
      for (int i = 0; i < n; i++) {
        lsm_status[st[i]]++;
        if (st[i] == MODS_LSM_OK || st[i] == MODS_LSM_MAXITER) { lsm_zncc[0] += zb[i]; lsm_zncc[1] += za[i]; n_z++; }
        matches[4 * (size_t)i] = u6[6 * (size_t)i]; matches[4 * (size_t)i + 1] = u6[6 * (size_t)i + 1];
        matches[4 * (size_t)i + 2] = u6[6 * (size_t)i + 3]; matches[4 * (size_t)i + 3] = u6[6 * (size_t)i + 4];
      }
      if (n_z) { lsm_zncc[0] /= n_z; lsm_zncc[1] /= n_z; }
      if (cfg.refit_model && n >= (model_is_f ? 8 : 4)) {
        double M[9];
        if (mods_refit_model(u6.data(), n, model_is_f ? 1 : 0, M)) return fail("[MatchRefinement] refitModel");
        for (int i = 0; i < 9; i++) res.H[i] = M[i];
        lsm_refit = true;
      }
    }
  }
  // [MatchPropagation] doPropagation = 1: after everything else, from the verified frames (the refined ones when the refinement
  // ran) under the model that goes to the H / F file; its rows go to a file of their own and nothing else changes
  std::vector<double> prop_rows;        // x1 y1 x2 y2 zncc round
  std::vector<int> prop_stats;
  int prop_n = -1, prop_trunc = 0;
  if (cfg.propagate) {
    if (pre_extracted || multi) std::cerr << "Note: [MatchPropagation] is ignored in pre-extracted mode and with MODS_DEVICES" << std::endl;
    else if (ver_type != 0 && ver_type != 2) std::cerr << "Note: [MatchPropagation] is ignored unless RANSAC or ORSA verifies (verification type 0 or 2)" << std::endl;
    else if (n_guided >= 0) std::cerr << "Note: [MatchPropagation] is ignored with guidedMatching (the verified list is not what the run ends with)" << std::endl;
    else {
      const int n = std::max(res.n_inliers, 0);
      std::vector<double> laf((size_t)14 * (size_t)std::max(n, 1));
      if (refined_laf.size() == (size_t)14 * (size_t)n && n > 0) laf = refined_laf;
      else {
        int n_laf = 0;
        if (mods_ctx_verified_lafs(ctx, laf.data(), n, &n_laf)) return fail("verified frames");
        if (n_laf != n) { std::cerr << "[MatchPropagation] " << n_laf << " verified frames for " << n << " matches" << std::endl; return 1; }
      }
      mods_propagate_params pp = cfg.prop_par;
      if (!cfg.prop_thr_set) pp.model_thr = cfg.pair.ransac.err_threshold;
      pp.model_type = -1;
      if (cfg.prop_use_model && n > 0) {
        pp.model_type = model_is_f ? 1 : 0;
        for (int i = 0; i < 9; i++) {   // the model as the H / F file will hold it: through the stream's digits
          std::ostringstream os;
          os << res.H[i];
          pp.model[i] = strtod(os.str().c_str(), nullptr);
        }
      }
      const size_t cap = (size_t)(img1.w / pp.cell) * (size_t)(img1.h / pp.cell);
      if (cap == 0 || cap > (size_t)1 << 28) { std::cerr << "[MatchPropagation] image 1 of " << img1.w << " x " << img1.h << " and cell " << pp.cell << std::endl; return 1; }
      std::vector<double> u6(6 * cap), z(cap);
      std::vector<int> rnd(cap);
      prop_stats.assign((size_t)(pp.rounds + 1) * MODS_PROP_STATUS_COUNT, 0);
      int m = 0;
      if (mods_propagate_matches_dev(ctx, (const float *)d1, img1.w, img1.h, img1.w, (const float *)d2, img2.w, img2.h, img2.w, laf.data(), n, &pp, (int)cap,
                                     nullptr, u6.data(), z.data(), nullptr, rnd.data(), nullptr, nullptr, &m, &prop_trunc, nullptr, prop_stats.data(), nullptr,
                                     nullptr))
        return fail("[MatchPropagation]");
      prop_n = m;
      prop_rows.resize((size_t)6 * (size_t)m);
      for (int i = 0; i < m; i++) {
        double *r = &prop_rows[6 * (size_t)i];
        r[0] = u6[6 * (size_t)i]; r[1] = u6[6 * (size_t)i + 1]; r[2] = u6[6 * (size_t)i + 3]; r[3] = u6[6 * (size_t)i + 4]; r[4] = z[i]; r[5] = rnd[i];
      }
    }
  }
  const int n_written = n_guided >= 0 ? n_guided_unique : res.n_inliers;
  const double final_time = now_s() - c_start;
  const int final_step = res.steps_done <= 0 ? 0 : (hessian_only && !pre_extracted && !multi) ? step_index[res.steps_done - 1] + 1 : res.steps_done;
  if (cfg.verbose) {
    std::cerr << res.n_views << " views synthesised, " << res.n_tentatives << " tentatives found." << std::endl;
    std::cerr << res.n_unique << " unique tentatives left" << std::endl;
    for (int i = 0; i < 2; i++)
      if (!det_mask[i].empty()) {
        int acc = 0, kept = 0;
        if (mods_ctx_detection_mask_counts(ctx, i, &acc, &kept)) return fail("[DetectionMask]");
        std::cerr << "Detection mask of image " << i + 1 << ": " << acc << " points accepted, " << kept << " kept" << std::endl;
      }
    if (!det_mask[0].empty() || !det_mask[1].empty()) {      // the rule itself over what is about to be written
      int on = 0;
      for (int i = 0; i < n_written; i++) {
        const double *m = &matches[4 * (size_t)i];
        on += (det_mask[0].empty() || mods_detection_mask_test(det_mask[0].data(), img1.w, img1.h, img1.w, m[0], m[1])) &&
              (det_mask[1].empty() || mods_detection_mask_test(det_mask[1].data(), img2.w, img2.h, img2.w, m[2], m[3]));
      }
      std::cerr << on << " of " << n_written << " matches have both centres on the detection masks" << std::endl;
    }
    if (cfg.local_affine && !multi) {
      int la_in = 0, la_kept = 0;
      if (mods_local_affine_counts(ctx, &la_in, &la_kept)) return fail("[LocalAffineFiltering]");
      std::cerr << "Local affine filtering (radius " << cfg.la_par.radius << "): " << la_in << " tentatives in, " << la_kept << " kept" << std::endl;
    }
    if (cfg.pair.ransac.groundTruth) {
      std::cerr << "Ground truth verification is used..." << std::endl
                << res.gt_true << " true matches got with error threshold = " << cfg.pair.ransac.err_threshold << std::endl;
      if (cfg.pair.ransac.groundTruth >= 2)
        std::cerr << "Now RANSAC" << std::endl << res.gt_ransac_inliers << " RANSAC matches are identified" << std::endl
                  << res.gt_true_of_ransac << " RANSAC true matches are identified" << std::endl;
    } else {
      static const char *const verifier[4] = {"LO-RANSAC(homography)", "LO-RANSAC(epipolar)", "ORSA(epipolar)", "ORSA(homography)"};
      std::cerr << verifier[cfg.pair.ransac.useF] << " verification is used..." << std::endl;
      if (cfg.pair.ransac.useF == 3 && !multi) {
        double thr_px = 0;
        float log_nfa = 0;
        if (!mods_orsa_h_last_threshold(&thr_px, &log_nfa))
          std::cerr << "ORSA(homography): log10(nfa) = " << log_nfa << ", inlier threshold = " << thr_px << " px" << std::endl;
      }
      std::cerr << res.n_inliers << " RANSAC correspondences got" << std::endl;
    }
    if (rematch_before >= 0) std::cerr << "Rematch under H: +" << rematch_added[0] << " | +" << rematch_added[1] << " regions, " << rematch_before
                                       << " verified before, " << res.n_inliers << " after" << std::endl;
    if (lsm_n >= 0) {
      static const char *const names[MODS_LSM_STATUS_COUNT] = {"ok", "maxiter", "bad frame", "outside", "flat", "diverged", "low zncc"};
      std::cerr << "Match refinement (radius " << cfg.lsm_par.radius << "): " << lsm_n << " correspondences:";
      for (int i = 0; i < MODS_LSM_STATUS_COUNT; i++) std::cerr << " " << lsm_status[i] << " " << names[i] << (i + 1 < MODS_LSM_STATUS_COUNT ? "," : ";");
      std::cerr << " mean zncc of the accepted " << lsm_zncc[0] << " before, " << lsm_zncc[1] << " after" << (lsm_refit ? "; model refit" : "") << std::endl;
    }
    if (prop_n >= 0) {
      std::cerr << "Match propagation (cell " << cfg.prop_par.cell << ", reach " << cfg.prop_par.reach << ", radius " << cfg.prop_par.lsm.radius << "): "
                << prop_n << " correspondences" << (prop_trunc ? " (cut)" : "") << std::endl;
      for (int r = 0; r <= cfg.prop_par.rounds; r++) {
        int tried = 0;
        for (int q = 0; q < MODS_PROP_STATUS_COUNT; q++) tried += prop_stats[(size_t)r * MODS_PROP_STATUS_COUNT + q];
        if (r > 0 && tried == 0) break;
        std::cerr << "  round " << r << ": " << tried << " rows tried, " << prop_stats[(size_t)r * MODS_PROP_STATUS_COUNT + MODS_LSM_OK] << " accepted" << std::endl;
      }
    }
    if (n_guided >= 0) std::cerr << "Guided matching (radius " << cfg.guided_radius << ", ratio " << cfg.guided_ratio << "): " << n_guided
                                 << " correspondences, " << n_guided_unique << " after duplicate filtering" << std::endl;
  }
  std::cerr << "Done in " << final_step << " iterations" << std::endl << "*********************" << std::endl;

  {   // WriteLog, io_mods.cpp:10-66
    std::ofstream lf(log_fn);
    if (lf.is_open()) {
      const double ratio = res.n_unique > 0 ? (double)res.n_inliers / (double)res.n_unique : std::nan("");
      if (cfg.pair.ransac.groundTruth) {   // GR_TRUTH / GR_PLUS_RANSAC rows of WriteLog
        const double r_all = res.n_unique > 0 ? (double)res.gt_true / (double)res.n_unique : std::nan("");
        lf << std::setprecision(3) << final_time << " ";
        if (cfg.pair.ransac.groundTruth >= 2) {
          const double r_rs = res.gt_ransac_inliers > 0 ? (double)res.gt_true_of_ransac / (double)res.gt_ransac_inliers : std::nan("");
          lf << res.gt_true_of_ransac << " " << res.gt_ransac_inliers << " " << r_rs * 100 << " ";
        }
        lf << res.gt_true << " " << res.n_unique << " " << r_all * 100 << " " << res.n_described[0] << " " << res.n_described[1] << " "
           << final_step << " " << std::endl;
      } else {
        lf << std::setprecision(3) << final_time << " " << res.n_inliers << " " << res.n_unique << " " << ratio * 100 << " ";
        if (model_is_f) lf << res.n_described[0] << " " << res.n_described[1] << " ";
        else lf << res.n_unoriented[0] << " " << res.n_unoriented[1] << " ";
        lf << final_step << " " << std::endl;
      }
    }
  }
  if (cfg.output_h && argc >= Tmin + 3) {   // WriteH
    std::ofstream hf(argv[Tmin + 2]);
    if (hf.is_open())
      hf << res.H[0] << " " << res.H[1] << " " << res.H[2] << std::endl << res.H[3] << " " << res.H[4] << " " << res.H[5] << std::endl
         << res.H[6] << " " << res.H[7] << " " << res.H[8] << std::endl;
  }
  if (prop_n >= 0) {   // [MatchPropagation] output
    std::ofstream pf(cfg.prop_output);
    if (!pf.is_open()) { std::cerr << "[MatchPropagation] cannot write " << cfg.prop_output << std::endl; return 1; }
    pf.precision(10);
    for (int i = 0; i < prop_n; i++) {
      const double *r = &prop_rows[6 * (size_t)i];
      pf << r[0] << " " << r[1] << " " << r[2] << " " << r[3] << " " << r[4] << " " << (int)r[5] << std::endl;
    }
  }
  if (!log_only) {
    if (cfg.write_matches) {
      std::ofstream mf(match_fn);
      if (mf.is_open())
        for (int i = 0; i < n_written; i++)
          mf << matches[4 * (size_t)i] << " " << matches[4 * (size_t)i + 1] << " " << matches[4 * (size_t)i + 2] << " " << matches[4 * (size_t)i + 3] << std::endl;
    }
    if (cfg.write_keypoints && !pre_extracted) {   // mods.cpp:433-447
      if (ends_with(k1_fn, ".npz")) write_regions_npz(k1_fn, reps1);
      else write_regions(k1_fn, reps1, cfg.det_names, cfg.use_zmq ? "ZMQ" : "RootSIFT");
      if (ends_with(k2_fn, ".npz")) write_regions_npz(k2_fn, reps2);
      else write_regions(k2_fn, reps2, cfg.det_names, cfg.use_zmq ? "ZMQ" : "RootSIFT");
    }
    if (cfg.write_images || cfg.draw_regions) {   // mods.cpp:452-505, over the verified list (not the guided one) and the banks
      const std::string out1_fn = argv[3], out2_fn = argv[4];
      std::vector<double> laf((size_t)14 * (size_t)std::max(res.n_inliers, 1));
      int n_laf = 0;
      if (multi ? mods_multi_verified_lafs(multi, laf.data(), res.n_inliers, &n_laf) : mods_ctx_verified_lafs(ctx, laf.data(), res.n_inliers, &n_laf))
        return fail("verified frames");
      laf.resize((size_t)14 * (size_t)std::min(n_laf, std::max(res.n_inliers, 0)));
      if (refined_laf.size() == laf.size()) laf = refined_laf;   // [MatchRefinement]: the images show the refined frames
      mods_draw_matches_params dp;
      memset(&dp, 0, sizeof(dp));
      dp.draw_only_centers = cfg.draw_only_centers;
      dp.reproject_to_one_image = !model_is_f && cfg.draw_reprojected;
      dp.draw_epipolar_lines = model_is_f && cfg.draw_epipolar;
      for (int i = 0; i < 9; i++) dp.M[i] = res.H[i];
      {   // without a usable model (no verified match: H is all -1, singular) the centres are drawn side by side
        const double *H = res.H;
        const double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
        if (dp.reproject_to_one_image && (det == 0. || !std::isfinite(det))) dp.reproject_to_one_image = 0;
      }
      if (const char *ff = getenv("MODS_DRAW_FRAMES")) {   // what the images are drawn from, to full precision: the model, then the frames
        std::ofstream fr(ff);
        fr << std::setprecision(17);
        for (int i = 0; i < 9; i++) fr << dp.M[i] << (i == 8 ? "\n" : " ");
        for (size_t i = 0; i < laf.size(); i++) fr << laf[i] << (i % 14 == 13 ? "\n" : " ");
      }
      if (cfg.write_images) {
        std::cerr << " Writing images with matches...";
        dp.r1 = 5; dp.r2 = 4;
        if (!draw_outputs(ctx, img1, img2, reps1, reps2, false, 0, true, laf, dp, out1_fn, out2_fn, cfg.verbose != 0)) return 1;
        std::cerr << " done" << std::endl;
      }
      if (cfg.draw_regions && multi) std::cerr << "Note: drawDetectedRegions is not run with MODS_DEVICES (the banks live in the devices' own contexts)" << std::endl;
      else if (cfg.draw_regions) {
        std::cerr << " Writing image with detected regions...";
        dp.r1 = 3; dp.r2 = 2;
        if (!draw_outputs(ctx, img1, img2, reps1, reps2, true, 2, false, laf, dp, out1_fn + "_reg.png", out2_fn + "_reg.png", cfg.verbose != 0)) return 1;
        if (!draw_outputs(ctx, img1, img2, reps1, reps2, true, 1, true, laf, dp, out1_fn + ".png", out2_fn + ".png", cfg.verbose != 0)) return 1;
        std::cerr << " done" << std::endl;
      }
    }
  }
  std::cerr << "Image1: regions descriptors | Image2: regions descriptors " << std::endl;
  std::cerr << res.n_unoriented[0] << " " << res.n_described[0] << " | " << res.n_unoriented[1] << " " << res.n_described[1] << std::endl << std::endl;
  std::cerr << "True matches | unique tentatives" << std::endl;
  {
    const int tm = cfg.pair.ransac.groundTruth ? res.gt_true : res.n_inliers;   // TrueMatch1st
    if (res.n_unique > 0) std::cerr << tm << " | " << res.n_unique << " | " << std::setprecision(3) << 100.0 * tm / res.n_unique << "%  1st geom inc" << std::endl;
    else std::cerr << tm << " | " << res.n_unique << " |  -  1st geom inc" << std::endl;
    if (cfg.pair.ransac.groundTruth >= 2) {   // mods.cpp:515-519
      if (res.gt_ransac_inliers > 0) std::cerr << res.gt_true_of_ransac << " | " << res.gt_ransac_inliers << " | " << std::setprecision(3)
                                               << 100.0 * res.gt_true_of_ransac / res.gt_ransac_inliers << "% RANSACed  1st geom inc" << std::endl;
      else std::cerr << res.gt_true_of_ransac << " | " << res.gt_ransac_inliers << " | -  RANSACed  1st geom inc" << std::endl;
    }
  }
  // [OverlapMatching] doOverlapMatch = 1 (mods.cpp:522-523): the banks of every detector under the ground-truth homography, one to one
  if (cfg.overlap && ver_type != 1) std::cerr << "Note: doOverlapMatch needs the ground truth homography (verification type 1), skipped" << std::endl;
  else if (cfg.overlap && multi) std::cerr << "Note: doOverlapMatch is not run with MODS_DEVICES" << std::endl;
  else if (cfg.overlap && cfg.overlap_area) {   // overlapMeasure = area: intersection over union, greedy one-to-one assignment
    mods_overlap_area_params op;
    memset(&op, 0, sizeof(op));
    for (int i = 0; i < 9; i++) op.H[i] = cfg.pair.ransac.gtH[i];
    op.max_error = cfg.overlap_area_error; op.one_to_one = 2;
    op.w1 = img1.w; op.h1 = img1.h; op.w2 = img2.w; op.h2 = img2.h;
    long n_overlap = 0;
    std::vector<mods_overlap_counts> oc((size_t)n_det);
    std::vector<mods_overlap_area_match> om;
    for (int d = 0; d < n_det; d++) {
      const int cap = mods_imgrep_count(reps1[d]);
      om.resize((size_t)std::max(cap, 1));
      int m = 0;
      if (mods_match_overlap_area_reps(ctx, reps1[d], reps2[d], &op, om.data(), cap, &m, &oc[d])) return fail("area overlap matching");
      n_overlap += m;
    }
    std::cerr << "Area overlap matches with error < " << cfg.overlap_area_error << std::endl << n_overlap << std::endl;
    if (cfg.verbose)
      for (int d = 0; d < n_det; d++)
        std::cerr << cfg.det_names[d] << ": " << oc[d].n_q_common << " | " << oc[d].n_t_common << " regions in the common area, repeatability "
                  << oc[d].repeatability << std::endl;
  } else if (cfg.overlap) {
    mods_overlap_params op;
    memset(&op, 0, sizeof(op));
    for (int i = 0; i < 9; i++) op.H[i] = cfg.pair.ransac.gtH[i];
    op.max_error = cfg.overlap_error; op.oriented = cfg.overlap_oriented; op.one_to_one = 1;
    op.w1 = img1.w; op.h1 = img1.h; op.w2 = img2.w; op.h2 = img2.h;
    long n_overlap = 0;
    std::vector<mods_overlap_counts> oc((size_t)n_det);
    std::vector<mods_overlap_match> om;
    for (int d = 0; d < n_det; d++) {
      const int cap = mods_imgrep_count(reps1[d]);
      om.resize((size_t)std::max(cap, 1));
      int m = 0;
      if (mods_match_overlap_reps(ctx, reps1[d], reps2[d], &op, om.data(), cap, &m, &oc[d])) return fail("overlap matching");
      n_overlap += m;
    }
    std::cerr << "Overlap matches with E < " << cfg.overlap_error << std::endl << n_overlap << std::endl;
    if (cfg.verbose)
      for (int d = 0; d < n_det; d++)
        std::cerr << cfg.det_names[d] << ": " << oc[d].n_q_common << " | " << oc[d].n_t_common << " regions in the common area, repeatability "
                  << oc[d].repeatability << std::endl;
  }
  const double total = now_s() - c_start;
  std::cerr << std::endl << "Main matching | All Time: " << std::endl << final_time << " | " << total << " seconds" << std::endl;
  if (cfg.time_log) {   // WriteTimeLog(TimingLog, file, 0, 1, 0): Synth Detect Orient Desc Match RANSAC MISC Total (seconds)
    const double dd = res.ms_detect_describe / 1000, mt = res.ms_match / 1000, rs = (res.ms_duplicates + res.ms_ransac) / 1000;
    std::ofstream tf("time.log");
    if (tf.is_open()) tf << 0.0 << " " << dd << " " << 0.0 << " " << 0.0 << " " << mt << " " << rs << " " << total - (dd + mt + rs) << " " << total << std::endl;
    std::cerr << "Timings: (sec) " << std::endl << "Synth+Detect+Orient+Desc|Match|RANSAC|MISC|Total " << std::endl
              << dd << " " << mt << " " << rs << " " << total - (dd + mt + rs) << " " << total << std::endl;
  }
  if (!multi) for (int d = 0; d < n_det; d++) { mods_imgrep_destroy(reps1[d]); mods_imgrep_destroy(reps2[d]); }
  mods_dev_free(d1); mods_dev_free(d2);
  mods_ctx_destroy(ctx);
  mods_net_destroy(net_desc); mods_net_destroy(net_aff); mods_net_destroy(net_ori);
  return 0;
}
