"""-m gpu parity tests of the detector stages between the scale space and the description away from the .ini's threshold,
edgeEigenValueRatio, maxIterations and convergenceThreshold: the NMS and localisation thresholds of all three detectors, the
second-moment and the Hessian form of the Baumberg iteration (also crossed with smmWindowSize and without the iteration),
NotLessThanRegions off its default threshold, parameter changes on a live context and in a batch, and the regionsNumber cut
of a tilted or shrunk view through the single-view and the paired-view entry points.  Every comparison is np.array_equal
against the CPU oracle; the keypoint counts beside the cases are the oracle's, at 203x131 / 320x240 of synth.texture(seed=7)."""
import functools
import math

import numpy as np
import pytest

import orc
import synth

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "octave", "level", "r0", "c0")   # as test_gpu_detect.py
SIZES = [(203, 131), (320, 240)]
OCTAVES = {203: 4, 320: 5}                       # border 5 (test_gpu_scale_space.py)
REGION_FIELDS = ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "desc")


def _params(mod, det="hessian", over=()):
    """The .ini section of `det` with the keys of `over` = ((name, value), ...) replaced."""
    p = {"hessian": mod.HessAffParams.default, "dog": mod.HessAffParams.dog, "harris": mod.HessAffParams.harris}[det]()
    for name, value in over:
        assert hasattr(p, name), name
        setattr(p, name, value)
    return p


def _over(**kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _image(w, h, seed):
    img = synth.texture(w, h, seed=seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _oracle_keys(w, h, seed, det="hessian", over=()):
    keys = orc.detect_hessian_affine(_image(w, h, seed), _params(orc, det, over))
    keys.setflags(write=False)
    return keys


def _assert_keys_equal(got, want):
    assert len(got) == len(want)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), "field %s differs" % f


def _same_keys(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)


def _assert_candidates_equal(ctx, pyr, img=0):
    cand_want, _ = pyr.candidates()
    cand_got = ctx.pyramid_candidates(img)
    cand_got = cand_got[np.lexsort((cand_got["c0"], cand_got["r0"], cand_got["level"], cand_got["octave"]))]
    assert len(cand_got) == len(cand_want)
    for f in cand_want.dtype.names:
        assert np.array_equal(cand_got[f], cand_want[f]), f
    return len(cand_want)


def _detect_and_compare(pkg, w, h, det, over, candidates=False, seed=7):
    """One detection on a context sized to the image against the oracle; returns (oracle keypoints, oracle candidate count)."""
    img = _image(w, h, seed)
    want = _oracle_keys(w, h, seed, det, over)
    n_cand = None
    ctx = pkg.Context(0, w, h, 1)
    try:
        got = ctx.detect_hessian_affine(img, params=_params(pkg, det, over))
        if candidates:
            pyr = orc.Pyramid(img, _params(orc, det, over))
            assert ctx.pyramid_octaves() == pyr.n_oct == OCTAVES[w]
            n_cand = _assert_candidates_equal(ctx, pyr)
        _assert_keys_equal(got, want)
    finally:
        ctx.close()
    return want, n_cand


# ---- 1. localisation thresholds ----------------------------------------------------------------------------
# (detector, overrides, sizes, oracle keypoints 203x131 / 320x240).  HessianAffine: the NMS bound is 0.8 * threshold, the final one
# threshold^2; threshold 0 in FixedTh mode leaves pos_th = neg_th = 0 with the strict comparisons of the NMS.
# edgeEigenValueRatio 1.0 is the bound 4, which no real pair of eigenvalues passes: its own test below.  The ratios are values a
# float holds exactly (mods_hessaff_params keeps a float where PyramidParams keeps a double).
LOCALISE_CASES = [
    ("hessian", _over(threshold=0.0), SIZES),                                     # 154 / 556
    ("hessian", _over(threshold=1.0), SIZES),                                     # 133 / 465
    ("hessian", _over(threshold=3.0), SIZES),                                     # 103 / 367
    ("hessian", _over(threshold=9.0), SIZES),                                     # 44 / 188
    ("hessian", _over(threshold=16.0), SIZES[1:]),                                # 15 / 60: 320x240 only
    ("hessian", _over(edgeEigenValueRatio=1.5), SIZES),                           # 46 / 153
    ("hessian", _over(edgeEigenValueRatio=2.0), SIZES),                           # 59 / 202
    ("hessian", _over(edgeEigenValueRatio=5.0), SIZES),                           # 80 / 280
    ("hessian", _over(edgeEigenValueRatio=40.0), SIZES),                          # 91 / 338
    ("hessian", _over(threshold=9.0, edgeEigenValueRatio=2.0), SIZES),            # 58 / 176 candidates, 37 / 151 keypoints
    ("dog", _over(edgeEigenValueRatio=3.0), SIZES),                               # 51 / 182
    ("harris", _over(edgeEigenValueRatio=3.0), SIZES),                            # 75 / 207
]
LOCALISE = [(det, over, w, h) for det, over, sizes in LOCALISE_CASES for (w, h) in sizes]


@pytest.mark.parametrize("det,over,w,h", LOCALISE)
def test_localisation_thresholds(pkg, det, over, w, h):
    """nms_kernel / nms4_kernel (pos_th, neg_th), localize_kernel (edge_th, final_th) and accept_kernel: octave count, pyramid
    candidates and keypoints equal the oracle's."""
    want, n_cand = _detect_and_compare(pkg, w, h, det, over, candidates=True)
    assert n_cand > 20
    assert 20 < len(want) <= n_cand


@pytest.mark.parametrize("w,h", SIZES)
def test_edge_ratio_one_gives_nothing(pkg, w, h):
    """edgeEigenValueRatio = 1: edge_th = 4 = the score of two equal eigenvalues, and the test is >=: 0 / 0 candidates and
    keypoints on both sides, and the call returns cleanly (every later stage runs on empty lists)."""
    over = _over(edgeEigenValueRatio=1.0)
    want, n_cand = _detect_and_compare(pkg, w, h, "hessian", over, candidates=True)
    assert len(want) == 0 and n_cand == 0
    assert len(orc.Pyramid(_image(w, h, 7), _params(orc, "hessian", over)).candidates()[1]) > 20      # the NMS itself found points


# ---- 2. the Baumberg iteration -----------------------------------------------------------------------------
# (detector, overrides, lower bound on the oracle's keypoints, oracle keypoints 203x131 / 320x240)
DEFAULT_BOUND = 21                                # "> 20"
BAUMBERG_CASES = [
    ("hessian", _over(maxIterations=1), 1),                                                     # 1 / 12
    ("hessian", _over(maxIterations=2), 1),                                                     # 1 / 12
    ("hessian", _over(maxIterations=3), DEFAULT_BOUND),                                         # 43 / 162
    ("hessian", _over(maxIterations=5), DEFAULT_BOUND),                                         # 76 / 283
    ("hessian", _over(maxIterations=40), DEFAULT_BOUND),                                        # 85 / 310
    ("hessian", _over(convergenceThreshold=0.005), DEFAULT_BOUND),                              # 75 / 278
    ("hessian", _over(convergenceThreshold=0.02), DEFAULT_BOUND),                               # 82 / 287
    ("hessian", _over(convergenceThreshold=0.2), DEFAULT_BOUND),                                # 107 / 347
    ("hessian", _over(convergenceThreshold=1.0), DEFAULT_BOUND),                                # 123 / 372
    ("hessian", _over(doBaumberg=0), DEFAULT_BOUND),                                            # 126 / 375 = the candidates
    # crossed with the window size (the lanes of a keypoint, the LDS layout and the sampling path follow it)
    ("hessian", _over(smmWindowSize=9, maxIterations=3), DEFAULT_BOUND),                        # 26 / 65
    ("hessian", _over(smmWindowSize=31, maxIterations=3), DEFAULT_BOUND),                       # 36 / 180
    ("hessian", _over(smmWindowSize=9, convergenceThreshold=0.2), DEFAULT_BOUND),               # 105 / 349
    ("hessian", _over(smmWindowSize=31, convergenceThreshold=0.2), DEFAULT_BOUND),              # 105 / 341
    ("hessian", _over(smmWindowSize=9, maxIterations=5, convergenceThreshold=0.02), DEFAULT_BOUND),    # 56 / 150
    ("hessian", _over(smmWindowSize=31, maxIterations=5, convergenceThreshold=0.02), DEFAULT_BOUND),   # 43 / 229
    # the Hessian form (baumberg_hessian_kernel)
    ("hessian", _over(affBmbrgMethod=1, maxIterations=3), DEFAULT_BOUND),                       # 99 / 304
    ("hessian", _over(affBmbrgMethod=1, convergenceThreshold=0.2), DEFAULT_BOUND),              # 126 / 375
    ("hessian", _over(affBmbrgMethod=1, maxIterations=40, convergenceThreshold=0.01), DEFAULT_BOUND),  # 125 / 371
    # DoG and Harris with the iteration switched on
    ("dog", _over(doBaumberg=1, maxIterations=4), DEFAULT_BOUND),                               # 26 / 149
    ("harris", _over(doBaumberg=1, maxIterations=4), DEFAULT_BOUND),                            # 64 / 235
    ("dog", _over(doBaumberg=1, convergenceThreshold=0.3), DEFAULT_BOUND),                      # 50 / 193
    ("harris", _over(doBaumberg=1, convergenceThreshold=0.3), DEFAULT_BOUND),                   # 97 / 268
]
# the key is not ignored: these differ from the default parameters' result (84 / 306 keypoints) in the oracle
DIFFERS_FROM_DEFAULT = (_over(maxIterations=3), _over(maxIterations=5), _over(maxIterations=40), _over(convergenceThreshold=0.2))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("det,over,bound", BAUMBERG_CASES)
def test_baumberg_limits(pkg, det, over, bound, w, h):
    """max_iter and conv_th of baumberg_kernel<KP> (several keypoints share a wave: one that is done idles while its neighbours
    iterate, and the loop ends with the last of them or at max_iter) and of baumberg_hessian_kernel; without the iteration the
    HessianAffine keypoints are the pyramid's candidates."""
    want, _ = _detect_and_compare(pkg, w, h, det, over)
    assert len(want) >= bound
    if over in DIFFERS_FROM_DEFAULT and det == "hessian":
        assert not _same_keys(want, _oracle_keys(w, h, 7))
    if over == _over(doBaumberg=0):
        assert len(want) == len(orc.Pyramid(_image(w, h, 7)).candidates()[0])
        assert np.all(want["a11"] == 1.0) and np.all(want["a21"] == 0.0) and np.all(want["a22"] == 1.0)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("over", [_over(maxIterations=0), _over(convergenceThreshold=0.0)])
def test_baumberg_limits_that_keep_nothing(pkg, over, w, h):
    """maxIterations = 0: the loop body never runs and findAffineShape returns false; convergenceThreshold = 0: no eigenvalue
    ratio is below it (eigen_ratio_bef starts at 0 and the test is strict).  0 / 0 keypoints on both sides."""
    want, _ = _detect_and_compare(pkg, w, h, "hessian", over)
    assert len(want) == 0
    assert len(orc.Pyramid(_image(w, h, 7)).candidates()[0]) > 20


@pytest.mark.parametrize("m", [1, 3, 40])
def test_baumberg_work_counters_follow_max_iterations(pkg, m):
    """mods_baumberg_stats under maxIterations = m: every keypoint that enters runs 1 .. m iterations, with m = 1 exactly one."""
    w, h = 320, 240
    over = _over(maxIterations=m)
    want = _oracle_keys(w, h, 7, "hessian", over)
    ctx = pkg.Context(0, w, h, 1)
    try:
        ctx.baumberg_stats_enable(True)
        got = ctx.detect_hessian_affine(_image(w, h, 7), params=_params(pkg, "hessian", over))
        kp, it = ctx.baumberg_stats(0)
        _assert_keys_equal(got, want)
        assert len(want) >= (1 if m == 1 else DEFAULT_BOUND)
        assert kp >= len(got) and kp <= it <= m * kp
        assert kp == len(orc.Pyramid(_image(w, h, 7)).candidates()[0])       # the points the pyramid accepted
        if m == 1:
            assert it == kp
    finally:
        ctx.close()


# ---- 3. NotLessThanRegions off the default threshold --------------------------------------------------------------
# mode 4 uses `threshold` un-squared as its bound (rank_sort_kernel / select_keys_kernel).  Oracle keypoints at 320x240,
# regionsNumber 50 / 400:
#   hessian   th 2.0: 439 / 439    th 5.33: 391 / 400    th 12.0: 354 / 400
#   dog       th 2.0: 304 / 335    th 5.33: 238 / 335    th 12.0: 167 / 335
#   harris    th 2.0: 290 / 342    th 5.33: 286 / 342    th 12.0: 283 / 342
@pytest.mark.parametrize("n_regions", [50, 400])
@pytest.mark.parametrize("th", [2.0, 5.33, 12.0])
@pytest.mark.parametrize("det", ["hessian", "dog", "harris"])
def test_not_less_than_regions_off_the_default_threshold(pkg, det, th, n_regions):
    want, _ = _detect_and_compare(pkg, 320, 240, det, _over(mode=4, threshold=th, regionsNumber=n_regions))
    assert len(want) > 20 and len(want) >= min(n_regions, 335)


def test_not_less_than_regions_in_a_batch_of_five(pkg):
    """Five images in one call rank their keys by rank_sort_kernel (one workgroup per image; up to four images count instead) ahead
    of select_keys_kernel: per-image counts on both sides of regionsNumber.  Oracle keypoints of seeds 1 .. 5 at 203x131 with
    threshold 12.0, regionsNumber 100: 100, 100, 114, 102, 100."""
    import torch
    w, h, seeds = 203, 131, (1, 2, 3, 4, 5)
    over = _over(mode=4, threshold=12.0, regionsNumber=100)
    imgs = [_image(w, h, s) for s in seeds]
    wants = [_oracle_keys(w, h, s, "hessian", over) for s in seeds]
    assert min(len(x) for x in wants) == 100 < max(len(x) for x in wants)
    ctx = pkg.Context(0, w, h, 5)
    try:
        t = torch.from_numpy(np.stack(imgs)).cuda()
        got = ctx.detect_hessian_affine_dev(t.data_ptr(), 5, w, h, params=_params(pkg, "hessian", over), max_out=1 << 12)
        for b in range(5):
            _assert_keys_equal(got[b], wants[b])
    finally:
        ctx.close()


# ---- 4. one live context, and a batch --------------------------------------------------------------------------
LIVE_STEPS = [("hessian", ()),
              ("hessian", _over(threshold=9.0)),
              ("hessian", _over(maxIterations=3)),
              ("hessian", _over(edgeEigenValueRatio=1.0)),                         # the empty result
              ("hessian", ()),
              ("hessian", _over(affBmbrgMethod=1, convergenceThreshold=0.2)),
              ("hessian", _over(doBaumberg=0)),
              ("hessian", _over(smmWindowSize=31, maxIterations=5)),
              ("harris", _over(doBaumberg=1, maxIterations=4)),
              ("hessian", ())]


def test_detector_parameter_changes_on_a_live_context(pkg):
    """A fixed walk through thresholds, iteration limits, both forms of the iteration, window sizes and detectors on ONE context:
    the constants of every launch, the Gaussian window, the occupancy map (reset by the call that claimed its cells), the
    counters and the NMS masks follow the call - the empty step included, which must not disturb the one behind it."""
    w, h = 320, 240
    img = _image(w, h, 7)
    ctx = pkg.Context(0, w, h, 1)
    try:
        for i, (det, over) in enumerate(LIVE_STEPS):
            got = ctx.detect_hessian_affine(img, params=_params(pkg, det, over))
            want = _oracle_keys(w, h, 7, det, over)
            if over == _over(edgeEigenValueRatio=1.0):
                assert len(want) == 0
            else:
                assert len(want) > 20, (i, det, over)
            assert _assert_candidates_equal(ctx, orc.Pyramid(img, _params(orc, det, over))) >= len(want), i
            _assert_keys_equal(got, want)
    finally:
        ctx.close()


# seeds 1, 2, 3 at 203x131 give 37, 36, 56 keypoints with maxIterations = 3 and 90, 102, 108 with convergenceThreshold = 0.2
@pytest.mark.parametrize("over", [_over(maxIterations=3), _over(convergenceThreshold=0.2)])
def test_batch_of_three_images(pkg, over):
    """Three different images in one launch of every stage (blockIdx.y / z = image): per-image candidate lists, accept lists,
    key counts and work, none of them at the .ini's limits."""
    import torch
    w, h, seeds = 203, 131, (1, 2, 3)
    imgs = [_image(w, h, s) for s in seeds]
    ctx = pkg.Context(0, w, h, 3)
    try:
        t = torch.from_numpy(np.stack(imgs)).cuda()
        got = ctx.detect_hessian_affine_dev(t.data_ptr(), 3, w, h, params=_params(pkg, "hessian", over), max_out=1 << 12)
        for b, seed in enumerate(seeds):
            want = _oracle_keys(w, h, seed, "hessian", over)
            assert len(want) > 20
            _assert_candidates_equal(ctx, orc.Pyramid(imgs[b], _params(orc, "hessian", over)), img=b)
            _assert_keys_equal(got[b], want)
    finally:
        ctx.close()


# ---- 5. the region cut of a view --------------------------------------------------------------------------------
# DetectAffineKeypoints (scale-space-detector.cpp:20-21): on a view with tilt > 2 or zoom < 0.5 regionsNumber becomes
# floor(zoom * regionsNumber / tilt).  (tilt, phi, zoom) -> is the view's regionsNumber scaled
VIEW_CUT = [((4.0, 0.0, 1.0), True), ((-4.0, 0.0, 1.0), True), ((3.0, 1.0, 1.0), True), ((1.0, 0.0, 0.25), True),
            ((6.0, math.pi / 3, 0.5), True), ((2.0, 0.0, 1.0), False),       # tilt > 2 is strict
            ((1.0, 0.0, 0.5), False)]                                        # zoom < 0.5 is strict
N_REG = 300
# what the oracle keeps WITHOUT the rule, hessian / dog / harris (mode 2; with it: 75, 75, 100, 75, 25 and 300, 300)
UNSCALED_MODE2 = {(4.0, 0.0, 1.0): (300, 300, 300), (-4.0, 0.0, 1.0): (300, 300, 300), (3.0, 1.0, 1.0): (300, 300, 300),
                  (1.0, 0.0, 0.25): (227, 91, 87), (6.0, math.pi / 3, 0.5): (156, 63, 75)}
# (detector, view) -> oracle keypoints with the rule, without it (mode 4)
VIEW_CUT_MODE4 = [("hessian", (1.0, 0.0, 0.25), 217, 227), ("hessian", (6.0, math.pi / 3, 0.5), 147, 156), ("dog", (4.0, 0.0, 1.0), 298, 300)]


@functools.lru_cache(maxsize=None)
def _oracle_view(view):
    tilt, phi, zoom = view
    px, g = orc.synth_view(_image(640, 480, 11), tilt, phi, zoom, 0.2, 1)
    px.setflags(write=False)
    return px, g


@functools.lru_cache(maxsize=None)
def _oracle_view_regions(view, det, over, scaled=True):
    px, g = _oracle_view(view)
    par = _params(orc, det, over)
    if scaled:
        par = orc.view_params(par, g.tilt, g.zoom)
    regs, _, nd = orc.detect_describe_view(px, np.array(g.H), 640, 480, params=par)
    regs.setflags(write=False)
    return regs, nd


def _view_detect_and_compare(pkg, view, det, over):
    import torch
    w, h = 640, 480
    img = _image(w, h, 11)
    tilt, phi, zoom = view
    want_px, g0 = _oracle_view(view)
    want, nd0 = _oracle_view_regions(view, det, over)
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    try:
        t = torch.from_numpy(img.copy()).cuda()
        torch.cuda.synchronize()
        g, nd, nr = ctx.detect_describe_view_dev(t.data_ptr(), w, h, tilt, phi, zoom, 0.2, 1, det=_params(pkg, det, over))
        got_px = ctx.view_pixels(g)
        assert got_px.shape == want_px.shape
        assert np.array_equal(got_px.view(np.uint32), want_px.view(np.uint32))
        assert (nd, nr) == (nd0, len(want))
        got = ctx.regions_fetch(0)
        for f in REGION_FIELDS:
            assert np.array_equal(got[f], want[f]), f
    finally:
        ctx.close()
    return want, nd0, g0


@pytest.mark.parametrize("view,scaled", VIEW_CUT)
@pytest.mark.parametrize("det", ["hessian", "dog", "harris"])
def test_view_region_cut_fixed_number(pkg, det, view, scaled):
    """mode 2 (FixedRegNumber) with regionsNumber 300 through mods_detect_describe_view_dev: view pixels, counts, regions and
    descriptors equal the oracle's under the view's own regionsNumber."""
    over = _over(mode=2, regionsNumber=N_REG)
    want, nd0, g = _view_detect_and_compare(pkg, view, det, over)
    tilt, phi, zoom = view
    assert g.tilt == abs(tilt) and g.zoom == zoom
    assert nd0 == (math.floor(zoom * N_REG / abs(tilt)) if scaled else N_REG) > 20
    assert len(want) > 10          # (6, pi / 3, 0.5): 15 / 11 / 12 of its 25 keypoints have their centre and frame inside
    if scaled:      # without the rule the oracle keeps more: the cut binds
        unscaled = _oracle_view_regions(view, det, over, scaled=False)[1]
        assert unscaled == UNSCALED_MODE2[view][("hessian", "dog", "harris").index(det)] > nd0


@pytest.mark.parametrize("det,view,with_rule,without_rule", VIEW_CUT_MODE4)
def test_view_region_cut_not_less_than(pkg, det, view, with_rule, without_rule):
    """mode 4 (NotLessThanRegions): the scaled regionsNumber is the floor below which the threshold stops cutting."""
    over = _over(mode=4, regionsNumber=N_REG)
    want, nd0, _ = _view_detect_and_compare(pkg, view, det, over)
    assert nd0 == with_rule > 20 and len(want) > 20
    assert _oracle_view_regions(view, det, over, scaled=False)[1] == without_rule


def test_ladder_region_cut_paired_views(pkg):
    """The step loop with a context of two image slots: both images of a view go through one chain of launches
    (mods_detect_describe_view2_dev, csrc/imgrep.hip), whose detection applies the view's regionsNumber to both.  HessianAffine
    in mode 2 with regionsNumber 400 - 100 on the views of tilt 4 - against the oracle chain: views, both banks, tentatives,
    RANSAC statistics and the inlier list."""
    import torch
    import pipeline_oracle as po
    import refdeg
    from test_gpu_views import _hard_pair
    if not refdeg.available():
        pytest.skip("oracle/_ref not built")
    w, h = 480, 360
    a, b, _ = _hard_pair(w, h, seed=21)
    steps_spec = [((1, 2, 4), 360.0), ((1, 2, 4), 120.0)]
    over = _over(mode=2, regionsNumber=400)
    want = po.match_ladder(a, b, steps_spec, seed_time=31, min_matches=10 ** 6, params=_params(orc, "hessian", over))
    plain = po.match_ladder(a, b, steps_spec, seed_time=31, min_matches=10 ** 6, params=_params(orc, "hessian", over), view_rule=False)
    # 10 views per image, 6 of them of tilt 4: banks of 1590 and 1949 regions with the rule, 2814 and 2234 without
    assert all(20 < n < m for n, m in zip(want["n_described"], plain["n_described"]))
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 2)          # two image slots: paired views
    rep1, rep2 = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
    try:
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        pkg.ransac_pin_seed(31)
        par = pkg.PairParams.default()
        par.det = _params(pkg, "hessian", over)
        steps = [pkg.LadderStep.make(tl, ph) for tl, ph in steps_spec]
        res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, rep1, rep2, params=par, min_matches=10 ** 6, max_matches=100000)
        assert res.steps_done == want["steps_done"] == 2 and res.n_views == want["n_views"] == 20
        assert list(res.n_described) == want["n_described"] == [len(rep1), len(rep2)]
        for got, exp in ((rep1.fetch(), want["regions"][0]), (rep2.fetch(), want["regions"][1])):
            assert len(got) == len(exp) > 20
            for f in ("x", "y", "s", "a11", "a12", "a21", "a22", "desc"):
                assert np.array_equal(got[f], exp[f]), f
        assert res.n_tentatives == want["n_tentatives"] > 20 and res.n_unique == want["n_unique"]
        assert [res.ransac_samples, res.ransac_lo, res.ransac_rejects] == want["stats"]
        assert res.n_inliers == want["n_inliers"] >= 15          # 121
        assert np.array_equal(m, want["u6"][want["mask"]][:, [0, 1, 3, 4]])
    finally:
        rep1.close(); rep2.close(); ctx.close()
