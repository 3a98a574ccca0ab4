"""-m gpu tests of the doubled first octave (mods_ctx_upscale_input): the primitive, every plane of the upscaled scale space in the
fused (mode 1) and the unfused (mode 2) form, keys and candidates against the CPU oracle's plain detection of the doubled image,
detect + describe end to end, a view, a live context with recorded graphs, and the refusals.  The contract is restated in
tests/upscale_ref.py.  Every comparison is np.array_equal; there are no tolerances."""
import functools

import numpy as np
import pytest

import detection_mask_ref as mref
import orc
import synth
import upscale_ref as ur

pytestmark = pytest.mark.gpu

SAME = ("octave", "level", "r0", "c0", "sub_type", "response", "a11", "a12", "a21", "a22")
HALVED = ("x", "y", "s")


def _params(mod, det="hessian", **over):
    p = {"hessian": mod.HessAffParams.default, "dog": mod.HessAffParams.dog, "harris": mod.HessAffParams.harris}[det]()
    for k, v in over.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _image(w, h, seed=7):
    img = synth.texture(w, h, seed=seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _doubled(w, h, seed=7):
    d = ur.double_image(_image(w, h, seed))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _ref_planes(w, h, det, S, s0):
    return ur.planes(_image(w, h), _params(orc, det, numberOfScales=S, initialSigma=s0))


@functools.lru_cache(maxsize=None)
def _oracle_keys(w, h, det, seed=7, **over):
    """the oracle's plain detection of the doubled image: what the upscaled detection is at initialSigma <= 0.5, up to the halving"""
    keys = orc.detect_hessian_affine(_doubled(w, h, seed), _params(orc, det, **over))
    keys.setflags(write=False)
    return keys


def _assert_upscaled_keys(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in SAME:
        assert np.array_equal(got[f], want[f]), f
    for f in HALVED:
        assert np.array_equal(2.0 * got[f], want[f]), f


# ---- 1. the primitive ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (1, 7), (7, 1), (64, 32), (65, 33), (127, 3), (203, 131), (320, 240)])
def test_upscale2x(pkg, w, h):
    img = synth.texture(max(w, 16), max(h, 16), seed=3)[:h, :w].copy()
    ctx = pkg.Context(0, w, h, 1)
    try:
        assert np.array_equal(ctx.upscale2x(img), ur.double_image(img))
        hard = np.array([[1e8, 1.0], [-1e8, 1.0]], np.float32)          # the summation order (tests/test_cpu_upscale.py)
        if w >= 2 and h >= 2:
            assert ctx.upscale2x(hard)[1, 1] == np.float32(0.25)
    finally:
        ctx.close()


# ---- 2. planes -------------------------------------------------------------------------------------------------
# (numberOfScales, initialSigma): the initial blur has sigma sqrt(s0^2 - 1): 9 taps at 1.6 and 1.8, 5 at 1.2, 11 at 2.0, 19 at 3.2 (wider
# than the fast kernel: the unfused route in both modes); none at <= 1.0
SCHEDULES = [(3, 1.6), (3, 1.2), (3, 1.8), (3, 2.0), (3, 3.2), (3, 1.0), (3, 0.5), (6, 0.7), (2, 1.6)]
INITIAL_TAPS = {1.6: 9, 1.2: 5, 1.8: 9, 2.0: 11, 3.2: 19}
DIMS = {(203, 131): [(406, 262), (203, 131), (102, 66), (51, 33), (26, 16)],
        (320, 240): [(640, 480), (320, 240), (160, 120), (80, 60), (40, 30), (20, 15)]}


def test_initial_blur_taps():
    f = np.float32
    for s0, taps in INITIAL_TAPS.items():
        assert orc.gauss_ksize(float(np.sqrt(f(s0) * f(s0) - f(1.0)))) == taps, s0


def _assert_planes(ctx, dims, planes, n_levels, img=0):
    assert ctx.pyramid_octaves() == len(dims)
    for o, d in enumerate(dims):
        assert ctx.pyramid_dims(o) == d
        for lv in range(n_levels):
            for kind in (0, 1):
                assert np.array_equal(ctx.pyramid_plane(img, o, lv, kind), planes[(o, lv, kind)]), (img, o, lv, kind)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("S,s0", SCHEDULES)
@pytest.mark.parametrize("w,h", sorted(DIMS))
def test_planes(pkg, w, h, S, s0, mode):
    """octaves, dims and every blur and response plane of the upscaled HessianAffine scale space equal the composition from the
    oracle's primitives, with the first level made by one launch (mode 1) and by two (mode 2)"""
    dims, planes = _ref_planes(w, h, "hessian", S, s0)
    assert dims == DIMS[(w, h)]
    ctx = pkg.Context(0, w, h, 1)
    try:
        ctx.upscale_input(mode)
        assert ctx.upscale_input_get() == mode
        ctx.detect_hessian_affine(_image(w, h), params=_params(pkg, numberOfScales=S, initialSigma=s0))
        _assert_planes(ctx, dims, planes, S + 2)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("det", ["dog", "harris"])
@pytest.mark.parametrize("s0", [1.6, 0.5])
@pytest.mark.parametrize("w,h", sorted(DIMS))
def test_planes_dog_and_harris(pkg, w, h, s0, det, mode):
    dims, planes = _ref_planes(w, h, det, 3, s0)
    assert dims == DIMS[(w, h)]
    ctx = pkg.Context(0, w, h, 1)
    try:
        ctx.upscale_input(mode)
        ctx.detect_hessian_affine(_image(w, h), params=_params(pkg, det, numberOfScales=3, initialSigma=s0))
        _assert_planes(ctx, dims, planes, 5)
    finally:
        ctx.close()


def test_tiny_images(pkg):
    """13 x 9 gives one octave of 26 x 18 (its planes checked); 6 x 40 doubles to 12 x 80, not wider than 2 border + 2: no octave, an
    empty list, no error"""
    for mode in (1, 2):
        for (w, h), want_dims in (((13, 9), [(26, 18)]), ((6, 40), [])):
            img = synth.texture(48, 48, seed=5)[:h, :w].copy()
            ctx = pkg.Context(0, w, h, 1)
            try:
                ctx.upscale_input(mode)
                keys = ctx.detect_hessian_affine(img)
                dims, planes = ur.planes(img)
                assert dims == want_dims
                _assert_planes(ctx, dims, planes, 5)
                if not want_dims:
                    assert len(keys) == 0
            finally:
                ctx.close()


# ---- 3. keys against the oracle --------------------------------------------------------------------------------
# detector, settings, then per size the oracle's (keys, of which in octave 0) - counted on the CPU; a case proves nothing unless
# the doubled octave contributes
KEY_CASES = [
    ("hessian", dict(threshold=2.0, initialSigma=0.5), {(160, 120): (42, 12), (203, 131): (82, 24), (320, 240): (325, 69)}),
    ("hessian", dict(threshold=2.0, initialSigma=0.4), {(160, 120): (29, 10), (203, 131): (55, 22), (320, 240): (224, 52)}),
    ("harris", dict(initialSigma=0.5), {(160, 120): (177, 48), (203, 131): (240, 65)}),
    ("dog", dict(threshold=1.0, initialSigma=0.5), {(160, 120): (42, 18), (203, 131): (84, 42)}),
    # selection modes (default threshold): FixedRegNumber, RelativeRegNumber, NotLessThanRegions
    ("hessian", dict(initialSigma=0.5, mode=2, regionsNumber=60), {(160, 120): (60, 29)}),
    ("hessian", dict(initialSigma=0.5, mode=3, relativeRegionsNumber=0.02), {(160, 120): (229, 198)}),
    ("hessian", dict(initialSigma=0.5, mode=4, regionsNumber=60), {(160, 120): (60, 29)}),
]
KEY_PARAMS = [(det, tuple(sorted(over.items())), w, h, n, n0) for det, over, sizes in KEY_CASES for (w, h), (n, n0) in sorted(sizes.items())]


@pytest.mark.parametrize("det,over,w,h,n,n0", KEY_PARAMS)
def test_keys_and_candidates_against_the_oracle(pkg, det, over, w, h, n, n0):
    """At initialSigma <= 0.5 neither side blurs the first level, so the upscaled detection of I is the oracle's plain detection of
    double_image(I): the same keys with x, y, s halved (exact), the same candidates at pixelDistance 0.5 * 2^octave"""
    over = dict(over)
    want = _oracle_keys(w, h, det, **over)
    assert (len(want), int((want["octave"] == 0).sum())) == (n, n0)
    ctx = pkg.Context(0, w, h, 1)
    try:
        ctx.upscale_input(1)
        got = ctx.detect_hessian_affine(_image(w, h), params=_params(pkg, det, **over))
        _assert_upscaled_keys(got, want)
        assert int((got["octave"] == 0).sum()) == n0
        pyr = orc.Pyramid(_doubled(w, h), _params(orc, det, **over))
        cw, _ = pyr.candidates()
        cg = ctx.pyramid_candidates(0)
        cg = cg[np.lexsort((cg["c0"], cg["r0"], cg["level"], cg["octave"]))]
        assert len(cg) == len(cw) >= n
        for f in ("octave", "level", "r0", "c0", "r", "c", "response", "type"):
            assert np.array_equal(cg[f], cw[f]), f
        for f in ("x", "y", "s", "pixelDistance"):
            assert np.array_equal(np.float32(2.0) * cg[f], cw[f]), f
        assert np.array_equal(cg["pixelDistance"], np.float32(0.5) * np.float32(2.0) ** cg["octave"].astype(np.float32))
        assert ctx.pyramid_dims(0) == (2 * w, 2 * h)
    finally:
        ctx.close()


# ---- 4. end to end ---------------------------------------------------------------------------------------------
def _oracle_regions(img, keys):
    """the oracle's orientation and description (oracle/capi.cpp: orc_detect_describe_ex) of keys given in image coordinates"""
    h, w = img.shape
    r = orc.filter_centres_inside(orc.regions_from_keys(keys), w, h)
    r = orc.filter_touch_boundary(orc.detect_orientation(img, r), w, h)
    return orc.describe_rootsift(img, r)


def _assert_regions(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "desc"):
        assert np.array_equal(got[f], want[f]), f


def test_detect_describe_end_to_end(pkg):
    """detect + describe with the switch on: the same regions and descriptors as the detection followed by orient_describe on the
    same context, equal to the oracle's composition at initialSigma 0.5 (its keys of the doubled image, halved, oriented and
    described on the original image); a batch of three equals the three single calls; under a detection mask (the right half of
    the image zero) the list is the unmasked list without the off-mask entries"""
    import torch
    w, h = 203, 131
    seeds = (7, 8, 9)
    over = dict(threshold=2.0, initialSigma=0.5)
    par = _params(pkg, **over)
    t = torch.from_numpy(np.stack([_image(w, h, s) for s in seeds])).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 3)
    try:
        ctx.upscale_input(1)
        singles = []
        for b, seed in enumerate(seeds):
            img = _image(w, h, seed)
            nd, nr = ctx.detect_describe_dev(t.data_ptr() + 4 * b * w * h, 1, w, h, det=par)
            regs = ctx.regions_fetch(0)
            keys = ctx.detect_hessian_affine(img, params=par)
            assert nd == [len(keys)] and nr == [len(regs)] and len(regs) > 20
            assert regs.tobytes() == ctx.orient_describe(img, keys).tobytes()
            want_keys = ur.halved(_oracle_keys(w, h, "hessian", seed=seed, **over))
            assert int((want_keys["octave"] == 0).sum()) >= 10
            _assert_regions(regs, _oracle_regions(img, want_keys))
            singles.append(regs)
        nd, nr = ctx.detect_describe_dev(t.data_ptr(), 3, w, h, det=par)
        for b in range(3):
            assert ctx.regions_fetch(b).tobytes() == singles[b].tobytes(), b
        mask = np.full((h, w), 255, np.uint8)
        mask[:, w // 2:] = 0
        mref.assert_non_vacuous(singles[0], mask)
        ctx.set_detection_mask(0, mask)
        ctx.detect_describe_dev(t.data_ptr(), 1, w, h, det=par)
        mref.assert_same_but_positions(ctx.regions_fetch(0), mref.filter_regions(singles[0], mask))
    finally:
        ctx.close()


# ---- 5. a view -------------------------------------------------------------------------------------------------
def test_view(pkg):
    """One tilt view (tilt 2, phi 0) through mods_detect_describe_view_dev with the switch on.  Observable: the view's pixels are
    fetched (view_pixels) and detected as an identity image on the same context, switch on - at initialSigma 0.5 these keys are the
    oracle's of the doubled view, halved, some in octave 0 - and the view call detected as many; every region of the view call
    carries the response of one of those keys (responses are unique and survive the way back to the original frame), lies inside
    the original image, and has the descriptor that orient_describe gives that key on the view's pixels (orientation and
    description work in the view's frame).  With the switch off the view detects another number of keys."""
    import torch
    w, h, tilt, phi = 320, 240, 2.0, 0.0
    img = _image(w, h, 3)
    over = dict(threshold=2.0, initialSigma=0.5)
    par = _params(pkg, **over)
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    try:
        t = torch.from_numpy(np.array(img)).cuda()
        torch.cuda.synchronize()
        _, nd_off, _ = ctx.detect_describe_view_dev(t.data_ptr(), w, h, tilt, phi, det=par)
        ctx.upscale_input(1)
        g, nd, nr = ctx.detect_describe_view_dev(t.data_ptr(), w, h, tilt, phi, det=par)
        regs = ctx.regions_fetch(0)
        px = ctx.view_pixels(g)
        keys = ctx.detect_hessian_affine(px, params=par)
        want = orc.detect_hessian_affine(ur.double_image(px), _params(orc, **over))
        _assert_upscaled_keys(keys, want)
        assert nd == len(keys) != nd_off and int((keys["octave"] == 0).sum()) >= 5
        assert nr == len(regs) > 20 and len(np.unique(keys["response"])) == len(keys)
        assert np.all(np.isin(regs["response"], keys["response"]))
        assert regs["x"].min() > 0 and regs["x"].max() < w and regs["y"].min() > 0 and regs["y"].max() < h
        in_view = ctx.orient_describe(px, keys)
        by_resp = {float(r["response"]): r["desc"] for r in in_view}
        shared = [r for r in regs if float(r["response"]) in by_resp]
        assert len(shared) > 20
        for r in shared:
            assert np.array_equal(r["desc"], by_resp[float(r["response"])])
    finally:
        ctx.close()


# ---- 6. a live context -----------------------------------------------------------------------------------------
def test_off_on_off_on_a_live_context_with_graphs(pkg):
    """55 copies of the 320 x 240 image of test 3: 4.2 Mpx, so the scale space forks and the calls are recorded and replayed
    (mods_ctx_graphs).  off -> on -> off on one context: the two "off" results are equal to each other and to a fresh context's, the
    "on" result is the oracle's composition of test 4 for every image slot, and no recording is replayed across a change"""
    import torch
    w, h, n = 320, 240, 55
    assert w * h * n >= 4 << 20
    over = dict(threshold=2.0, initialSigma=0.5)
    par = _params(pkg, **over)
    img = _image(w, h)
    t = torch.from_numpy(np.stack([img] * n)).cuda()
    torch.cuda.synchronize()
    want_on = _oracle_regions(img, ur.halved(_oracle_keys(w, h, "hessian", **over)))
    assert len(_oracle_keys(w, h, "hessian", **over)) == 325

    def call(ctx):
        nd, nr = ctx.detect_describe_dev(t.data_ptr(), n, w, h, det=par)
        return nd, [ctx.regions_fetch(b).tobytes() for b in (0, n // 2, n - 1)]

    fresh = pkg.Context(0, w, h, n)
    try:
        want_off = call(fresh)
    finally:
        fresh.close()
    ctx = pkg.Context(0, w, h, n)
    try:
        ctx.graphs(True)
        off1 = [call(ctx) for _ in range(3)]
        replays = ctx.graph_replays()
        assert replays >= 1 and off1 == [want_off] * 3
        ctx.upscale_input(1)
        on = [call(ctx) for _ in range(3)]
        assert ctx.graph_replays() > replays and on[1] == on[0] and on[2] == on[0]
        assert on[0][0] == [325] * n and on[0] != want_off
        for b in (0, n // 2, n - 1):
            _assert_regions(ctx.regions_fetch(b), want_on)
        ctx.upscale_input(0)
        assert [call(ctx) for _ in range(3)] == [want_off] * 3
    finally:
        ctx.close()


def test_pair_and_pipeline(pkg):
    """mods_match_pair_dev with the switch on describes the regions detect + describe gives for both images; a pipeline with
    mods_pipeline_upscale_input returns what mods_match_pair_dev returns on a context set the same way; after the first submit the
    setter is refused"""
    import torch
    w, h = 320, 240
    pairs = [synth.pair(w, h, seed=s)[:2] for s in (0, 5)]
    par = pkg.PairParams.default()
    ctx = pkg.Context(0, w, h, 2)
    pipe = pkg.Pipeline(0, w, h, params=par, gpu_workers=1, verify_workers=1, pairs_per_batch=2)
    try:
        ctx.upscale_input(1)
        want = []
        for a, b in pairs:
            a, b = a.astype(np.uint8).astype(np.float32), b.astype(np.uint8).astype(np.float32)      # (the pipeline takes 8-bit images)
            t = torch.from_numpy(np.stack([a, b])).cuda()
            torch.cuda.synchronize()
            ctx.detect_describe_dev(t.data_ptr(), 2, w, h, det=par.det)
            regs = [ctx.regions_fetch(i) for i in range(2)]
            ctx.upscale_input(0)
            pkg.ransac_pin_seed(11)
            plain, _ = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, par, max_matches=10000)
            ctx.upscale_input(1)
            pkg.ransac_pin_seed(11)
            res, m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, par, max_matches=10000)
            for i in range(2):
                assert ctx.regions_fetch(i).tobytes() == regs[i].tobytes() and len(regs[i]) > 20
            assert list(res.n_detected) != list(plain.n_detected) and res.n_inliers >= 15
            want.append((res, m))
        pipe.upscale_input(1)
        pkg.ransac_pin_seed(11)
        u8 = [pkg.PinnedBuffer((2, h, w), np.uint8) for _ in pairs]
        for k, (a, b) in enumerate(pairs):
            u8[k].array[:] = np.stack([a, b]).astype(np.uint8)
            pipe.submit_host(u8[k].ptr.value, tag=k, u8=True)
        for k in range(len(pairs)):
            res, tag, m = pipe.next_matches()
            exp, exp_m = want[k]
            assert tag == k
            for f in ("n_tentatives", "n_unique", "n_inliers"):
                assert getattr(res, f) == getattr(exp, f), (tag, f)
            assert list(res.n_detected) == list(exp.n_detected) and list(res.n_described) == list(exp.n_described)
            assert np.array_equal(m, exp_m) and list(res.H) == list(exp.H), tag
        with pytest.raises(pkg.ModsError, match="after the first submit"):
            pipe.upscale_input(0)
        for b in u8:
            b.close()
    finally:
        pkg.ransac_pin_seed(-1)
        pipe.close(); ctx.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------
def test_refusals(pkg):
    """4096 x 2048 doubles to 2^25 pixels, past the order key of an octave: MODS_E_ARG (-2) before anything is allocated or
    launched, and the context works afterwards with the switch off; a bad mode is refused and changes nothing; MSER ignores the
    switch"""
    import torch
    W, H = 4096, 2048
    w, h = 320, 240
    ctx = pkg.Context(0, W, H, 1)
    try:
        big = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.upscale_input(1)
        stages = ("blur", "blur_small", "response", "resize", "nms")
        ctx.timing_enable(stages)
        ctx.timing_reset()
        with pytest.raises(pkg.ModsError, match=r"error -2: upscale_input: the doubled 4096x2048 image"):
            ctx.detect_hessian_affine_dev(big.data_ptr(), 1, W, H)
        assert [ctx.timing_read(s)[1] for s in stages] == [0] * len(stages)
        ctx.timing_enable(())
        with pytest.raises(pkg.ModsError, match="upscale_input: mode 3"):
            ctx.upscale_input(3)
        assert ctx.upscale_input_get() == 1
        ctx.upscale_input(0)
        got = ctx.detect_hessian_affine(_image(w, h))
        want = orc.detect_hessian_affine(_image(w, h))
        assert len(got) == len(want) > 20
        for f in SAME + HALVED:
            assert np.array_equal(got[f], want[f]), f
        mser = pkg.HessAffParams.mser()
        off = ctx.detect_hessian_affine(_image(w, h), params=mser)
        ctx.upscale_input(1)
        on = ctx.detect_hessian_affine(_image(w, h), params=mser)
        assert len(off) > 20 and on.tobytes() == off.tobytes()
    finally:
        ctx.close()
