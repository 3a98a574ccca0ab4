"""-m gpu parity tests of the scale space away from numberOfScales = 3, initialSigma = 1.6, border = 5: every blur radius of the
fused and the generic kernel, the one-launch LDS tail with 3 .. 8 levels and 3 .. 17 taps, small octaves through the tiled kernels,
no initial blur, parameter changes on a live context, per-image planes of a batch, and the forked build on large tiles.  Every
comparison is np.array_equal against the CPU oracle."""
import functools

import numpy as np
import pytest

import orc
import synth

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "octave", "level", "r0", "c0")   # as test_gpu_detect.py

# (numberOfScales, initialSigma) -> Gaussian kernel sizes: the initial blur (None: skipped), then the increments to levels 1 .. S + 1
SCHEDULES = {
    (3, 0.5): (None, 3, 3, 5, 5),                # no initial blur; R = 1, 2 fused; the LDS kernel's n <= 5 row branch
    (3, 0.4): (None, 3, 3, 3, 5),                # initialSigma below the assumed 0.5 of the input
    (3, 1.0): (7, 5, 7, 9, 11),                  # R = 2, 3 fused
    (3, 1.8): (11, 9, 11, 15, 17),               # R = 8 fused; 17 taps in the LDS kernel
    (3, 2.0): (13, 11, 13, 15, 19),              # last level generic + separate response; LDS kernel off: small octaves tiled
    (3, 3.2): (19, 15, 19, 25, 31),              # generic initial blur; fused and generic levels mixed
    (2, 1.6): (11, 11, 15, 21),                  # 4 levels, mixed
    (2, 1.0): (7, 7, 9, 13),                     # 4 levels, LDS kernel on
    (1, 0.8): (5, 9, 17),                        # 3 levels
    (4, 1.6): (11, 7, 9, 9, 11, 13),             # 6 levels
    (5, 1.6): (11, 7, 7, 9, 9, 11, 11),          # 7 levels
    (6, 1.6): (11, 5, 7, 7, 7, 9, 9, 11),        # 8 levels = kMaxLevels
    (6, 0.7): (3, 3, 3, 3, 5, 5, 5, 5),          # 8 levels, R = 1, 2 only
}
REFUSED = (1, 1.6)                               # (11, 17, 35): level 2 is wider than kMaxBlurRadius allows


def _schedule_ksizes(S, s0):
    """The kernel sizes of a schedule in the detector's fp32 arithmetic (pyramid.cpp:428-494)."""
    f = np.float32
    step = f(2.0) ** f(1.0 / S)
    out = [orc.gauss_ksize(float(np.sqrt(f(s0) * f(s0) - f(0.25)))) if s0 > 0.5 else None]
    cur = f(s0)
    for _ in range(S + 1):
        out.append(orc.gauss_ksize(float(cur * np.sqrt(step * step - f(1.0)))))
        cur = cur * step
    return tuple(out)


def test_schedule_table_is_what_the_oracle_computes():
    for (S, s0), want in SCHEDULES.items():
        assert _schedule_ksizes(S, s0) == want, (S, s0)
    assert _schedule_ksizes(*REFUSED) == (11, 17, 35)


def _params(mod, S, s0, border=5, det="hessian", threshold=None):
    p = {"hessian": mod.HessAffParams.default, "dog": mod.HessAffParams.dog, "harris": mod.HessAffParams.harris}[det]()
    p.numberOfScales, p.initialSigma, p.border = S, s0, border
    if threshold is not None:
        p.threshold = threshold
    return p


@functools.lru_cache(maxsize=None)
def _image(w, h, seed):
    img = synth.texture(w, h, seed=seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _oracle_keys(w, h, seed, S, s0, border=5, det="hessian", threshold=None):
    keys = orc.detect_hessian_affine(_image(w, h, seed), _params(orc, S, s0, border, det, threshold))
    keys.setflags(write=False)
    return keys


def _assert_keys_equal(got, want):
    assert len(got) == len(want)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), "field %s differs" % f


def _assert_planes_equal(ctx, pyr, n_levels, img=0):
    assert ctx.pyramid_octaves() == pyr.n_oct
    for o in range(pyr.n_oct):
        assert ctx.pyramid_dims(o) == pyr.dims(o)
        for lv in range(n_levels):
            for kind in (0, 1):
                assert np.array_equal(ctx.pyramid_plane(img, o, lv, kind), pyr.plane(o, lv, kind)), (img, o, lv, kind)


def _assert_candidates_equal(ctx, pyr, img=0):
    cand_want, _ = pyr.candidates()
    cand_got = ctx.pyramid_candidates(img)
    cand_got = cand_got[np.lexsort((cand_got["c0"], cand_got["r0"], cand_got["level"], cand_got["octave"]))]
    assert len(cand_got) == len(cand_want)
    for f in cand_want.dtype.names:
        assert np.array_equal(cand_got[f], cand_want[f]), f
    return len(cand_want)


# ---- 1. schedule sweep --------------------------------------------------------------------------
# 320x240 -> 160x120, 80x60, 40x30, 20x15 (border 2: + 10x8; border 9: without 20x15); 203x131 -> 102x66, 51x33, 26x16 (border 2:
# + 13x8; border 9: without 26x16): octave 0 of odd width takes the narrow NMS kernel and the any-width response kernel.
# 256x1000 at numberOfScales 4: 43360 NMS ballot words of which the context's own allocation held 40512.
SWEEP = [(w, h, S, s0, 5) for (S, s0) in SCHEDULES for (w, h) in ((320, 240), (203, 131))]
SWEEP += [(w, h, 3, 1.6, b) for b in (2, 9) for (w, h) in ((320, 240), (203, 131))]
SWEEP += [(256, 1000, 4, 1.6, 5)]
DESCRIBED = ((3, 0.5), (3, 1.8), (5, 1.6))


@pytest.mark.parametrize("w,h,S,s0,border", SWEEP)
def test_schedule_sweep(pkg, w, h, S, s0, border):
    """One detection per schedule on a context sized exactly to its image (so that no buffer is larger than the image's own
    context would make it): octaves, every blur and response plane, candidates and keypoints equal the oracle's bit for bit; for
    three schedules the descriptors behind them as well."""
    img = _image(w, h, 7)
    po = _params(orc, S, s0, border)
    want = _oracle_keys(w, h, 7, S, s0, border)
    assert len(want) > 20
    ctx = pkg.Context(0, w, h, 1)
    try:
        got = ctx.detect_hessian_affine(img, params=_params(pkg, S, s0, border))
        pyr = orc.Pyramid(img, po)
        assert pyr.n_oct == {(320, 5): 5, (320, 2): 6, (320, 9): 4, (203, 5): 4, (203, 2): 5, (203, 9): 3, (256, 5): 5}[(w, border)]
        _assert_planes_equal(ctx, pyr, S + 2)
        _assert_candidates_equal(ctx, pyr)
        _assert_keys_equal(got, want)
        if (S, s0) in DESCRIBED and border == 5 and w != 256:
            wr, ndet = orc.detect_describe(img, po)
            regs = ctx.orient_describe(img, got)
            assert ndet == len(want) and len(regs) == len(wr) > 20
            assert np.array_equal(regs["desc"], wr["desc"]) and np.array_equal(regs["x"], wr["x"])
    finally:
        ctx.close()


# ---- 2. DoG and Harris off the default ----------------------------------------------------------------
# Thresholds: the .ini's (DoG 8.0, Harris 15.0) wherever the oracle alone then returns more than 20 keypoints; DoG (3, 0.5) returns
# 14 at 203x131 with 8.0, so it runs at 2.0.  Oracle keypoints per case at 203x131 / 320x240:
#   dog    (3, 0.5) th 2.0: 35 / 121     dog    (2, 1.6) th 8.0: 50 / 189     dog    (5, 1.0) th 8.0: 54 / 178
#   harris (3, 0.5) th 15.0: 243 / 762   harris (2, 1.6) th 15.0: 91 / 256    harris (5, 1.0) th 15.0: 156 / 478
# (3, 0.5): the response blurs have 3 taps (DoG sigma 0.25 .. 0.63, Harris 0.39 .. 0.61), wide_blur_row_kernel's n <= 5 branch.
ALT_CASES = [("dog", 3, 0.5, 2.0), ("dog", 2, 1.6, 8.0), ("dog", 5, 1.0, 8.0),
             ("harris", 3, 0.5, 15.0), ("harris", 2, 1.6, 15.0), ("harris", 5, 1.0, 15.0)]


@pytest.mark.parametrize("det,S,s0,th", ALT_CASES)
@pytest.mark.parametrize("w,h", [(203, 131), (320, 240)])
def test_dog_and_harris_off_the_default(pkg, det, S, s0, th, w, h):
    img = _image(w, h, 7)
    po = _params(orc, S, s0, 5, det, th)
    want = _oracle_keys(w, h, 7, S, s0, 5, det, th)
    assert len(want) > 20
    ctx = pkg.Context(0, w, h, 1)
    try:
        got = ctx.detect_hessian_affine(img, params=_params(pkg, S, s0, 5, det, th))
        pyr = orc.Pyramid(img, po)
        _assert_planes_equal(ctx, pyr, S + 2)
        assert _assert_candidates_equal(ctx, pyr) > 20
        _assert_keys_equal(got, want)
        assert set(np.unique(want["sub_type"])) <= ({30, 31} if det == "harris" else {10, 11})
    finally:
        ctx.close()


# ---- 3. parameter changes on one live context ------------------------------------------------------------
LIVE_STEPS = [("hessian", 3, 1.6), ("hessian", 6, 1.6), ("hessian", 3, 0.5), ("hessian", 2, 1.6), ("dog", 3, 1.6), ("dog", 2, 1.6),
              ("harris", 3, 0.5), ("hessian", 3, 1.6), ("hessian",) + REFUSED, ("hessian", 3, 1.6)]


def test_parameter_changes_on_a_live_context(pkg):
    """The tap slots (keyed by sigma), the response-blur tables of DoG / Harris, the device copy of the octave table, the plane
    pool (regrown when the level count rises) and the NMS mask layout all follow the parameters of the call: a fixed walk through
    schedules and detectors on ONE context gives the oracle's planes and keypoints at every step.  numberOfScales = 1 at
    initialSigma = 1.6 needs a 35-tap kernel, which the blur kernels do not have: the call is refused before any launch, and
    the context's next call is unaffected."""
    w, h = 320, 240
    img = _image(w, h, 7)
    ctx = pkg.Context(0, w, h, 1)
    launch_stages = ("blur", "blur_small", "response", "resize", "nms", "localize", "baumberg", "sort")
    try:
        for det, S, s0 in LIVE_STEPS:
            if (S, s0) == REFUSED:
                ctx.timing_enable(launch_stages)
                ctx.timing_reset()
                with pytest.raises(pkg.ModsError, match="gaussian kernel too wide.*ksize=35"):
                    ctx.detect_hessian_affine(img, params=_params(pkg, S, s0, 5, det))
                assert [ctx.timing_read(s)[1] for s in launch_stages] == [0] * len(launch_stages)
                ctx.timing_enable(())
                continue
            got = ctx.detect_hessian_affine(img, params=_params(pkg, S, s0, 5, det))
            want = _oracle_keys(w, h, 7, S, s0, 5, det)
            assert len(want) > 20, (det, S, s0)
            _assert_planes_equal(ctx, orc.Pyramid(img, _params(orc, S, s0, 5, det)), S + 2)
            _assert_keys_equal(got, want)
    finally:
        ctx.close()


# ---- 4. planes of batched images ----------------------------------------------------------------------
@pytest.mark.parametrize("S,s0", [(3, 0.5), (4, 1.6), (3, 2.0)])
def test_batch_planes_per_image(pkg, S, s0):
    """Three different images in one launch: the fused response's, the separate response's and the LDS kernel's per-image plane
    offsets, read back for every image index (fused + LDS, no initial blur; six levels; generic last level, LDS kernel off)."""
    import torch
    w, h, seeds = 203, 131, (1, 2, 3)
    imgs = [_image(w, h, s) for s in seeds]
    ctx = pkg.Context(0, w, h, 3)
    try:
        t = torch.from_numpy(np.stack(imgs)).cuda()
        got = ctx.detect_hessian_affine_dev(t.data_ptr(), 3, w, h, params=_params(pkg, S, s0), max_out=1 << 12)
        for b, seed in enumerate(seeds):
            want = _oracle_keys(w, h, seed, S, s0)
            assert len(want) > 20
            _assert_planes_equal(ctx, orc.Pyramid(imgs[b], _params(orc, S, s0)), S + 2, img=b)
            _assert_keys_equal(got[b], want)
    finally:
        ctx.close()


# ---- 5. side-stream fork with large tiles ----------------------------------------------------------------
@pytest.mark.parametrize("S,s0", [(4, 1.6), (6, 0.7), (3, 1.8)])
def test_forked_build_on_large_tiles(pkg, S, s0):
    """17 images of 512x496 = 4 317 184 px: above the 4 Mpx threshold of the fork (octaves from the third on, and their NMS, on a
    side stream), and 4 x 8 x 17 = 544 tiles in octave 0, above the 384 that select the 32-row, two-float4 instantiations of the
    fused blur + response kernel - the three schedules cover R = 1 .. 8 there.  Keypoints of all images and the planes of the
    first, a middle and the last image equal the oracle's; one stream and two streams agree byte for byte."""
    import torch
    w, h, n = 512, 496, 17
    imgs = [_image(w, h, 100 + i) for i in range(n)]
    assert w * h * n >= 4 << 20 and ((w + 127) // 128) * ((h + 63) // 64) * n >= 384
    plane_imgs = (0, 8, 16)
    ctx = pkg.Context(0, w, h, n)
    try:
        t = torch.from_numpy(np.stack(imgs)).cuda()
        runs = []
        for streams in (2, 1):
            ctx.pyramid_streams(streams)
            keys = ctx.detect_hessian_affine_dev(t.data_ptr(), n, w, h, params=_params(pkg, S, s0), max_out=1 << 13)
            planes = [ctx.pyramid_plane(b, o, lv, kind) for b in plane_imgs for o in range(ctx.pyramid_octaves())
                      for lv in range(S + 2) for kind in (0, 1)]
            runs.append((keys, planes))
        for b in range(n):
            want = _oracle_keys(w, h, 100 + b, S, s0)
            assert len(want) > 20
            _assert_keys_equal(runs[0][0][b], want)
            assert runs[0][0][b].tobytes() == runs[1][0][b].tobytes(), b
        assert len(runs[0][1]) == len(runs[1][1])
        for p2, p1 in zip(runs[0][1], runs[1][1]):
            assert p2.tobytes() == p1.tobytes()
        for b in plane_imgs:      # (the context still holds the one-stream run)
            _assert_planes_equal(ctx, orc.Pyramid(imgs[b], _params(orc, S, s0)), S + 2, img=b)
    finally:
        ctx.close()
