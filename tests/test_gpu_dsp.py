"""-m gpu: domain-size pooling of SIFT descriptors (mods_ctx_domain_pooling; contract in include/mods_hip.h) against its numpy
restatement (tests/dsp_ref.py), bit for bit: the accumulate and finish kernels on crafted patch sets, the describe entry points with
chosen keypoints whose domains cross every tier of the extraction and reach past the image, the 8-bit sampling paths, batches with
an empty image, the HalfSIFT twins, graphs, the refusals, the pipeline, and that pooling switched off costs nothing."""
import ctypes as C

import numpy as np
import pytest

import dsp_ref
import orc
import synth
from test_gpu_describe import RFIELDS, _assert_regions_equal
from test_gpu_describe_u8_keys import _border_key, _iso_key, _oracle, _sift_constants

pytestmark = pytest.mark.gpu

W, H = 320, 240
CONFIGS = [(3, 0.5, 1.5), (2, 1.0, 2.0), (8, 0.5, 4.0)]
FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_int))


def _p2_at(s, c):
    """side of the window the extraction samples for a region of scale s at the domain c * mrSize (region_geom, csrc/sift.hip)"""
    return 2 * int(np.ceil(s * (orc.DESC_MRSIZE * c))) + 3


# ---- 1. the kernels on crafted patch sets -----------------------------------------------------------------------------------------
def _patch_set(K, ps, seed, flat_first):
    """K patches of one region: textures at different zooms, a step edge and a single bright pixel among them"""
    rng = np.random.RandomState(seed)
    tex = synth.texture(160, 120, seed=seed)
    yy, xx = np.mgrid[0:ps, 0:ps]
    out = []
    for k in range(K):
        kind = (k + seed) % 4
        if kind == 0:
            y0, x0 = rng.randint(0, 120 - ps), rng.randint(0, 160 - ps)
            p = tex[y0:y0 + ps, x0:x0 + ps].copy()
        elif kind == 1:
            p = np.where(xx * (k + 1) + yy * 2 < ps * (k + 2) // 2, 30.0, 220.0)
        elif kind == 2:
            p = np.full((ps, ps), 12.0)
            p[ps // 2 - k, ps // 2 + 2] = 255.0
        else:
            p = rng.randint(0, 256, (ps, ps)) * 1.0
        out.append(np.asarray(p, np.float32))
    if flat_first:
        out[0] = np.full((ps, ps), 131.0, np.float32)      # variance 0 < 1e-4: no photometric pass, and h_0 = 0
    return np.stack(out)


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("ps", [41, 33, 47])
def test_sift_pooled_kernels(pkg, gpu_ctx, K, ps):
    """mods_test_sift_pooled: RootSIFT and SIFT, half on and off, photoNorm on and off, clipping at two levels; one set has its
    first scale flat and the others textured.  Patch sizes 41 and 33 accumulate in the wave form (sift_wave2_kernel), 47 in the
    block-per-region form (dsp_accumulate_kernel), as the describe stage does."""
    n = 0
    for seed, flat_first in ((1, False), (2, False), (3, True)):
        patches = _patch_set(K, ps, seed + 10 * K, flat_first)
        if flat_first:
            assert not dsp_ref.raw_histogram(patches[0]).any() and dsp_ref.pooled_histogram(patches).any()
        for photo in (False, True):
            pooled = dsp_ref.pooled_histogram(patches, photo)
            for rootsift in (True, False):
                for half in (False, True):
                    for max_bin in (0.2, 0.08):
                        want = dsp_ref.tail(pooled, rootsift, max_bin, half)
                        got = gpu_ctx.sift_pooled(patches, rootsift, half, photo, max_bin)
                        assert np.array_equal(got, want), (seed, photo, rootsift, half, max_bin, np.nonzero(got != want)[0][:8])
                        assert want.any() and (not half or not want[64:].any())
                        n += 1
    assert n == 48


def test_sift_pooled_of_one_patch_is_sift_patch(pkg, gpu_ctx):
    """K = 1 through the pooled kernels = the unpooled kernel and the oracle"""
    p = _patch_set(1, 41, 7, False)
    want = orc.sift_desc(p[0], True, 0.2)
    assert np.array_equal(gpu_ctx.sift_pooled(p), want) and np.array_equal(gpu_ctx.sift_patch(p[0]), want)


# ---- 2. chosen keypoints ----------------------------------------------------------------------------------------------------------
SCALES = [1.2, 1.9, 2.6, 3.1, 3.9, 4.4, 5.1, 6.0, 7.0]


@pytest.fixture(scope="module")
def keys_case():
    """320 x 240, 40 isotropic keys: nine scales on a 3 x 3 grid of places (and again at other places), and four regions next to the
    four borders whose unpooled window already touches the border.  The oracle's regions (orientation, border filter, unpooled
    descriptors) and the pooled raw histograms, computed once."""
    img = synth.texture(W, H, seed=61)
    base = orc.detect_hessian_affine(img)[:1].copy()
    keys = []
    for i, s in enumerate(SCALES * 4):
        gx, gy = i % 6, (i // 6) % 6
        keys.append(_iso_key(base, 100.5 + 24.25 * gx, 96.25 + 9.5 * gy, s))
    for side, s in enumerate((2.6, 3.9, 4.4, 3.1)):
        keys.append(_border_key(img, base, s, side))
    keys = np.concatenate(keys)
    want = _oracle(img, keys)
    assert len(keys) == 40 and len(want) >= 36, len(want)
    return img, keys, want, dsp_ref.Describer(img, want)


def _want_pooled(want, desc):
    out = want.copy()
    out["desc"] = desc
    return out


def test_keys_cover_the_tiers_and_the_borders(keys_case):
    """for (3, 0.5, 1.5): the direct branch, the three LDS tiers and the big tier are each entered between the smallest and the
    largest domain of some region; the border regions' largest domains hold samples from outside the image"""
    img, keys, want, _ = keys_case
    k = _sift_constants()
    direct = max(P + 2 for P in range(1, 64, 2) if float(np.float32(P) / np.float32(orc.DESC_PATCH)) <= 0.4)
    for limit in (direct, k["t_lo"], k["t_mid"], k["small_cap"]):
        crossing = [s for s in want["s"] if _p2_at(s, 0.5) <= limit < _p2_at(s, 1.5)]
        assert crossing, limit
    assert max(_p2_at(s, 4.0) for s in want["s"]) > H                  # (8, 0.5, 4.0): windows taller than the image
    for r in want[-4:]:
        x, y, half = r["x"], r["y"], np.ceil(r["s"] * orc.DESC_MRSIZE * 1.5)
        assert min(x, y, W - 1 - x, H - 1 - y) < half                   # the axis-aligned half window alone passes the border


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "K%d-%g-%g" % c)
def test_orient_describe_pooled(pkg, keys_case, cfg):
    img, keys, want, ref = keys_case
    ctx = pkg.Context(0, W, H, 1)
    try:
        unpooled = ctx.orient_describe(img, keys)
        _assert_regions_equal(unpooled, want)
        ctx.set_domain_pooling(*cfg)
        assert ctx.domain_pooling() == cfg
        got = ctx.orient_describe(img, keys)
        for f in RFIELDS:
            assert np.array_equal(got[f], unpooled[f]), f
        exp = _want_pooled(want, ref.descriptors(*cfg))
        _assert_regions_equal(got, exp)
        assert (got["desc"] != unpooled["desc"]).any(axis=1).sum() > len(want) // 2
        ctx.set_domain_pooling(0)
        assert ctx.domain_pooling() == (0, 0.0, 0.0)
        assert ctx.orient_describe(img, keys).tobytes() == unpooled.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("ps", [41, 47])
def test_pooled_plain_sift_without_photonorm(pkg, keys_case, ps):
    """the other branches of the tail and of the accumulation through the describe entry point, at the default patch size and at
    one that takes the block-per-region kernels"""
    img, keys, want, _ = keys_case
    ref = dsp_ref.Describer(img, want[::3], ps=ps, photonorm=False)
    par = pkg.DescribeParams.default()
    par.photoNorm, par.rootSift, par.maxBinValue, par.desc_patchSize = 0, 0, 0.15, ps
    ctx = pkg.Context(0, W, H, 1)
    try:
        ctx.set_domain_pooling(3, 0.5, 1.5)
        got = ctx.orient_describe(img, keys, par)
        assert len(got) == len(want)
        assert np.array_equal(got["desc"][::3], ref.descriptors(3, 0.5, 1.5, rootsift=False, max_bin=0.15))
    finally:
        ctx.close()


# ---- 3. the 8-bit paths and batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", [-1, 15])
def test_orient_describe_u8_pooled(pkg, keys_case, kernels):
    img, keys, want, ref = keys_case
    assert np.array_equal(img, np.round(img)) and img.min() >= 0 and img.max() <= 255
    ctx = pkg.Context(0, W, H, 1)
    try:
        ctx.set_u8_kernels(kernels)
        ctx.set_domain_pooling(3, 0.5, 1.5)
        got = ctx.orient_describe_u8(img.astype(np.uint8), keys)
        assert ctx.u8_source_calls() == 1
        _assert_regions_equal(got, _want_pooled(want, ref.descriptors(3, 0.5, 1.5)))
    finally:
        ctx.close()


BW, BH = 320, 240
DET_THRESHOLD = 2.5         # times the default: some 80 regions per image instead of 250 (the reference is computed per region)


def _det(cls):
    det = cls.default()
    det.threshold *= DET_THRESHOLD
    return det


@pytest.fixture(scope="module")
def batch_case():
    """three 320 x 240 images, the middle one blank (no regions); the oracle's detect + describe and the pooled histograms"""
    imgs = [synth.texture(BW, BH, seed=71), np.full((BH, BW), 127.0, np.float32), synth.texture(BW, BH, seed=73)]
    want = [orc.detect_describe(im, _det(orc.HessAffParams)) for im in imgs]
    assert len(want[1][0]) == 0 and len(want[0][0]) > 30 and len(want[2][0]) > 30, [len(x[0]) for x in want]
    refs = [dsp_ref.Describer(im, regs) for im, (regs, _) in zip(imgs, want)]
    return np.stack(imgs), want, refs


def _check_batch(ctx, nd, nr, want, refs, cfg):
    out = []
    for i, ((regs, n_det), ref) in enumerate(zip(want, refs)):
        assert nd[i] == n_det and nr[i] == len(regs)
        got = ctx.regions_fetch(i)
        _assert_regions_equal(got, _want_pooled(regs, ref.descriptors(*cfg)) if cfg else regs)
        out.append(got.tobytes())
    return out


@pytest.mark.parametrize("kernels", [-1, 15])
def test_detect_describe_batch_pooled_fp32_and_u8(pkg, batch_case, kernels):
    import torch
    batch, want, refs = batch_case
    t32 = torch.from_numpy(batch).cuda()
    t8 = torch.from_numpy(batch.astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    c32, c8 = pkg.Context(0, BW, BH, 3), pkg.Context(0, BW, BH, 3)
    try:
        c8.set_u8_kernels(kernels)
        for c in (c32, c8):
            c.set_domain_pooling(3, 0.5, 1.5)
        nd, nr = c32.detect_describe_dev(t32.data_ptr(), 3, BW, BH, _det(pkg.HessAffParams))
        a = _check_batch(c32, nd, nr, want, refs, (3, 0.5, 1.5))
        nd, nr = c8.detect_describe_dev_u8(t8.data_ptr(), 3, BW, BH, _det(pkg.HessAffParams))
        assert c8.u8_source_calls() == 1
        assert _check_batch(c8, nd, nr, want, refs, (3, 0.5, 1.5)) == a
        # a batch of one image with no regions, and a partial batch that ends with it
        nd, nr = c32.detect_describe_dev(t32[1:].data_ptr(), 1, BW, BH, _det(pkg.HessAffParams))
        assert nr == [0] and len(c32.regions_fetch(0)) == 0
        nd, nr = c32.detect_describe_dev(t32.data_ptr(), 2, BW, BH, _det(pkg.HessAffParams))
        _check_batch(c32, nd, nr, want[:2], refs[:2], (3, 0.5, 1.5))
    finally:
        c32.close(); c8.close()


# ---- 4. HalfSIFT ----------------------------------------------------------------------------------------------------------------------
def test_half_descriptors_pooled(pkg, keys_case):
    img, keys, want, ref = keys_case
    par = pkg.DescribeParams.default()
    par.halfDesc = 1
    ctx = pkg.Context(0, W, H, 1)
    try:
        ctx.set_domain_pooling(3, 0.5, 1.5)
        full_alone = ctx.orient_describe(img, keys)
        with pytest.raises(pkg.ModsError, match="did not ask"):
            ctx.regions_fetch_half(0)
        full = ctx.orient_describe(img, keys, par)
        half = ctx.regions_fetch_half(0)
        assert full.tobytes() == full_alone.tobytes()
        _assert_regions_equal(full, _want_pooled(want, ref.descriptors(3, 0.5, 1.5)))
        _assert_regions_equal(half, _want_pooled(want, ref.descriptors(3, 0.5, 1.5, half=True)))
        assert not half["desc"][:, 64:].any() and half["desc"][:, :64].any(axis=1).all()
    finally:
        ctx.close()


# ---- 5. graphs ------------------------------------------------------------------------------------------------------------------------
def test_graphs_with_pooling_switched_on_and_off(pkg, batch_case):
    """One context with mods_ctx_graphs: three calls each with pooling on, off, and on with other coefficients.  The batch is the
    three images nineteen times over - the smallest multiple whose scale space forks onto the side stream, which is what makes
    a recording replayable (csrc/pyramid.hip) - so the unpooled calls do replay, and no recording survives a change of the
    setting: pooled calls are issued eagerly."""
    import torch
    batch, want, refs = batch_case
    reps = 19
    n_img = 3 * reps
    det = _det(pkg.HessAffParams)
    assert BW * BH * n_img >= 4 << 20 and BW * BH * (n_img - 3) < 4 << 20
    t = torch.from_numpy(np.tile(batch, (reps, 1, 1))).cuda()
    torch.cuda.synchronize()
    ctx, fresh = pkg.Context(0, BW, BH, n_img, nonblocking=True), pkg.Context(0, BW, BH, n_img)
    try:
        fresh.detect_describe_dev(t.data_ptr(), n_img, BW, BH, det)
        off = [fresh.regions_fetch(i).tobytes() for i in range(n_img)]
        ctx.graphs(True)
        replays = []
        for cfg in ((3, 0.5, 1.5), None, (2, 1.0, 2.0)):
            ctx.set_domain_pooling(*(cfg or (0, 0.0, 0.0)))
            exp = [_want_pooled(regs, ref.descriptors(*cfg)) if cfg else regs for (regs, _), ref in zip(want, refs)]
            for call in range(3):
                nd, nr = ctx.detect_describe_dev(t.data_ptr(), n_img, BW, BH, det)
                for i in (range(n_img) if call == 2 else (0, 1, 2, n_img - 1)):      # every slot behind the phase's last call
                    got = ctx.regions_fetch(i)
                    assert nr[i] == len(exp[i % 3])
                    _assert_regions_equal(got, exp[i % 3])
                    if cfg is None:
                        assert got.tobytes() == off[i]
            replays.append(ctx.graph_replays())
        print("graph replays after the pooled, the unpooled and the second pooled calls: %s" % replays)
        assert replays[0] == 0 and replays[1] >= 1 and replays[2] == replays[1]
    finally:
        ctx.close(); fresh.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
DESCRIBE_STAGES = ["blur", "response", "nms", "orient", "describe", "extract", "sift", "pyramid"]


def test_refusals(pkg, keys_case):
    import torch
    import nets_ref
    img, keys, want, _ = keys_case
    t = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, W, H, 1)
    try:
        d = C.c_double
        for K, a, b, word in [(9, 0.5, 1.5, "numScales"), (3, 0.0, 1.5, "startCoef"), (3, -1.0, 1.5, "startCoef"), (3, 1.5, 1.5, "endCoef"),
                              (3, 1.5, 1.0, "endCoef"), (3, 0.5, 4.5, "endCoef"), (3, float("nan"), 1.5, "startCoef"), (3, 0.5, float("nan"), "endCoef")]:
            with pytest.raises(pkg.ModsError, match=word):
                ctx.set_domain_pooling(K, a, b)
            assert ctx.domain_pooling() == (0, 0.0, 0.0)
        ctx.set_domain_pooling(1, -7.0, float("nan"))                   # one domain: off, the coefficients are not looked at
        assert ctx.domain_pooling() == (0, 0.0, 0.0)
        ctx.set_domain_pooling(3, 0.5, 1.5)
        ctx.timing_enable(DESCRIBE_STAGES)
        ctx.timing_reset()

        def refused(par=None):
            with pytest.raises(pkg.ModsError, match="domain-size pooling"):
                ctx.orient_describe(img, keys, par)
            with pytest.raises(pkg.ModsError, match="domain-size pooling"):
                ctx.detect_describe_dev(t.data_ptr(), 1, W, H, None, par)
            assert [ctx.timing_read(s)[1] for s in DESCRIBE_STAGES] == [0] * len(DESCRIBE_STAGES)
        fast = pkg.DescribeParams.default()
        fast.fastExtraction = 1
        refused(fast)
        calls = []

        def fn(user, patches, n, ps, out, cap, dim):
            calls.append(n)
            return 1
        cb = FN(fn)
        ctx.set_external_descriptor(C.cast(cb, C.c_void_p).value, None, 5.1962, 32)
        refused()
        assert not calls
        ctx.set_external_descriptor(None, None)
        net = pkg.Net("hardnet", nets_ref.synthetic_state("hardnet", 3))
        ctx.set_builtin_descriptor(net, 5.1962, True)
        refused()
        ctx.set_builtin_descriptor(None)
        ctx.timing_enable([])
        assert len(ctx.orient_describe(img, keys)) == len(want)          # the context is usable afterwards
    finally:
        ctx.close()


def test_external_orientation_hook_is_compatible(pkg, keys_case):
    """an orientation hook runs before description: the pooled call describes the hook's regions"""
    img, keys, want, _ = keys_case

    def fn(user, patches, n, ps, out, cap, dim):
        for i in range(n):
            out[2 * i], out[2 * i + 1] = 0.0, 1.0                       # atan2(0, 1): no rotation
        dim[0] = 2
        return 0
    cb = FN(fn)
    ctx = pkg.Context(0, W, H, 1)
    try:
        ctx.set_external_orientation(C.cast(cb, C.c_void_p).value, None, 5.1962, 32)
        unpooled = ctx.orient_describe(img, keys)
        assert len(unpooled) >= 30
        ctx.set_domain_pooling(2, 1.0, 2.0)
        got = ctx.orient_describe(img, keys)
        for f in RFIELDS:
            assert np.array_equal(got[f], unpooled[f]), f
        assert np.array_equal(got["desc"], dsp_ref.Describer(img, unpooled).descriptors(2, 1.0, 2.0))
    finally:
        ctx.close()


# ---- 7. the pipeline --------------------------------------------------------------------------------------------------------------------
def test_pipeline_pooled(pkg):
    import torch
    pairs = [synth.pair(W, H, seed=s)[:2] for s in (7, 9)]
    dev = [torch.from_numpy(np.stack(p)).cuda() for p in pairs]
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    cfg = (3, 0.5, 1.5)
    ctx = pkg.Context(0, W, H, 2)
    try:
        pkg.ransac_pin_seed(7)
        ctx.set_domain_pooling(*cfg)
        want = [pkg.match_pair_dev(ctx, x.data_ptr(), W, H, par, max_matches=10000) for x in dev]
        results = {}
        for pooled in (True, False):
            pipe = pkg.Pipeline(0, W, H, par, 1, 2, 2)
            try:
                if pooled:
                    pipe.set_domain_pooling(*cfg)
                for i, x in enumerate(dev):
                    pipe.submit(x.data_ptr(), i)
                if pooled:
                    with pytest.raises(pkg.ModsError, match="after the first submit"):
                        pipe.set_domain_pooling(0)
                results[pooled] = [pipe.next_matches(10000) for _ in dev]
            finally:
                pipe.close()
        for i, (exp, m_exp) in enumerate(want):
            res, tag, m = results[True][i]
            assert tag == i and list(res.n_described) == list(exp.n_described)
            for f in ("n_tentatives", "n_unique", "n_inliers", "ransac_samples"):
                assert getattr(res, f) == getattr(exp, f), (f, i)
            assert np.array_equal(m, m_exp) and res.n_inliers > 0
            plain = results[False][i][0]
            print("pair %d: %d tentatives pooled, %d unpooled" % (i, res.n_tentatives, plain.n_tentatives))
            assert list(plain.n_described) == list(res.n_described) and plain.n_tentatives != res.n_tentatives
    finally:
        pkg.ransac_pin_seed(-1)
        ctx.close()


# ---- 8. off is free -----------------------------------------------------------------------------------------------------------------------
def test_pooling_switched_off_is_free(pkg, keys_case):
    img, keys, want, _ = keys_case
    stages = ["describe", "extract", "sift"]
    par = pkg.DescribeParams.default()
    par.halfDesc = 1
    fresh, ctx = pkg.Context(0, W, H, 1), pkg.Context(0, W, H, 1)
    try:
        out = []
        for c in (fresh, ctx):
            if c is ctx:
                c.set_domain_pooling(3, 0.5, 1.5)
                c.orient_describe(img, keys, par)
                c.set_domain_pooling(0)
            c.timing_enable(stages)
            c.timing_reset()
            regs = c.orient_describe(img, keys, par)
            out.append((regs.tobytes(), c.regions_fetch_half(0).tobytes(), [c.timing_read(s)[1] for s in stages]))
        print("launch scopes (describe, extract, sift) of an unpooled call: %s" % out[0][2])
        assert out[0] == out[1] and all(n > 0 for n in out[0][2])
        ctx.set_domain_pooling(3, 0.5, 1.5)
        ctx.timing_reset()
        ctx.orient_describe(img, keys, par)
        pooled = [ctx.timing_read(s)[1] for s in stages]
        print("... of a pooled call with three domains: %s" % pooled)
        assert pooled[1] == 3 * out[0][2][1] and pooled[2] > out[0][2][2]
    finally:
        fresh.close(); ctx.close()
