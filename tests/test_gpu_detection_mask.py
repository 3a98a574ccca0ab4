"""-m gpu tests of the detection masks (include/mods_hip.h, "detection masks"): a masked call returns what the unmasked call
returns with the off-mask entries deleted (FixedTh), masked points never reach the affine adaptation, the selection modes see
on-mask points only, and the same holds for views, MSER, recorded graphs, the pair, ladder and pipeline entry points and the
command line.  Every equivalence test first makes sure its mask both keeps and removes at least 5 entries
(detection_mask_ref.assert_non_vacuous); the counts below are the CPU oracle's for tests/synth.texture."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import detection_mask_ref as ref
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
W, H = 256, 192
KEY_FIELDS = ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "octave", "level", "r0", "c0")


def _det(pkg, det, **over):
    p = {"hessian": pkg.HessAffParams.default, "dog": pkg.HessAffParams.dog, "harris": pkg.HessAffParams.harris}[det]()
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _same_keys(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in KEY_FIELDS:
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8), np.ascontiguousarray(want[f]).view(np.uint8)), f


@pytest.fixture(scope="module")
def batch():
    """two 256 x 192 images and a different mask for each: per-pixel random (the rounding of the centre decides), and a
    checkerboard handed over with a row stride of w + 13 and poisoned padding"""
    import torch
    imgs = np.stack([synth.texture(W, H, seed=1), synth.texture(W, H, seed=2)])
    masks = [ref.random_pixels(W, H), ref.with_row_padding(ref.checkerboard(W, H), pad=13, poison=255)]
    assert masks[1].strides[0] == W + 13
    t = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    return imgs, masks, t


@pytest.fixture(scope="module")
def ctx2(pkg):
    ctx = pkg.Context(0, W, H, 2)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("det", ["hessian", "dog", "harris"])
def test_fixed_th_equals_the_filtered_unmasked_lists(pkg, ctx2, batch, det):
    """keys (detect_hessian_affine_dev) and regions with descriptors (detect_describe_dev) of a batch of 2 with a mask each.
    Oracle counts for HessianAffine: 173 keys / 141 regions of image 0, 97 / 82 on its mask; 151 / 94 of image 1, 71 / 44."""
    _, masks, t = batch
    par = _det(pkg, det)
    ctx2.clear_detection_masks()
    keys0 = ctx2.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par)
    nd0, nr0 = ctx2.detect_describe_dev(t.data_ptr(), 2, W, H, det=par)
    regs0 = [ctx2.regions_fetch(i) for i in range(2)]
    assert nd0 == [len(k) for k in keys0]
    for i in range(2):
        ref.assert_non_vacuous(keys0[i], masks[i])
        ref.assert_non_vacuous(regs0[i], masks[i])
        ctx2.set_detection_mask(i, masks[i])
    keys1 = ctx2.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par)
    counts = [ctx2.detection_mask_counts(i) for i in range(2)]
    nd1, nr1 = ctx2.detect_describe_dev(t.data_ptr(), 2, W, H, det=par)
    for i in range(2):
        _same_keys(keys1[i], ref.filter_regions(keys0[i], masks[i]))
        want = ref.filter_regions(regs0[i], masks[i])
        got = ctx2.regions_fetch(i)
        ref.assert_same_but_positions(got, want)
        assert nd1[i] == len(keys1[i]) and nr1[i] == len(want)
        assert np.array_equal(got["id"], np.arange(len(got)))
        assert counts[i][0] > counts[i][1] >= len(keys1[i])
    # one image masked, the other not: the unmasked one is untouched, id / parent included
    ctx2.set_detection_mask(0, None)
    keys2 = ctx2.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par)
    ctx2.detect_describe_dev(t.data_ptr(), 2, W, H, det=par)
    _same_keys(keys2[0], keys0[0])
    assert ctx2.regions_fetch(0).tobytes() == regs0[0].tobytes()
    _same_keys(keys2[1], ref.filter_regions(keys0[1], masks[1]))
    assert ctx2.detection_mask_counts(0) == (-1, -1)
    ctx2.clear_detection_masks()


def test_all_on_and_all_off_masks(pkg, ctx2, batch):
    _, _, t = batch
    par = _det(pkg, "hessian")
    ctx2.clear_detection_masks()
    keys0 = ctx2.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par)
    ctx2.detect_describe_dev(t.data_ptr(), 2, W, H, det=par)
    regs0 = [ctx2.regions_fetch(i) for i in range(2)]
    assert min(len(r) for r in regs0) > 20
    ctx2.set_detection_mask(0, np.full((H, W), 255, np.uint8))
    ctx2.set_detection_mask(1, np.zeros((H, W), np.uint8))
    keys1 = ctx2.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par)
    nd, nr = ctx2.detect_describe_dev(t.data_ptr(), 2, W, H, det=par)          # MODS_OK with an empty list
    _same_keys(keys1[0], keys0[0])
    assert ctx2.regions_fetch(0).tobytes() == regs0[0].tobytes()                # id / parent included
    assert len(keys1[1]) == 0 and nd[1] == 0 and nr[1] == 0 and len(ctx2.regions_fetch(1)) == 0
    acc, kept = ctx2.detection_mask_counts(1)
    assert kept == 0 and acc > 20
    acc0, kept0 = ctx2.detection_mask_counts(0)
    assert acc0 == kept0 > 20
    # a mask of another size than the image of the call is an error, not a silent no-op
    ctx2.set_detection_mask(1, np.full((H, W - 1), 255, np.uint8))
    with pytest.raises(pkg.ModsError, match="detection mask"):
        ctx2.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par)
    ctx2.clear_detection_masks()
    _same_keys(ctx2.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par)[1], keys0[1])


def test_masked_points_cost_nothing_downstream(pkg, batch):
    """the Baumberg work counter: the masked run adapts n_kept points, and n_accepted is what the unmasked run adapts"""
    imgs, masks, t = batch
    ctx = pkg.Context(0, W, H, 2)
    try:
        par = _det(pkg, "hessian")
        ctx.baumberg_stats_enable(True)
        ctx.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par, fetch=False)
        plain = [ctx.baumberg_stats(i)[0] for i in range(2)]
        for i in range(2):
            ctx.set_detection_mask(i, masks[i])
        ctx.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par, fetch=False)
        for i in range(2):
            acc, kept = ctx.detection_mask_counts(i)
            assert acc == plain[i] > 100
            assert ctx.baumberg_stats(i)[0] - plain[i] == kept and 5 <= kept <= acc - 5
        # no mask: the LOCALIZE stage is the launches it was (one scope per call), with a mask it still is one scope
        ctx.clear_detection_masks()
        ctx.timing_enable(["localize"])
        ctx.detect_hessian_affine_dev(t.data_ptr(), 2, W, H, par, fetch=False)
        assert ctx.timing_read("localize")[1] == 1
    finally:
        ctx.close()


def test_mask_first_then_select(pkg, batch):
    """FixedRegNumber and RelativeTh see on-mask points only.  Oracle: 303 candidates of image 0 with thresholds 0, 117 on the
    half-plane mask; 26 of the 80 strongest are on it, so a cut at 40 before the mask would keep about 13."""
    imgs, _, t = batch
    hp = ref.half_plane(W, H)
    ctx = pkg.Context(0, W, H, 1)
    try:
        every = ctx.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, _det(pkg, "hessian", mode=2, regionsNumber=100000))[0]
        on = ref.filter_regions(every, hp)
        assert len(every) < 100000 and len(on) >= 45 and len(every) - len(on) >= 5
        assert ref.on_mask(hp, every["x"][:40], every["y"][:40]).sum() <= 35
        ctx.set_detection_mask(0, hp)
        got = ctx.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, _det(pkg, "hessian", mode=2, regionsNumber=40))[0]
        _same_keys(got, on[:40])
        rel = float(np.float32(0.25))
        got = ctx.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, _det(pkg, "hessian", mode=1, relativeThreshold=rel))[0]
        thr = float(np.float32(abs(on["response"][0]) * rel))          # the float effectiveThreshold of pyramid.h:74, off the on-mask maximum
        want = on[np.abs(on["response"]) > abs(thr)]
        assert abs(on["response"][0]) < abs(every["response"][0]) or len(want) < (np.abs(every["response"]) > abs(thr)).sum()
        assert 5 <= len(want) <= len(on) - 5
        _same_keys(got, want)
    finally:
        ctx.close()


def test_views(pkg):
    """tilt 2, phi 60 degrees of 320 x 240: the mask lives in the original frame, the gate tests the reprojected centres"""
    import torch
    w, h = 320, 240
    img = synth.texture(w, h, seed=3)
    cb = ref.checkerboard(w, h)
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    try:
        t = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        ctx.detect_describe_view_dev(t.data_ptr(), w, h, 2.0, math.pi / 3)
        regs0 = ctx.regions_fetch(0)
        ref.assert_non_vacuous(regs0, cb)
        ctx.set_detection_mask(0, cb)
        _, nd, nr = ctx.detect_describe_view_dev(t.data_ptr(), w, h, 2.0, math.pi / 3)
        got = ctx.regions_fetch(0)
        ref.assert_same_but_positions(got, ref.filter_regions(regs0, cb))
        assert nr == len(got) and ref.on_mask(cb, got["x"], got["y"]).all()
        acc, kept = ctx.detection_mask_counts(0)
        assert acc > kept >= nd
        # the mask's size is the ORIGINAL image's: one of the view's size is refused
        g = pkg.view_geometry(w, h, 2.0, math.pi / 3, 1.0, 0.2)
        assert (g.w_new, g.h_new) != (w, h)
        ctx.set_detection_mask(0, np.full((g.h_new, g.w_new), 255, np.uint8))
        with pytest.raises(pkg.ModsError, match="detection mask"):
            ctx.detect_describe_view_dev(t.data_ptr(), w, h, 2.0, math.pi / 3)
    finally:
        ctx.close()


def test_mser(pkg, batch):
    """the exported MSER key list loses its off-mask keys, order kept (oracle: 122 keys of image 0, 59 on the checkerboard)"""
    imgs, _, t = batch
    cb = ref.checkerboard(W, H)
    ctx = pkg.Context(0, W, H, 1)
    try:
        par = pkg.HessAffParams.mser()
        keys0 = ctx.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, par)[0]
        ctx.detect_describe_dev(t.data_ptr(), 1, W, H, det=par)
        regs0 = ctx.regions_fetch(0)
        ref.assert_non_vacuous(keys0, cb)
        ref.assert_non_vacuous(regs0, cb)
        ctx.set_detection_mask(0, cb)
        keys1 = ctx.detect_hessian_affine_dev(t.data_ptr(), 1, W, H, par)[0]
        _same_keys(keys1, ref.filter_regions(keys0, cb))
        assert ctx.detection_mask_counts(0) == (len(keys0), len(keys1))
        ctx.detect_describe_dev(t.data_ptr(), 1, W, H, det=par)
        ref.assert_same_but_positions(ctx.regions_fetch(0), ref.filter_regions(regs0, cb))
    finally:
        ctx.close()


def test_recorded_graphs(pkg):
    """ctx.graphs(True) on a batch whose scale space forks (2 x 2048 x 1024, the calls that are recorded): unmasked, unmasked
    (replayed), masked, masked with other mask contents behind the same device pointer (replayed), cleared - each equals its eager
    counterpart, and no replay reads a stale mask"""
    import torch
    w, h = 2048, 1024
    tile = synth.texture(512, 256, seed=4)
    img = np.tile(tile, (4, 4))
    imgs = np.stack([img, img[::-1].copy()])
    m1 = np.stack([ref.half_plane(w, h), ref.checkerboard(w, h)])
    m2 = np.stack([ref.checkerboard(w, h, 32), ref.half_plane(w, h)[:, ::-1].copy()])
    t = torch.from_numpy(imgs).cuda()
    md = torch.from_numpy(m1).cuda()
    torch.cuda.synchronize()

    def run(ctx, record):
        out = []
        ctx.detect_describe_dev(t.data_ptr(), 2, w, h)          # (the call that sizes the context's pools is never a repeat)
        ctx.graphs(record)

        def call():
            ctx.detect_describe_dev(t.data_ptr(), 2, w, h)
            out.append([ctx.regions_fetch(i).tobytes() for i in range(2)])
        call(); call()
        for i in range(2):
            ctx.set_detection_mask_dev(i, md.data_ptr() + i * w * h, w, h)
        md.copy_(torch.from_numpy(m1)); torch.cuda.synchronize()
        call()
        md.copy_(torch.from_numpy(m2)); torch.cuda.synchronize()
        call()
        ctx.clear_detection_masks()
        call()
        return out

    eager, graphs = pkg.Context(0, w, h, 2), pkg.Context(0, w, h, 2)
    try:
        want = run(eager, False)
        got = run(graphs, True)
        assert graphs.graph_replays() >= 2 and eager.graph_replays() == 0
        assert got == want
        assert want[0] == want[1] == want[4] and want[2] != want[3] and want[2] != want[0]
    finally:
        eager.close(); graphs.close()


def _pair_setup():
    w, h = 320, 240
    a, b, _ = synth.pair(w, h)
    masks = [ref.half_plane(w, h), ref.checkerboard(w, h, 32)]
    return w, h, a, b, masks


def test_ladder_banks_and_tentatives(pkg):
    """match_ladder_dev with masks on both images, the views spread over the ladder's worker contexts: the banks are the unmasked
    banks filtered, and the search over them is the search over banks rebuilt from the filtered lists"""
    import torch
    w, h, a, b, masks = _pair_setup()
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 2)
    reps = [pkg.ImgRep(ctx) for _ in range(4)]
    try:
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        steps = [pkg.LadderStep.make((1, 2), 360.0)]
        pkg.ransac_pin_seed(5)
        res0, _ = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, reps[0], reps[1], min_matches=10 ** 6, max_matches=100000)
        assert res0.n_views >= 4
        for i in range(2):
            ctx.set_detection_mask(i, masks[i])
        pkg.ransac_pin_seed(5)
        res1, m1 = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, reps[2], reps[3], min_matches=10 ** 6, max_matches=100000)
        ctx.clear_detection_masks()
        filtered = []
        for i in range(2):
            plain, got = reps[i].fetch(), reps[2 + i].fetch()
            ref.assert_non_vacuous(plain, masks[i])
            want = ref.filter_regions(plain, masks[i])
            ref.assert_same_but_positions(got, want)
            filtered.append(want)
        rq, rt = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
        try:
            rq.append_host(filtered[0]); rt.append_host(filtered[1])
            tent, u6, _ = pkg.match_reps(ctx, rq, rt)
        finally:
            rq.close(); rt.close()
        assert res1.n_tentatives == len(tent) > 20
        rows = {tuple(r) for r in u6[:, [0, 1, 3, 4]].tolist()}
        assert len(m1) == res1.n_inliers and all(tuple(r) in rows for r in m1.tolist())
        for x1, y1, x2, y2 in m1.tolist():
            assert ref.on_mask(masks[0], x1, y1) and ref.on_mask(masks[1], x2, y2)
    finally:
        for r in reps:
            r.close()
        ctx.close()


def test_ladder_counts_are_sums_over_the_views(pkg):
    import torch
    w, h, a, b, masks = _pair_setup()
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 2)
    rep1, rep2 = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
    try:
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        ctx.set_detection_mask(1, masks[1])
        res, _ = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, [pkg.LadderStep.make((1, 2), 360.0)], rep1, rep2, min_matches=10 ** 6)
        assert ctx.detection_mask_counts(0) == (-1, -1)
        acc, kept = ctx.detection_mask_counts(1)
        assert acc > kept >= res.n_detected[1] > 20
    finally:
        rep1.close(); rep2.close(); ctx.close()


def test_pair_and_pipeline(pkg):
    """Pipeline.submit_host(u8, mask=...) returns what match_pair_dev returns on a context with the same masks set; an unmasked
    pair in the same batch returns today's result"""
    import torch
    w, h, a, b, masks = _pair_setup()
    pkg.ransac_pin_seed(11)
    ctx = pkg.Context(0, w, h, 2)
    pipe = pkg.Pipeline(0, w, h, gpu_workers=1, verify_workers=1, pairs_per_batch=2)
    try:
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        plain, plain_m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, max_matches=10000)
        plain_regs = [ctx.regions_fetch(i) for i in range(2)]
        for i in range(2):
            ref.assert_non_vacuous(plain_regs[i], masks[i])
            ctx.set_detection_mask(i, masks[i])
        want, want_m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, max_matches=10000)
        for i in range(2):
            ref.assert_same_but_positions(ctx.regions_fetch(i), ref.filter_regions(plain_regs[i], masks[i]))
        assert 15 <= want.n_inliers < plain.n_inliers
        for x1, y1, x2, y2 in want_m.tolist():
            assert ref.on_mask(masks[0], x1, y1) and ref.on_mask(masks[1], x2, y2)
        u8 = pkg.PinnedBuffer((2, h, w), np.uint8)
        mk = pkg.PinnedBuffer((2, h, w), np.uint8)
        u8.array[:] = np.stack([a, b]).astype(np.uint8)
        mk.array[:] = np.stack(masks)
        pipe.submit_host(u8.ptr.value, tag=1, u8=True, mask=mk.ptr.value)
        pipe.submit_host(u8.ptr.value, tag=2, u8=True)
        pipe.submit_host(u8.ptr.value, tag=3, u8=True, mask=mk.ptr.value)
        got = [pipe.next_matches() for _ in range(3)]
        for (res, tag, m), (exp, exp_m) in zip(got, ((want, want_m), (plain, plain_m), (want, want_m))):
            for f in ("n_tentatives", "n_unique", "n_inliers"):
                assert getattr(res, f) == getattr(exp, f), (tag, f)
            assert list(res.n_detected) == list(exp.n_detected) and list(res.n_described) == list(exp.n_described)
            assert np.array_equal(m, exp_m) and list(res.H) == list(exp.H), tag
        u8.close(); mk.close()
    finally:
        pipe.close(); ctx.close()


def _cli(tmp_path, ini_tail, img1, img2):
    text = open(os.path.join(CFG, "classic.ini")).read() + "\n" + ini_tail + "\n"
    (tmp_path / "mask.ini").write_text(text)
    p = subprocess.run([MODS, img1, img2, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", str(tmp_path / "mask.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, env=dict(os.environ, MODS_RANSAC_SEED="4242"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return np.loadtxt(tmp_path / "m.txt", ndmin=2), p.stderr.decode()


def test_cli(pkg, tmp_path):
    """[DetectionMask] mask1 / mask2 on a 320 x 240 pair, then the same masks found as <stem>_mask.png: every row of the matchings
    file has both endpoints on the masks"""
    from test_cpu_detection_mask import write_png_grey
    w, h, a, b, masks = _pair_setup()
    g1, g6 = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    write_png_grey(g1, a.astype(np.uint8))
    write_png_grey(g6, b.astype(np.uint8))
    plain, _ = _cli(tmp_path, "", g1, g6)
    assert plain.shape[1] == 4
    off = ~(ref.on_mask(masks[0], plain[:, 0], plain[:, 1]) & ref.on_mask(masks[1], plain[:, 2], plain[:, 3]))
    assert off.sum() >= 5                      # the unmasked run does match through the masked parts
    write_png_grey(tmp_path / "ma.png", masks[0])
    write_png_grey(tmp_path / "mb.png", masks[1])
    named, _ = _cli(tmp_path, "[DetectionMask]\nmask1 = ma.png\nmask2 = mb.png", g1, g6)
    assert len(named) >= 5
    assert ref.on_mask(masks[0], named[:, 0], named[:, 1]).all() and ref.on_mask(masks[1], named[:, 2], named[:, 3]).all()
    shutil.copy(g1, tmp_path / "first.png")
    shutil.copy(g6, tmp_path / "second.png")
    shutil.copy(tmp_path / "ma.png", tmp_path / "first_mask.png")
    shutil.copy(tmp_path / "mb.png", tmp_path / "second_mask.png")
    found, _ = _cli(tmp_path, "[DetectionMask]\nuseMaskFiles = 1", str(tmp_path / "first.png"), str(tmp_path / "second.png"))
    assert np.array_equal(found, named)
    unused, _ = _cli(tmp_path, "[DetectionMask]\nuseMaskFiles = 0", str(tmp_path / "first.png"), str(tmp_path / "second.png"))
    assert np.array_equal(unused, plain)
