"""-m gpu tests of the homography views (include/mods_hip.h, "homography views"): the perspective warp and the post-pass against
the restatement of tests/view_h_ref.py to the bit, a whole view against the CPU oracle's plain-image path fed with the restated
warp, and the rematch step under a verified H on graf1 / graf6 and on a synthetic pair with a known homography."""
import os
import subprocess

import numpy as np
import pytest

import detection_mask_ref
import view_h_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
OW, OH = 320, 240

# a general homography of the 37 x 23 source
GENERAL = [1.7, 0.1, -2.0, 0.05, 0.4, -0.5, 1e-3, 2e-3, 1.0]       # (view pixel (0, 0) shows the source near (1.1, 1.1))
# det = -1024, so G = adj(H) / det(H) is exact: G6 = 1 / 32, G7 = 0, G8 = -1, W = x / 32 - 1 is 0 on column 32, negative left of it,
# positive right of it; d0 = 18 + 1 > 0: the columns right of 32 show the source, the others lie on or behind the horizon
HORIZON = [32.0, 0.0, 64.0, 0.0, 32.0, 32.0, 1.0, 0.0, 1.0]
# source x = 2^22 (x - 35): times 32 beyond the int range on both sides for |x - 35| >= 16
FAR = [2.0 ** -22, 0.0, 35.0, 0.0, 2.0 ** -22, 4.0, 0.0, 0.0, 1.0]
# view(x, y) = source(x - 0.5, y + 0.25): column 0 has sx = -1, column 37 has sx = sw - 1 (its right tap is outside)
HALF_PIXEL = [1.0, 0.0, 0.5, 0.0, 1.0, -0.25, 0.0, 0.0, 1.0]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0, OW, OH, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def src():
    return np.random.default_rng(5).uniform(0, 255, (23, 37)).astype(np.float32)


def _same_pixels(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("dw,dh", [(70, 9), (64, 4), (1, 1)])
def test_warp_equals_the_restatement(ctx, src, dw, dh):
    """tile tails in both axes, exactly one tile, one pixel; the source rows 41 floats apart (the gap holds NaNs)"""
    for Hm in (GENERAL, HALF_PIXEL):
        want = ref.warp_perspective(src, Hm, dw, dh, cval=77.0)
        _same_pixels(ctx.warp_perspective(src, Hm, dw, dh, cval=77.0, stride=41), want)
        assert not np.isnan(want).any() and (want != 77.0).any()
    _same_pixels(ctx.warp_perspective(src, GENERAL, dw, dh, cval=77.0), ref.warp_perspective(src, GENERAL, dw, dh, cval=77.0))   # dense rows


def test_warp_across_the_horizon_and_under_negation(ctx, src):
    G, d0 = ref.inverse_and_d0(HORIZON, 37, 23)
    x = np.arange(70, dtype=np.float64)
    Wd = ((G[6] * x + G[7] * 3.0) + G[8]) * d0
    assert Wd[32] == 0 and (Wd[:32] < 0).all() and (Wd[33:] > 0).all()
    want = ref.warp_perspective(src, HORIZON, 70, 9, cval=77.0)
    got = ctx.warp_perspective(src, HORIZON, 70, 9, cval=77.0, stride=41)
    _same_pixels(got, want)
    assert (got[:, :33] == 77.0).all() and (got[:, 33:] != 77.0).any()
    neg = ctx.warp_perspective(src, [-v for v in HORIZON], 70, 9, cval=77.0, stride=41)
    _same_pixels(neg, got)
    _same_pixels(ctx.warp_perspective(src, [-v for v in GENERAL], 70, 9, stride=41), ctx.warp_perspective(src, GENERAL, 70, 9, stride=41))


def test_warp_clamps_beyond_the_int_range(ctx, src):
    G, _ = ref.inverse_and_d0(FAR, 37, 23)
    fx = ((G[0] * np.arange(70.0) + G[1] * 0.0) + G[2]) * 32.0
    assert (fx < ref.INT_MIN).any() and (fx > ref.INT_MAX).any() and (np.abs(fx) < 2.0 ** 31).any()
    _same_pixels(ctx.warp_perspective(src, FAR, 70, 9, cval=77.0, stride=41), ref.warp_perspective(src, FAR, 70, 9, cval=77.0))


def test_warp_taps_on_the_source_edge(ctx, src):
    got = ctx.warp_perspective(src, HALF_PIXEL, 70, 9, cval=77.0, stride=41)
    _same_pixels(got, ref.warp_perspective(src, HALF_PIXEL, 70, 9, cval=77.0))
    # sx = -1 (column 0) and sx = sw - 1 (column 37): half cval, half source; row 0 has sy = 0, fy = 8 / 32
    v, w = np.float32(0.75) * np.float32(0.5), np.float32(0.25) * np.float32(0.5)      # the weights of the upper / lower taps
    c = np.float32(77.0)
    assert got[0, 0] == ((c * v + src[0, 0] * v) + c * w) + src[1, 0] * w             # the left taps are outside
    assert got[0, 37] == ((src[0, 36] * v + c * v) + src[1, 36] * w) + c * w          # the right taps are
    assert (got[:, 38:] == 77.0).all()


def test_warp_refuses_what_has_no_view(pkg, ctx, src):
    for bad in ([1, 2, 3, 2, 4, 6, 0, 0, 1], [1, 0, 0, 0, 1, 0, 2.0, 0, -36.0], [1, 0, 0, 0, 1, 0, 0, float("nan"), 1]):
        with pytest.raises(pkg.ModsError):
            ctx.warp_perspective(src, bad, 8, 8)


# ---- the post-pass
PROJ = [1.05, 0.04, 6.0, -0.03, 0.95, 9.0, 2e-4, -1e-4, 1.0]       # original (320 x 240) -> view


def _regions(pkg, n, seed, lo=-0.15, hi=1.15, s_max=6.0):
    """n regions of a view of the 320 x 240 original under PROJ, centres the images of original points in [lo, hi] of its extent"""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, pkg.REGION_DTYPE)
    pts = np.c_[rng.uniform(lo * OW, hi * OW, n), rng.uniform(lo * OH, hi * OH, n)]
    v = ref.apply_h(PROJ, pts) if n else np.zeros((0, 2))
    r["x"], r["y"] = v[:, 0], v[:, 1]
    r["s"] = rng.uniform(0.8, s_max, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    k = rng.uniform(0.6, 1.6, n)
    r["a11"], r["a12"], r["a21"], r["a22"] = k * np.cos(ang), -np.sin(ang) / k, k * np.sin(ang), np.cos(ang) / k
    r["response"] = rng.normal(size=n)
    r["sub_type"] = rng.integers(0, 3, n)
    r["id"] = np.arange(n)
    r["parent"] = rng.integers(0, 1 << 20, n)
    r["desc"] = rng.integers(0, 256, (n, 128))
    return r


def _same_regions(got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (len(got), len(want))
    assert got.tobytes() == want.tobytes(), [f for f in got.dtype.names if got[f].tobytes() != want[f].tobytes()]


@pytest.mark.parametrize("n", [0, 1, 256, 257, 1500])
def test_post_pass_equals_the_restatement(pkg, ctx, n):
    """a chunk of the kernel is 256 regions: an empty list, one region, exactly one chunk, a chunk and one, several chunks"""
    r = _regions(pkg, n, seed=100 + n, **(dict(lo=0.4, hi=0.6, s_max=1.0) if n == 1 else {}))
    want = ref.reproject_regions_h(r, PROJ, OW, OH)
    _same_regions(ctx.reproject_regions_h(r, PROJ, OW, OH), want)
    assert n != 1 or len(want) == 1
    if n >= 256:
        assert 0.2 * n < len(want) < 0.9 * n                    # both outcomes


def test_post_pass_all_kept_and_none_kept(pkg, ctx):
    r = _regions(pkg, 300, seed=3, lo=0.3, hi=0.7, s_max=1.5)
    want = ref.reproject_regions_h(r, PROJ, OW, OH)
    assert len(want) == 300
    _same_regions(ctx.reproject_regions_h(r, PROJ, OW, OH), want)
    r = _regions(pkg, 300, seed=4, lo=1.05, hi=1.5)
    assert len(ref.reproject_regions_h(r, PROJ, OW, OH)) == 0
    assert len(ctx.reproject_regions_h(r, PROJ, OW, OH)) == 0


def test_post_pass_strict_inequalities_sign_and_box(pkg, ctx):
    # a translation by (8, 16) is exact: view x = 8 is rx = 0, view x = 328 is rx = ow, view y = 16 / 256 are ry = 0 / oh
    T = [1.0, 0.0, 8.0, 0.0, 1.0, 16.0, 0.0, 0.0, 1.0]
    r = np.zeros(7, pkg.REGION_DTYPE)
    r["x"] = [8.0, 328.0, 168.0, 168.0, 168.0, 13.0, 8.0 + 2.0 ** -40]
    r["y"] = [136.0, 136.0, 16.0, 256.0, 136.0, 136.0, 136.0]
    r["s"] = [0.01, 0.01, 0.01, 0.01, 1.0, 1.0, 0.01]          # s = 0.01: a box of size 0, its four corners are the centre
    r["a11"] = r["a22"] = 1.0
    r["id"] = np.arange(7)
    r["parent"] = np.arange(7)
    want = ref.reproject_regions_h(r, T, OW, OH)
    got = ctx.reproject_regions_h(r, T, OW, OH)
    _same_regions(got, want)
    # kept: the centre of the image; (5, 120) is inside by its centre and dropped by its box; a centre 2^-40 right of 0 has
    # floor(x) <= 0 in the border test and goes too
    assert list(got["parent"]) == [4] and got["x"][0] == 160.0 and got["y"][0] == 120.0
    # den of the wrong sign alone: behind the horizon of G the centre lands inside the image with a tiny frame
    Hs = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0 / 256, 0.0, 1.0]
    G, d0 = ref.inverse_and_d0(Hs, OW, OH)
    b = np.zeros(2, pkg.REGION_DTYPE)
    b["x"], b["y"], b["s"] = [-10000.0, 100.0], [-3800.0, 100.0], 1.0
    b["a11"] = b["a22"] = 1.0
    b["parent"] = [0, 1]
    den = (G[6] * b["x"] + G[7] * b["y"]) + G[8]
    assert den[0] * d0 < 0 < den[1] * d0 and 0 < ((G[0] * b["x"][0] + G[2]) / den[0]) < OW and 0 < ((G[4] * b["y"][0] + G[5]) / den[0]) < OH
    got = ctx.reproject_regions_h(b, Hs, OW, OH)
    _same_regions(got, ref.reproject_regions_h(b, Hs, OW, OH))
    assert list(got["parent"]) == [1]


def test_post_pass_with_a_mask_and_a_twin_list(pkg, ctx):
    r = _regions(pkg, 700, seed=9, lo=0.1, hi=0.9, s_max=2.0)
    half = r.copy()
    half["desc"] = np.random.default_rng(1).integers(0, 256, (700, 128))
    mask = detection_mask_ref.with_row_padding(detection_mask_ref.random_pixels(OW, OH), pad=13, poison=255)
    plain = ref.reproject_regions_h(r, PROJ, OW, OH)
    want, want_half = ref.reproject_regions_h(r, PROJ, OW, OH, mask=mask, half=half)
    assert 50 < len(want) < len(plain) - 50
    ctx.set_detection_mask(0, mask)
    try:
        got, got_half = ctx.reproject_regions_h(r, PROJ, OW, OH, half=half)
        with pytest.raises(pkg.ModsError, match="detection mask"):
            ctx.reproject_regions_h(r, PROJ, OW - 1, OH)
    finally:
        ctx.clear_detection_masks()
    _same_regions(got, want)
    _same_regions(got_half, want_half)
    assert np.array_equal(got_half["parent"], got["parent"]) and not np.array_equal(got_half["desc"], got["desc"])
    _same_regions(ctx.reproject_regions_h(r, PROJ, OW, OH), plain)          # the mask is gone again


# ---- a whole view, the rematch, the command line
def _grey(fn):
    import orc
    from PIL import Image
    return orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB")))


VIEW_H = [1.08, 0.12, -14.0, -0.06, 0.92, 21.0, 2.5e-4, -1.5e-4, 1.0]


@pytest.mark.parametrize("do_blur", [0, 1])
def test_whole_view_equals_oracle_and_restatement(pkg, do_blur):
    """a 320 x 240 crop of graf1 under a moderate H: the restated warp (of the oracle's blur) through the oracle's plain-image
    detection and description, then the restated post-pass, is the list mods_detect_describe_view_h_dev leaves in slot 0"""
    import orc
    import torch
    img = np.ascontiguousarray(_grey(G1)[200:200 + OH, 240:240 + OW])
    geo = ref.view_geometry_h(OW, OH, VIEW_H, OW, OH, 0.8)
    pre = orc.gauss_blur_xy(img, geo["ksize"], geo["ksize"], geo["sigma"], geo["sigma"]) if do_blur else img
    view = ref.warp_perspective(pre, VIEW_H, geo["w_new"], geo["h_new"], cval=128.0)
    det, nd0 = orc.detect_describe(view)
    want = ref.reproject_regions_h(det, VIEW_H, OW, OH)
    assert 30 < len(want) < len(det)
    c = pkg.Context(0, OW, OH, 1)
    try:
        t = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        g, nd, nr = c.detect_describe_view_h_dev(t.data_ptr(), OW, OH, VIEW_H, OW, OH, init_sigma=0.8, do_blur=do_blur)
        assert (g.w_new, g.h_new) == (geo["w_new"], geo["h_new"])
        _same_pixels(c.view_pixels(g), view)
        got = c.regions_fetch(0)
        assert nd == nd0 and nr == len(want) == len(got)
        for f in ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "id", "parent", "desc"):
            assert got[f].tobytes() == want[f].tobytes(), f
        # the same call with a mask on slot 0: the list above filtered by its centres
        mask = detection_mask_ref.checkerboard(OW, OH)
        c.set_detection_mask(0, mask)
        _, _, nr_m = c.detect_describe_view_h_dev(t.data_ptr(), OW, OH, VIEW_H, OW, OH, init_sigma=0.8, do_blur=do_blur)
        c.clear_detection_masks()
        wm = detection_mask_ref.filter_regions(want, mask)
        gm = c.regions_fetch(0)
        assert 5 < len(wm) < len(want) - 5 and nr_m == len(wm)
        detection_mask_ref.assert_same_but_positions(gm, wm.astype(gm.dtype))
    finally:
        c.close()


def synthetic_pair():
    """(image 1 = a 400 x 300 crop of graf1, image 2 = its restated warp by H_true, H_true)"""
    a = np.ascontiguousarray(_grey(G1)[150:450, 200:600])
    H_true = [0.82, 0.21, 18.0, -0.17, 0.93, 42.0, 3.5e-4, 2.0e-4, 1.0]
    return a, ref.warp_perspective(a, H_true, a.shape[1], a.shape[0], cval=128.0), H_true


def _corner_error(H, H_true, w, h):
    c = np.array([[0.0, 0.0], [w, 0.0], [0.0, h], [w, h]])
    return float(np.hypot(*(ref.apply_h(H, c) - ref.apply_h(H_true, c)).T).max())


def _first_pass_and_rematch(pkg, a, b, seed, both):
    """the one-view ladder (tests/configs/iters_one_view.ini: TiltSet 1, ScaleSet 1, Phi 360, initSigma 0.2, FGINN 0.8, minMatches 15)
    and the rematch under its H, on one context; returns (first result, rematch result, its matches, regions added per bank)"""
    import torch
    h, w = a.shape
    d = pkg.view_ctx_dims(w, h)
    c = pkg.Context(0, d[0], d[1], 1)
    rep1, rep2 = pkg.ImgRep(c), pkg.ImgRep(c)
    try:
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        pkg.ransac_pin_seed(seed)
        first, _ = pkg.match_ladder_dev(c, t.data_ptr(), w, h, [pkg.LadderStep.make((1,), 360.0, init_sigma=0.2)], rep1, rep2, min_matches=15,
                                        max_matches=100000)
        n1, n2 = len(rep1), len(rep2)
        assert first.n_inliers > 0
        pkg.ransac_pin_seed(seed)
        again, m = pkg.rematch_under_h_dev(c, t.data_ptr(), w, h, t.data_ptr() + 4 * w * h, w, h, list(first.H), rep1, rep2, both=both,
                                           init_sigma=0.2, max_matches=100000)
        return first, again, m, (len(rep1) - n1, len(rep2) - n2)
    finally:
        pkg.ransac_pin_seed(-1)
        rep1.close(); rep2.close(); c.close()


def test_rematch_on_graf_finds_more(pkg, capsys):
    """graf1 / graf6: strictly more verified correspondences than the first pass, every row finite and inside both images.
    Measured on an MI355X (seed 4242): see profiles/view_h_timing.txt."""
    a, b = _grey(G1), _grey(G6)
    h, w = a.shape
    first, again, m, added = _first_pass_and_rematch(pkg, a, b, 4242, both=1)
    with capsys.disabled():
        print("\ngraf1/graf6 one view: %d tentatives, %d verified; rematch under its H: +%d | +%d regions, %d tentatives, %d verified"
              % (first.n_tentatives, first.n_inliers, added[0], added[1], again.n_tentatives, again.n_inliers))
    assert added[0] > 0 and added[1] > 0
    assert again.n_inliers > first.n_inliers
    assert len(m) == again.n_inliers and np.isfinite(m).all()
    assert (m[:, [0, 2]] > 0).all() and (m[:, [0, 2]] < w).all() and (m[:, [1, 3]] > 0).all() and (m[:, [1, 3]] < h).all()


def test_rematch_on_a_known_homography_is_no_worse(pkg, capsys):
    """image 2 = the restated warp of image 1 (a 400 x 300 crop of graf1) by H_true: the largest transfer error of the four image
    corners under the rematch's H does not exceed that under the first pass's H (both against H_true, within one run)."""
    a, b, H_true = synthetic_pair()
    h, w = a.shape
    first, again, m, added = _first_pass_and_rematch(pkg, a, b, 4242, both=0)
    e1, e2 = _corner_error(list(first.H), H_true, w, h), _corner_error(list(again.H), H_true, w, h)
    with capsys.disabled():
        print("\nsynthetic pair: first pass %d verified, corner error %.4f px; rematch +%d regions, %d verified, corner error %.4f px"
              % (first.n_inliers, e1, added[0], again.n_inliers, e2))
    assert added == (added[0], 0) and added[0] > 0
    assert again.n_inliers > 0 and e2 <= e1


def test_rematch_refuses_f_models(pkg, ctx):
    rep1, rep2 = pkg.ImgRep(ctx, 16), pkg.ImgRep(ctx, 16)
    try:
        par = pkg.PairParams.default()
        par.ransac.useF = 1
        with pytest.raises(pkg.ModsError, match="useF"):
            pkg.rematch_under_h_dev(ctx, 8, 64, 64, 8, 64, 64, np.eye(3), rep1, rep2, params=par)   # refused before the images are looked at
    finally:
        rep1.close(); rep2.close()


def _cli(tmp_path, name, config):
    out = tmp_path / name
    out.mkdir()
    env = dict(os.environ, MODS_RANSAC_SEED="4242")
    args = [MODS, G1, G6, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", config,
            os.path.join(CFG, "iters_one_view.ini")]
    p = subprocess.run(args, cwd=out, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    return out, p.stderr.decode() + p.stdout.decode()


def test_cli_rematch_under_h(tmp_path):
    """[Matching] rematchUnderH = 1 on graf changes the matches file and, under verbose, prints the regions added and the verified
    counts before and after; = 0 and the key absent write the same files"""
    ini = open(os.path.join(CFG, "classic.ini")).read()
    assert "[Matching]\n" in ini and "rematchUnderH" not in ini
    assert "verbose=1" in ini
    for v in ("0", "1"):
        (tmp_path / ("c%s.ini" % v)).write_text(ini.replace("[Matching]\n", "[Matching]\nrematchUnderH = %s\n" % v))
    off, text_off = _cli(tmp_path, "off", str(tmp_path / "c0.ini"))
    absent, text_absent = _cli(tmp_path, "absent", os.path.join(CFG, "classic.ini"))
    on, text_on = _cli(tmp_path, "on", str(tmp_path / "c1.ini"))
    for f in ("m.txt", "H.txt", "k1.txt", "k2.txt", "log.txt"):
        if f == "log.txt":       # (its first column is the run time)
            assert (off / f).read_text().split()[1:] == (absent / f).read_text().split()[1:]
        else:
            assert (off / f).read_bytes() == (absent / f).read_bytes(), f
    assert "Rematch under H" not in text_off and "Rematch under H" not in text_absent
    assert (on / "m.txt").read_bytes() != (off / "m.txt").read_bytes()
    line = [l for l in text_on.splitlines() if l.startswith("Rematch under H")]
    assert len(line) == 1, text_on
    words = line[0].replace(",", " ").replace(":", " ").split()
    nums = [int(x) for x in words if x.lstrip("+").isdigit()]
    added1, added2, before, after = nums[:4]
    assert added1 > 0 and added2 == 0 and before > 0
    assert after == len(np.loadtxt(on / "m.txt").reshape(-1, 4)) == int((on / "log.txt").read_text().split()[1])
    assert before == len(np.loadtxt(off / "m.txt").reshape(-1, 4))
