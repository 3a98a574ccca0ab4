"""-m gpu: the canvas and the tile rasteriser (csrc/draw.hip) against the numpy restatement of the contract (tests/draw_ref.py).
Every case compares whole canvases byte for byte, and n_dropped; canvases are at most 96 x 80 unless a case says otherwise."""
import os
import subprocess

import numpy as np
import pytest

import draw_ref as dr
import synth
from test_cpu_draw import F_TEST, H_TEST, synth_lafs

pytestmark = pytest.mark.gpu
SIZES = [(16, 16), (17, 33), (96, 80)]
RED, GREEN, BLUE, BLACK, GREY = 0xFF0000, 0x00FF00, 0x0000FF, 0x000000, 0x808080


def background(w, h, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def check(pkg, ctx, w, h, rows, want_dropped=0, what=""):
    """the list on a noise background through the library and through the restatement"""
    el = dr.elems(rows)
    base = background(w, h)
    cv = pkg.Canvas(ctx, w, h).blit(base)
    got_dropped = cv.draw(el)
    got = cv.fetch()
    cv.close()
    want = base.copy()
    ref_dropped = dr.draw(want, el)
    assert ref_dropped == want_dropped, (what, "the reference drops", ref_dropped)
    assert got_dropped == ref_dropped, (what, got_dropped, ref_dropped)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, "%d pixels differ, first (y, x) = %s" % (len(bad), bad[:4].tolist()))
    return got


def random_rows(rng, n, w, h, reach=24):
    """n elements of all kinds around the canvas, partly or wholly outside; groups repeat in runs"""
    rows, group = [], 0
    while len(rows) < n:
        kind = int(rng.integers(0, 3))
        ax, ay = int(rng.integers(-reach, w + reach)), int(rng.integers(-reach, h + reach))
        bx, by = ax + int(rng.integers(-30, 31)), ay + int(rng.integers(-30, 31))
        rgb = int(rng.integers(0, 1 << 24))
        if kind == dr.DISC:
            rows.append(dr.disc(ax, ay, int(rng.integers(0, 9)), rgb))
        elif kind == dr.LINE:
            rows.append(dr.line(ax, ay, bx, by, rgb))
        else:
            t = int(rng.integers(0, 7))
            for _ in range(int(rng.integers(1, 4))):                 # a short polyline
                rows.append(dr.seg(ax, ay, bx, by, t, rgb, group))
                ax, ay, bx, by = bx, by, bx + int(rng.integers(-20, 21)), by + int(rng.integers(-20, 21))
            group += int(rng.integers(0, 2))                          # the next run may carry the same id
    return rows[:n]


def test_canvas_fill_blit_fetch(pkg, gpu_ctx):
    import torch
    w, h = 37, 29
    cv = pkg.Canvas(gpu_ctx, w, h).fill(0x123456)
    want = np.zeros((h, w, 3), np.uint8)
    want[:] = (0x12, 0x34, 0x56)
    assert cv.size == (w, h) and np.array_equal(cv.fetch(), want)
    rng = np.random.default_rng(3)
    grey = rng.integers(0, 256, (10, 20), dtype=np.uint8)
    rgb = rng.integers(0, 256, (33, 12, 3), dtype=np.uint8)
    for img, x0, y0 in ((grey, 3, 4), (rgb, 30, -2), (grey, -5, 25), (rgb, -20, -40), (grey, w, 0)):
        cv.blit(img, x0, y0)
        dr.blit(want, img, x0, y0)
        assert np.array_equal(cv.fetch(), want), (x0, y0)
    f = rng.uniform(-40, 300, (9, 14)).astype(np.float32)
    f[0, :6] = [np.nan, -0.0, 0.5, 1.5, 254.5, 255.49]
    f[1, :4] = [np.inf, -np.inf, 2.5, 300.0]
    padded = np.zeros((9, 16), np.float32)
    padded[:, :14] = f
    t = torch.from_numpy(padded).cuda(0)
    torch.cuda.synchronize()
    cv.blit_f32_dev(t.data_ptr(), 14, 9, stride=16, x0=30, y0=22)
    dr.blit(want, dr.f32_to_u8(f), 30, 22)
    assert np.array_equal(cv.fetch(), want)
    other = pkg.Canvas(gpu_ctx, 8, 8).fill(0xFFFFFF)
    other.blit_canvas(cv, -10, -10)
    assert np.array_equal(other.fetch(), want[10:18, 10:18])
    other.close()
    cv.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_empty_list(pkg, gpu_ctx, w, h):
    check(pkg, gpu_ctx, w, h, [])


@pytest.mark.parametrize("w,h", SIZES)
def test_edges_and_degenerate_elements(pkg, gpu_ctx, w, h):
    rows = [dr.disc(-40, -40, 6, RED), dr.seg(-60, -5, -30, -9, 4, RED, 0), dr.line(-3, h + 5, w + 3, h + 9, RED),    # wholly outside
            dr.disc(0, 0, 5, GREEN), dr.disc(w - 1, h - 1, 4, BLUE), dr.seg(-8, 3, 9, 6, 5, BLACK, 1),               # partly outside
            dr.line(-10, -4, w + 10, h + 2, GREY), dr.line(w + 4, 2, -6, h - 3, RED),
            dr.disc(15, 15, 0, RED), dr.disc(16, 16, 0, GREEN), dr.disc(15, 16, 0, BLUE), dr.disc(16, 15, 0, BLACK),   # tile corners, r = 0
            dr.disc(16, 16, 3, GREY), dr.seg(12, 12, 20, 20, 3, RED, 2), dr.seg(20, 12, 12, 20, 2, BLUE, 3),         # four tiles
            dr.line(14, 17, 18, 13, GREEN),
            dr.seg(7, 9, 7, 9, 4, GREEN, 4), dr.seg(3, 12, 3, 12, 0, RED, 5), dr.line(9, 3, 9, 3, BLACK),             # zero length
            dr.seg(1, 1, 14, 1, 0, BLUE, 6), dr.seg(2, 14, 13, 10, 1, BLACK, 7)]
    check(pkg, gpu_ctx, w, h, rows)
    check(pkg, gpu_ctx, w, h, random_rows(np.random.default_rng(w), 120, w, h), what="random")


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_chunk_tails_one_tile(pkg, gpu_ctx, n):
    """n elements that all hit the one tile of a 16 x 16 canvas, and the first tile of a 17 x 33 one"""
    rng = np.random.default_rng(n)
    for w, h in ((16, 16), (17, 33)):
        rows = random_rows(rng, n, 16, 16, reach=0)
        assert len(rows) == n
        check(pkg, gpu_ctx, w, h, rows, what="%d elements" % n)


@pytest.mark.parametrize("lead", [236, 246, 255, 256])
def test_polyline_across_chunk_boundary(pkg, gpu_ctx, lead):
    """a 21-segment polyline whose hits straddle (or touch) the 256-entry boundary of the tile's hit list; in the second canvas every
    other element in front of it is culled from the tile under test, so list place and hit place differ"""
    ring = [(8 + int(round(6 * np.cos(k * np.pi / 10))), 8 + int(round(6 * np.sin(k * np.pi / 10)))) for k in range(22)]
    poly = [dr.seg(ring[k][0], ring[k][1], ring[k + 1][0], ring[k + 1][1], 3, BLUE, 9) for k in range(21)]
    rng = np.random.default_rng(lead)
    head = [dr.disc(int(rng.integers(0, 16)), int(rng.integers(0, 16)), 1, int(rng.integers(0, 1 << 24))) for _ in range(lead)]
    tail = [dr.line(0, 3, 15, 12, RED), dr.seg(0, 8, 15, 8, 1, GREEN, 9)]
    check(pkg, gpu_ctx, 16, 16, head + poly + tail, what="lead %d" % lead)
    far = [dr.disc(70, 60, 2, GREY)] * lead
    mixed = [e for pair in zip(head, far) for e in pair]
    check(pkg, gpu_ctx, 96, 80, mixed + poly + tail, what="lead %d, culled elements between" % lead)


def test_order_dependence(pkg, gpu_ctx):
    a, b, c = dr.disc(20, 20, 7, RED), dr.seg(10, 20, 30, 22, 5, BLUE, 0), dr.line(8, 14, 33, 27, GREEN)
    one = check(pkg, gpu_ctx, 40, 40, [a, b, c])
    two = check(pkg, gpu_ctx, 40, 40, [c, b, a])
    assert (one != two).any()


def test_adjacent_groups(pkg, gpu_ctx):
    s1, s2 = (4, 10, 14, 10), (14, 10, 20, 18)
    same = check(pkg, gpu_ctx, 28, 28, [dr.seg(*s1, 3, BLACK, 7), dr.seg(*s2, 3, BLACK, 7)])
    diff = check(pkg, gpu_ctx, 28, 28, [dr.seg(*s1, 3, BLACK, 7), dr.seg(*s2, 3, BLACK, 8)])
    assert (same != diff).any()
    # one id, but an element between the two (culled from their tiles), or two colours: two polylines
    check(pkg, gpu_ctx, 96, 80, [dr.seg(*s1, 3, BLACK, 7), dr.disc(80, 70, 2, RED), dr.seg(*s2, 3, BLACK, 7)])
    merged = check(pkg, gpu_ctx, 96, 80, [dr.seg(*s1, 3, BLACK, 7), dr.seg(*s2, 3, BLACK, 7), dr.disc(80, 70, 2, RED)])
    split = check(pkg, gpu_ctx, 96, 80, [dr.seg(*s1, 3, BLACK, 7), dr.disc(80, 70, 2, RED), dr.seg(*s2, 3, BLACK, 7)])
    assert (merged != split).any()
    check(pkg, gpu_ctx, 28, 28, [dr.seg(*s1, 3, BLACK, 7), dr.seg(*s2, 3, GREY, 7)])


def test_dropped_elements_are_counted(pkg, gpu_ctx):
    rows = [dr.disc(10, 10, 3, RED), dr.disc(32768, 5, 2, RED),
            dr.seg(2, 2, 8, 2, 2, BLACK, 1), dr.seg(8, 2, 8 + 2048, 9, 2, BLACK, 1), dr.seg(8, 9, 3, 9, 2, BLACK, 1),
            dr.seg(20, 20, 30, 25, 2, BLUE, 2), dr.line(0, 0, 12, 31, GREEN)]
    check(pkg, gpu_ctx, 40, 36, rows, want_dropped=4)


def bank_regions(pkg, n, w, h, seed=9):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, pkg.REGION_DTYPE)
    r["x"], r["y"] = rng.uniform(-15, w + 15, n), rng.uniform(-15, h + 15, n)
    r["s"] = np.exp(rng.uniform(np.log(0.5), np.log(40.0), n))
    ang, st = rng.uniform(0, 2 * np.pi, n), rng.uniform(1.0, 4.0, n)
    r["a11"], r["a12"], r["a21"], r["a22"] = np.cos(ang) * st, -np.sin(ang) / st, np.sin(ang) * st, np.cos(ang) / st
    r["id"] = np.arange(n)
    return r


@pytest.mark.parametrize("table,thickness", [(dr.TABLE_REGIONS, 2), (dr.TABLE_MATCHES, 1)])
def test_draw_regions(pkg, gpu_ctx, table, thickness):
    w, h, dx, dy = 96, 80, 5, -3
    reg = bank_regions(pkg, 300, w, h)
    rep = pkg.ImgRep(gpu_ctx, 1024)
    rep.append_host(reg)
    base = background(w, h, seed=4)
    cv = pkg.Canvas(gpu_ctx, w, h).blit(base)
    # a slice of the bank, so that `begin` counts
    begin, count = 7, 290
    got_el, got_dropped = cv.regions_elems(rep, begin, count, dx, dy, thickness, dr.COLOUR_REGIONS, table)
    want_el, want_dropped = dr.regions_elems(reg[begin:begin + count], dx, dy, thickness, dr.COLOUR_REGIONS, table)
    assert want_dropped == 0 and got_dropped == 0
    for f in dr.ELEM.names:
        assert np.array_equal(got_el[f], want_el[f]), f
    assert np.array_equal(cv.fetch(), base)                              # the list alone draws nothing
    assert cv.draw_regions(rep, begin, count, dx, dy, thickness, dr.COLOUR_REGIONS, table) == 0
    got = cv.fetch()
    host = pkg.Canvas(gpu_ctx, w, h).blit(base)
    assert host.draw(want_el) == 0
    assert np.array_equal(got, host.fetch()), "device-built contours differ from the host list drawn"
    want = base.copy()
    assert dr.draw(want, want_el) == 0
    assert np.array_equal(got, want)
    assert (got != base).any()
    for c in (cv, host):
        c.close()
    rep.close()


def test_draw_regions_drops_whole_contours(pkg, gpu_ctx):
    w, h = 48, 40
    reg = bank_regions(pkg, 6, w, h, seed=2)
    reg["s"][1] = 1e6                      # points beyond the coordinate range
    reg["x"][3] = np.nan
    reg["s"][4] = 300.0                    # far larger than the canvas, yet within both limits: drawn
    rep = pkg.ImgRep(gpu_ctx, 64)
    rep.append_host(reg)
    want_el, want_dropped = dr.regions_elems(reg, 0, 0, 2, dr.COLOUR_REGIONS, dr.TABLE_REGIONS)
    assert want_dropped == 42
    cv = pkg.Canvas(gpu_ctx, w, h).fill(0xFFFFFF)
    got_el, got_dropped = cv.regions_elems(rep, 0, 6, 0, 0, 2, dr.COLOUR_REGIONS, dr.TABLE_REGIONS)
    assert got_dropped == want_dropped
    for f in dr.ELEM.names:
        assert np.array_equal(got_el[f], want_el[f]), f
    assert cv.draw_regions(rep, 0, 6, 0, 0, 2) == want_dropped
    want = dr.white(w, h)
    dr.draw(want, want_el)
    assert np.array_equal(cv.fetch(), want)
    cv.close()
    rep.close()


def h_with_pole(x):
    """a homography whose third coordinate vanishes on the line of abscissa x (a power of two: the products are exact)"""
    return np.array([[1.0, 0.0, 2.0], [0.0, 1.0, -1.0], [-1.0 / x, 0.0, 1.0]])


MATCH_CASES = [("side by side", dict(), H_TEST), ("centres only", dict(centers_only=1), H_TEST),
               ("reprojected", dict(reproject=1), H_TEST), ("reprojected, centres only", dict(reproject=1, centers_only=1), H_TEST),
               ("reprojected, a centre on the pole", dict(reproject=1), h_with_pole(32.0)),
               ("epipolar lines", dict(epipolar=1), F_TEST),
               ("epipolar lines, vertical", dict(epipolar=1), np.array([[0., 0., 1.], [0., 0., 0.], [-1., 0., 0.]])),
               ("epipolar lines, out of frame", dict(epipolar=1, r1=3, r2=2), np.array([[0., 0., 0.], [0., 0., 1.], [0., -1., -500.]]))]


@pytest.mark.parametrize("what,kw,M", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_draw_matches(pkg, gpu_ctx, what, kw, M):
    rng = np.random.default_rng(8)
    img1 = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)             # colour
    img2 = rng.integers(0, 256, (56, 80), dtype=np.uint8)                # grey
    laf = synth_lafs(40, 64, 48, 80, 56)
    laf[5, 0:2] = (32.0, 20.0)                                           # on the pole of h_with_pole(32)
    s1, s2 = pkg.Canvas(gpu_ctx, 64, 48).blit(img1), pkg.Canvas(gpu_ctx, 80, 56).blit(img2)
    o1, o2, dropped = pkg.draw_matches(gpu_ctx, s1, s2, laf, pkg.DrawMatchesParams.default(M, **kw))
    w1, w2, wd = dr.draw_matches(img1, img2, laf, M, **kw)
    assert dropped == wd, (dropped, wd)
    if "pole" in what or "vertical" in what:
        assert sum(wd) > 0
    g1, g2 = o1.fetch(), o2.fetch()
    assert g1.shape == w1.shape and g2.shape == w2.shape
    if not kw.get("reproject"):
        assert g1.shape == (56, 64 + 80 + 20, 3) and g2.shape == (48 + 56 + 20, 80, 3)
    assert np.array_equal(g1, w1) and np.array_equal(g2, w2)
    for c in (s1, s2, o1, o2):
        c.close()


def test_verified_lafs_of_a_pair(pkg, gpu_ctx):
    import torch
    w, h = 320, 240
    a, b, _ = synth.pair(w, h, seed=7)
    t = torch.from_numpy(np.stack([a, b])).cuda(0)
    torch.cuda.synchronize()
    pkg.ransac_pin_seed(11)
    res, matches = pkg.match_pair_dev(gpu_ctx, t.data_ptr(), w, h, max_matches=10000)
    laf = gpu_ctx.verified_lafs()
    assert res.n_inliers >= 15 and len(laf) == res.n_inliers == len(matches)
    assert np.array_equal(laf[:, (0, 1, 7, 8)], matches)
    assert (laf[:, 6] > 0).all() and (laf[:, 13] > 0).all()


def test_verified_lafs_of_a_ladder_and_of_several_devices(pkg):
    """the one-GPU ladder and mods_match_ladder_multi (device 0 listed twice: the sharded path on one GPU) keep the same frames"""
    import torch
    w, h = 320, 240
    a, b, _ = synth.pair(w, h, seed=7)
    steps = [pkg.LadderStep.make((1,), 360.0)]
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 16), pkg.ImgRep(ctx, 1 << 16)
    t = torch.from_numpy(np.stack([a, b])).cuda(0)
    torch.cuda.synchronize()
    pkg.ransac_pin_seed(31)
    res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, rep1, rep2, max_matches=100000)
    laf = ctx.verified_lafs()
    assert res.n_inliers >= 15 and len(laf) == res.n_inliers and np.array_equal(laf[:, (0, 1, 7, 8)], m)
    multi = pkg.Multi([0, 0], w, h, rep_capacity=1 << 16)
    assert len(multi.verified_lafs()) == 0
    pkg.ransac_pin_seed(31)
    got, gm = multi.match_ladder(a, b, steps, max_matches=100000)
    pkg.ransac_pin_seed(-1)
    assert np.array_equal(gm, m) and np.array_equal(multi.verified_lafs(), laf)
    multi.close()
    rep1.close(); rep2.close(); ctx.close()


# ---- the command line ----------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))


def _cli(tmp_path, name, image_output):
    """one run of iters_one_view.ini on the golden pair in tmp_path/name with the [ImageOutput] section given (None: none);
    returns the directory"""
    d = tmp_path / name
    d.mkdir()
    cfg = open(os.path.join(CFG, "classic.ini")).read()
    assert "[ImageOutput]" not in cfg
    if image_output is not None:
        cfg += "\n[ImageOutput]\n" + image_output
    (d / "config.ini").write_text(cfg)
    env = dict(os.environ, MODS_RANSAC_SEED="4242", MODS_DRAW_FRAMES="frames.txt")
    args = [MODS, G1, G6, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", "config.ini",
            os.path.join(CFG, "iters_one_view.ini")]
    p = subprocess.run(args, cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    return d


def _png(fn):
    from PIL import Image
    return np.asarray(Image.open(fn).convert("RGB"))


def _frames(d):
    rows = (d / "frames.txt").read_text().splitlines()
    M = np.array(rows[0].split(), np.float64)
    laf = np.array([r.split() for r in rows[1:]], np.float64).reshape(-1, 14)
    return M, laf


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("draw_cli")
    return {"plain": _cli(tmp, "plain", None),
            "default": _cli(tmp, "default", "writeImages = 1\n"),
            "full": _cli(tmp, "full", "writeImages = 1\ndrawReprojected = 0\ndrawOnlyCenters = 0\ndrawDetectedRegions = 1\n")}


def test_cli_without_the_section_is_unchanged(cli_runs):
    plain, full = cli_runs["plain"], cli_runs["full"]
    assert sorted(f for f in os.listdir(plain) if f.endswith(".png")) == [] and not (plain / "frames.txt").exists()
    assert (plain / "m.txt").read_bytes() == (full / "m.txt").read_bytes() and len((plain / "m.txt").read_bytes()) > 100
    assert (plain / "log.txt").read_text().split()[1:] == (full / "log.txt").read_text().split()[1:]      # field 0 is the run time
    for k in ("k1.txt", "k2.txt"):
        assert (plain / k).read_bytes() == (full / k).read_bytes()


def test_cli_match_images_side_by_side(cli_runs):
    d = cli_runs["full"]
    s1, s2 = _png(G1), _png(G6)
    (h1, w1), (h2, w2) = s1.shape[:2], s2.shape[:2]
    M, laf = _frames(d)
    m = np.loadtxt(d / "m.txt").reshape(-1, 4)
    assert len(laf) == len(m) > 15 and np.allclose(laf[:, (0, 1, 7, 8)], m, rtol=1e-5, atol=1e-3)
    o1, o2 = _png(d / "o1.png"), _png(d / "o2.png")
    assert o1.shape == (max(h1, h2), w1 + w2 + 20, 3) and o2.shape == (h1 + h2 + 20, max(w1, w2), 3)
    plain = dr.white(w1 + w2 + 20, max(h1, h2))
    dr.blit(plain, s1, 0, 0)
    dr.blit(plain, s2, w1 + 20, 0)
    assert (o1 != plain).any()
    want = plain.copy()
    assert dr.draw(want, dr.matches_elems(0, w1, h1, w2, h2, laf, M, centers_only=0, reproject=0, r1=5, r2=4)) == 0
    assert np.array_equal(o1, want)
    # the region images: sources under contours, and the matches over them
    for fn, shape, src in (("o1.png_reg.png", s1.shape, s1), ("o2.png_reg.png", s2.shape, s2)):
        img = _png(d / fn)
        assert img.shape == shape and (img != src).any()
    r1, r2 = _png(d / "o1.png.png"), _png(d / "o2.png.png")
    assert r1.shape == o1.shape and r2.shape == o2.shape and (r1 != o1).any() and (r2 != o2).any()


def test_cli_match_images_default_keys(cli_runs):
    """writeImages = 1 alone: the reference's defaults - centres only, reprojected through the verified H"""
    d = cli_runs["default"]
    s1, s2 = _png(G1), _png(G6)
    M, laf = _frames(d)
    assert sorted(f for f in os.listdir(d) if f.endswith(".png")) == ["o1.png", "o2.png"]
    w1, w2, dropped = dr.draw_matches(s1, s2, laf, M, centers_only=1, reproject=1, r1=5, r2=4)
    o1, o2 = _png(d / "o1.png"), _png(d / "o2.png")
    assert o1.shape == s1.shape and o2.shape == s2.shape and (o1 != s1).any() and (o2 != s2).any()
    assert np.array_equal(o1, w1) and np.array_equal(o2, w2)
