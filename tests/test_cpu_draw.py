"""The numpy restatement of the drawing contract (tests/draw_ref.py) against cases worked out by hand, and the host half of the
library - the composition of DrawMatches' element lists (mods_draw_matches_elems, no device needed) - against the restatement."""
import numpy as np
import pytest

import draw_ref as dr

BLACK = 0x000000


def synth_lafs(n, w1, h1, w2, h2, seed=5):
    """n frames pairs: centres inside the images (a few outside), anisotropic shapes, s from 0.5 to 8"""
    rng = np.random.default_rng(seed)
    laf = np.zeros((n, 14))
    for half, (w, h) in enumerate(((w1, h1), (w2, h2))):
        o = 7 * half
        laf[:, o] = rng.uniform(-6, w + 6, n)
        laf[:, o + 1] = rng.uniform(-6, h + 6, n)
        ang = rng.uniform(0, 2 * np.pi, n)
        st = rng.uniform(1.0, 3.0, n)
        laf[:, o + 2] = np.cos(ang) * st
        laf[:, o + 3] = -np.sin(ang) / st
        laf[:, o + 4] = np.sin(ang) * st
        laf[:, o + 5] = np.cos(ang) / st
        laf[:, o + 6] = rng.uniform(0.5, 8.0, n)
    return laf


H_TEST = np.array([[0.95, 0.08, 3.0], [-0.05, 1.02, -2.0], [2e-4, -1e-4, 1.0]])
F_TEST = np.array([[1e-6, 2e-5, -3e-3], [-1.5e-5, 2e-6, 8e-3], [2e-3, -9e-3, 0.3]])


@pytest.mark.parametrize("r,count", [(2, 13), (4, 49), (7, 149), (30, 2821)])
def test_disc_pixel_counts(r, count):
    cv = dr.white(80, 80)
    assert dr.draw(cv, dr.elems([dr.disc(40, 40, r, BLACK)])) == 0
    assert int((cv[:, :, 0] == 0).sum()) == count


def test_horizontal_segment_coverage():
    cv = dr.white(16, 12)
    assert dr.draw(cv, dr.elems([dr.seg(2, 5, 10, 5, 2, BLACK, 0)])) == 0
    assert (cv[5, 2:11] == 0).all()
    assert (cv[4, 2:11] == 128).all() and (cv[6, 2:11] == 128).all()
    assert (cv[3] == 255).all() and (cv[7] == 255).all()
    masks = dr.seg_masks(dr.elems([dr.seg(2, 5, 10, 5, 2, BLACK, 0)])[0], 2, 10, 4, 6)
    pop = np.array([[bin(int(v)).count("1") for v in row] for row in masks])
    assert (pop[1] == 16).all() and (pop[0] == 8).all() and (pop[2] == 8).all()


@pytest.mark.parametrize("a,b", [((3, 4), (40, 17)), ((3, 4), (9, 60)), ((50, 2), (7, 31)), ((5, 5), (25, 25)), ((5, 25), (25, 5)),
                                 ((8, 8), (8, 8)), ((0, 0), (11, 0)), ((4, 30), (4, 2)), ((0, 0), (7, 3)), ((0, 3), (7, 0))])
def test_line_rule(a, b):
    fwd, back = dr.line_pixels(*a, *b), dr.line_pixels(*b, *a)
    assert set(fwd) == set(back)
    assert len(fwd) == len(set(fwd)) == max(abs(b[0] - a[0]), abs(b[1] - a[1])) + 1
    assert a in fwd and b in fwd
    if abs(b[0] - a[0]) == abs(b[1] - a[1]) and a != b:
        sx, sy = np.sign(b[0] - a[0]), np.sign(b[1] - a[1])
        assert set(fwd) == {(a[0] + sx * k, a[1] + sy * k) for k in range(abs(b[0] - a[0]) + 1)}
    for (x0, y0), (x1, y1) in zip(fwd, fwd[1:]):                            # 8-connected
        assert max(abs(x1 - x0), abs(y1 - y0)) == 1


def test_polyline_joint_is_blended_once():
    a, b = dr.seg(4, 10, 14, 10, 3, BLACK, 7), dr.seg(14, 10, 20, 18, 3, BLACK, 7)
    joined = dr.white(28, 28)
    dr.draw(joined, dr.elems([a, b]))
    # the union rule by hand: OR of the two capsules' subsample masks, one blend
    e = dr.elems([a, b])
    mask = dr.seg_masks(e[0], 0, 27, 0, 27) | dr.seg_masks(e[1], 0, 27, 0, 27)
    c = np.array([[bin(int(v)).count("1") for v in row] for row in mask])
    want = ((255 * (16 - c) + 8) >> 4).astype(np.uint8)
    assert np.array_equal(joined[:, :, 0], want) and np.array_equal(joined[:, :, 1], want)
    apart = dr.white(28, 28)
    dr.draw(apart, dr.elems([a, b[:7] + (8,)]))
    assert (apart != joined).any()
    assert (apart.astype(int) <= joined.astype(int)).all()                   # blending twice only darkens


def test_drop_rule():
    cv = dr.white(32, 32)
    el = dr.elems([dr.disc(40000, 3, 2, BLACK), dr.seg(2, 2, 8, 2, 1, BLACK, 1), dr.seg(8, 2, 8 + 2048, 9, 1, BLACK, 1),
                   dr.seg(8, 9, 3, 9, 1, BLACK, 1), dr.line(0, 0, 5, -32768, BLACK), dr.disc(5, 20, 1, BLACK)])
    assert dr.draw(cv, el) == 5
    want = dr.white(32, 32)
    dr.draw(want, dr.elems([dr.disc(5, 20, 1, BLACK)]))
    assert np.array_equal(cv, want)


def test_order_matters():
    a, b = dr.disc(10, 10, 5, 0xFF0000), dr.seg(4, 10, 16, 10, 3, 0x0000FF, 0)
    one, two = dr.white(24, 24), dr.white(24, 24)
    dr.draw(one, dr.elems([a, b]))
    dr.draw(two, dr.elems([b, a]))
    assert (one != two).any() and tuple(two[10, 10]) == (255, 0, 0) and tuple(one[10, 10]) == (0, 0, 255)


def _cases():
    return [dict(), dict(centers_only=1), dict(reproject=1), dict(reproject=1, centers_only=1), dict(epipolar=1), dict(r1=3, r2=2)]


@pytest.mark.parametrize("kw", _cases())
@pytest.mark.parametrize("which", [0, 1])
def test_matches_elems_host(pkg, kw, which):
    """the library's composition of the element lists equals the restatement's, element by element"""
    w1, h1, w2, h2 = 64, 48, 80, 56
    laf = synth_lafs(40, w1, h1, w2, h2)
    M = F_TEST if kw.get("epipolar") else H_TEST
    par = pkg.DrawMatchesParams.default(M, **kw)
    got = pkg.draw_matches_elems(which, w1, h1, w2, h2, laf, par)
    want = dr.matches_elems(which, w1, h1, w2, h2, laf, M, **kw)
    assert len(got) == len(want) and len(got) >= 40 * 3
    for f in dr.ELEM.names:
        assert np.array_equal(got[f], want[f]), f


def test_matches_elems_epipolar_edge_lines(pkg):
    """an epipolar line that is vertical (l_1 = 0: b is infinite, the LINE is emitted unclipped for the draw call to drop) and one
    that misses the frame (no element)"""
    w1, h1, w2, h2 = 64, 48, 80, 56
    laf = synth_lafs(3, w1, h1, w2, h2, seed=2)
    laf[:, 0:2] = [[10, 10], [20, 20], [30, 30]]
    laf[:, 7:9] = [[10, 10], [20, 20], [30, 30]]
    F = np.array([[0., 0., 1.], [0., 0., 0.], [-1., 0., 0.]])        # l = (1, 0, -px) for the second image's point: the line x = px
    for which in (0, 1):
        got = pkg.draw_matches_elems(which, w1, h1, w2, h2, laf, pkg.DrawMatchesParams.default(F, epipolar=1))
        want = dr.matches_elems(which, w1, h1, w2, h2, laf, F, epipolar=1)
        assert len(got) == len(want)
        for f in dr.ELEM.names:
            assert np.array_equal(got[f], want[f]), f
        assert (np.abs(want["by"][want["kind"] == dr.LINE]) > dr.COORD_MAX).any()
    F2 = np.array([[0., 0., 0.], [0., 0., 1.], [0., -1., -500.]])    # y = const far below the frame
    got = pkg.draw_matches_elems(0, w1, h1, w2, h2, laf, pkg.DrawMatchesParams.default(F2, epipolar=1))
    want = dr.matches_elems(0, w1, h1, w2, h2, laf, F2, epipolar=1)
    assert len(got) == len(want)
    for f in dr.ELEM.names:
        assert np.array_equal(got[f], want[f]), f
