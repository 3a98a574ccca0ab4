"""Host tests of the homography views (include/mods_hip.h, "homography views"): mods_view_geometry_h against the restatement of
tests/view_h_ref.py, the arguments it refuses, and sanity of the restatement itself (what the GPU tests compare against)."""
import numpy as np
import pytest

import view_h_ref as ref

W, H = 320, 240
SIMILARITY = [0.9 * np.cos(0.2), -0.9 * np.sin(0.2), 31.5, 0.9 * np.sin(0.2), 0.9 * np.cos(0.2), 4.25, 0, 0, 1]
AFFINE = [1.1, 0.3, 7.0, -0.2, 0.8, 60.0, 0, 0, 1]
MILD = [1.02, 0.05, 3.0, -0.03, 0.97, 8.0, 1e-4, -5e-5, 1.0]
STRONG = [1.4, 0.2, 10.0, 0.1, 1.2, 5.0, 1.5e-3, 8e-4, 1.0]


@pytest.mark.parametrize("name,Hm", [("similarity", SIMILARITY), ("affine", AFFINE), ("mild", MILD), ("strong", STRONG)])
def test_view_geometry_h_equals_the_restatement(pkg, name, Hm):
    for w, h, cw, ch, sig in ((W, H, 4096, 4096, 0.2), (W, H, 200, 150, 0.8), (801, 333, 4096, 4096, 2.0)):
        g = pkg.view_geometry_h(w, h, Hm, cw, ch, sig)
        want = ref.view_geometry_h(w, h, Hm, cw, ch, sig)
        assert (g.w_new, g.h_new) == (want["w_new"], want["h_new"]), (name, w, h)
        assert g.w_new > 0 and g.h_new > 0
        assert (g.ksize_x, g.ksize_y) == (want["ksize"], want["ksize"])
        assert g.sigma_x == g.sigma_y == want["sigma"]
        assert list(g.H) == [float(v) for v in Hm]
        assert (g.identity, g.tilt, g.zoom, g.rotation) == (0, 1.0, 1.0, 0.0)
        assert (g.w_rot, g.h_rot) == (w, h)
    # the clip is what limits the second case
    assert pkg.view_geometry_h(W, H, AFFINE, 200, 150, 0.8).w_new == 200
    # initSigma / 4 = 0.5 -> floor(8 * 0.5 + 1) = 5; 0.2 / 4 -> floor(1.4) = 1 -> 3
    assert pkg.view_geometry_h(W, H, AFFINE, 4096, 4096, 2.0).ksize_x == 5 and pkg.view_geometry_h(W, H, AFFINE, 4096, 4096, 0.2).ksize_x == 3


def test_view_geometry_h_refuses(pkg):
    singular = [1, 2, 3, 2, 4, 6, 0, 0, 1]
    d0_zero = [1, 0, 0, 0, 1, 0, 2.0, 0, -(W - 1.0)]                       # H6 cx + H8 = 2 * 159.5 - 319 = 0 at the centre, exactly
    behind = [1, 0, 0, 0, 1, 0, -1.0 / 200.0, 0, 1.0]                      # the horizon x = 200 cuts the image: corners at x = 320 lie behind
    nan = [1, 0, 0, 0, 1, 0, 0, float("nan"), 1]
    inf = [1, 0, float("inf"), 0, 1, 0, 0, 0, 1]
    for bad in (singular, d0_zero, behind, nan, inf):
        with pytest.raises(pkg.ModsError):
            pkg.view_geometry_h(W, H, bad, 4096, 4096, 0.2)
        with pytest.raises(ValueError):
            ref.view_geometry_h(W, H, bad, 4096, 4096, 0.2)
    with pytest.raises(pkg.ModsError, match="horizon"):
        pkg.view_geometry_h(W, H, behind, 4096, 4096, 0.2)
    with pytest.raises(pkg.ModsError, match="singular"):
        pkg.view_geometry_h(W, H, singular, 4096, 4096, 0.2)


def _src(w=37, h=23, seed=5):
    return np.random.default_rng(seed).uniform(0, 255, (h, w)).astype(np.float32)


def test_restated_warp_identity_returns_the_source():
    s = _src()
    out = ref.warp_perspective(s, np.eye(3), s.shape[1], s.shape[0], cval=-7.0)
    assert np.array_equal(out.view(np.uint32), s.view(np.uint32))


def test_restated_warp_integer_translation():
    s = _src()
    h, w = s.shape
    T = [1, 0, 5, 0, 1, -3, 0, 0, 1]                  # view(x, y) = source(x - 5, y + 3)
    out = ref.warp_perspective(s, T, w, h, cval=-7.0)
    want = np.full((h, w), np.float32(-7.0))
    want[:h - 3, 5:] = s[3:, :w - 5]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_restated_warp_does_not_depend_on_the_sign_of_h():
    s = _src()
    a = ref.warp_perspective(s, STRONG, 70, 9)
    b = ref.warp_perspective(s, [-v for v in STRONG], 70, 9)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_lin_h_is_the_jacobian_of_the_projective_map():
    """central differences with step e = 1e-4: their truncation error is e^2 / 6 times a third derivative (about 1e-9 for these
    maps, whose derivatives are of order 1 and fall with powers of the denominator), their rounding error about 2^-52 |p| / e =
    2e-16 * 1e3 / 1e-4 = 2e-9; 1e-6 absolute leaves two orders of room and is far below a first-order disagreement (a wrong sign or
    a dropped term changes an entry by 1e-3 or more here)."""
    e = 1e-4
    for Hm in (MILD, STRONG):
        G, _ = ref.invert3_adjugate(Hm)
        Gm = G.reshape(3, 3)
        for x, y in ((10.0, 20.0), (300.0, 7.5), (160.25, 230.0)):
            L = np.array(ref.lin_h(np.float64(x), np.float64(y), G)).reshape(2, 2)
            p = lambda u, v: ref.apply_h(Gm, np.array([[u, v]]))[0]
            J = np.c_[(p(x + e, y) - p(x - e, y)) / (2 * e), (p(x, y + e) - p(x, y - e)) / (2 * e)]
            assert np.abs(L - J).max() < 1e-6, (Hm, x, y, L, J)
            assert np.abs(L - np.eye(2)).max() > 1e-3      # (not the identity: the comparison says something)


def test_restated_post_pass_on_the_identity(pkg):
    """H = I: the post-pass keeps a region iff its centre is strictly inside and its box clear of the border, and leaves it as it is"""
    regs = np.zeros(4, pkg.REGION_DTYPE)
    regs["x"] = [100.0, 0.0, 100.0, 3.0]
    regs["y"] = [100.0, 50.0, float(H), 3.0]
    regs["s"] = 1.0
    regs["a11"] = regs["a22"] = 2.0
    regs["id"] = np.arange(4)
    out = ref.reproject_regions_h(regs, np.eye(3), W, H)
    assert len(out) == 1 and out["x"][0] == 100.0 and out["a11"][0] == 2.0 and out["id"][0] == 0
