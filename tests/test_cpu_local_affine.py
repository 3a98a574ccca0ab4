"""The local affine consistency filter (mods_filter_local_affine, csrc/local_affine.hip) without a GPU: hand-computed cases of the
numpy restatement of its contract (tests/local_affine_ref.py), a usefulness check of the contract on a synthetic planar scene, and
the argument errors, which the library answers before any device call."""
import ctypes as C
import math

import numpy as np
import pytest

import local_affine_ref as lr

MODS_E_ARG = -2


def _diag(laf, **kw):
    d = lr.diagnostics(laf, kw)
    return d["neighbours"].tolist(), d["support"].tolist(), d["backed"].tolist(), d["keep"].astype(int).tolist()


def test_five_points():
    """Four tentatives on a square that move together and one in their middle that lands elsewhere: everybody has four neighbours,
    the four confirm each other (3 each, all strong, so backed = 3), nobody confirms the fifth and it confirms nobody."""
    _, _, laf = lr.five_points()
    assert _diag(laf, radius=20.0) == ([4] * 5, [3, 3, 3, 3, 0], [3, 3, 3, 3, 0], [1, 1, 1, 1, 0])


def test_equality_on_every_threshold():
    """x1 = (0,0), (3,4): r2 = 25 = R2 = D2; x2 = (50,50), (56,58): the offset (6,8) against the mapped (3,4) leaves the error (3,4),
    e2 = 25 = A2 with relTol 0; q2 = 100 >= D2."""
    _, _, laf = lr.two_points()
    assert _diag(laf, **lr.THRESHOLD)[:2] == ([1, 1], [1, 1])
    below = math.nextafter(5.0, 0.0)
    assert _diag(laf, **dict(lr.THRESHOLD, radius=below, minDist=below))[0] == [0, 0]
    d = _diag(laf, **dict(lr.THRESHOLD, absTol=below))
    assert d[0] == [1, 1] and d[1] == [0, 0]
    # minDist just above the distance: no neighbours either (r2 >= D2 fails)
    assert _diag(laf, **dict(lr.THRESHOLD, radius=6.0, minDist=math.nextafter(5.0, 6.0)))[0] == [0, 0]


def test_area_ratio_equality():
    """the same two points moving together, s2 = (1, 2): dT = (1, 4)"""
    _, _, laf = lr.two_points(((50, 50), (53, 54)), (1, 2))
    assert lr.frames(laf)[4].tolist() == [1.0, 4.0]
    base = dict(lr.THRESHOLD, absTol=100.0)
    assert _diag(laf, **dict(base, areaTol=4.0))[1] == [1, 1]
    assert _diag(laf, **dict(base, areaTol=3.9))[1] == [0, 0]
    assert _diag(laf, **dict(base, areaTol=0.0))[1] == [1, 1]


def test_singular_and_non_finite_frames():
    tent, u6, laf, bad = lr.degenerate_frames()
    assert lr.frames(laf)[5].tolist() == [True] * 5 + [False] * 3 + [True]
    with_area = lr.diagnostics(laf, dict(radius=20.0))
    # with the area test such a tentative neither supports nor is supported (the NaN position is nobody's neighbour at all)
    for i in bad:
        assert with_area["support"][i] == 0 and with_area["backed"][i] == 0, i
    assert with_area["neighbours"][8] == 0 and with_area["support"][:4].tolist() == [3, 3, 3, 3]
    no_area = lr.diagnostics(laf, dict(radius=20.0, areaTol=0.0))
    # without it the frames with finite positions are still confirmed by the four good ones, and still confirm nobody
    for i in bad[:3]:
        assert no_area["support"][i] == 0 and no_area["backed"][i] == 4, i
    assert no_area["backed"][8] == 0 and no_area["neighbours"][8] == 0
    assert no_area["support"][:4].tolist() == [6, 6, 6, 6]


def test_rescue_and_keep_sparse():
    _, _, laf = lr.rescue_scene()
    p = dict(radius=20.0, areaTol=0.0)
    both = lr.diagnostics(laf, p)
    assert both["support"].tolist() == [4, 4, 4, 4, 0, 0] and both["backed"].tolist() == [3, 3, 3, 3, 4, 0]
    assert both["neighbours"].tolist() == [4, 4, 4, 4, 4, 0]
    assert both["keep"].tolist() == [True] * 6
    assert lr.diagnostics(laf, dict(p, rescue=0))["keep"].tolist() == [True, True, True, True, False, True]
    assert lr.diagnostics(laf, dict(p, keepSparse=0))["keep"].tolist() == [True, True, True, True, True, False]
    assert lr.diagnostics(laf, dict(p, rescue=0, keepSparse=0))["keep"].tolist() == [True, True, True, True, False, False]


def test_filter_keeps_rows_and_order():
    tent, u6, laf = lr.five_points()
    t2, u2, l2, d = lr.filter_lists(tent, u6, laf, dict(radius=20.0))
    assert t2.tobytes() == tent[:4].tobytes() and u2.tobytes() == u6[:4].tobytes() and l2.tobytes() == laf[:4].tobytes()


def test_contract_is_useful_on_a_planar_scene():
    """1920 x 1080, 2000 tentatives, 20 % inliers under a homography with mild perspective, 3 % frame noise, 0.3 px position noise,
    uniform outliers; radius 100 and the other defaults.  Conditions, not measurements: at least 95 % of the kept are true and at
    least 90 % of the true are kept."""
    tent, u6, laf, is_true = lr.planar_scene(2000, 0.2, seed=1)
    keep = lr.diagnostics(laf, dict(radius=100.0))["keep"]
    kept, true_kept, n_true = int(keep.sum()), int((keep & is_true).sum()), int(is_true.sum())
    print("kept %d, true among them %d, true in the list %d" % (kept, true_kept, n_true))
    assert n_true == 400
    assert true_kept >= 0.95 * kept
    assert true_kept >= 0.90 * n_true


def _par(pkg, **kw):
    return pkg.LocalAffineParams.default(**kw)


BAD = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")),
       dict(minDist=-1.0), dict(minDist=float("nan")), dict(absTol=-0.5), dict(absTol=float("nan")),
       dict(relTol=-0.1), dict(relTol=float("nan")), dict(areaTol=-2.0), dict(areaTol=float("nan")),
       dict(minDist=161.0), dict(areaTol=0.5), dict(minSupport=0), dict(rescue=2), dict(rescue=-1), dict(keepSparse=2)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_argument_errors_need_no_device(pkg, bad):
    """every refusal is MODS_E_ARG with a text, from each entry point that takes the parameters, before the context, the pipeline or a
    device is looked at"""
    lib = pkg.lib()
    par = _par(pkg, **bad)
    tent, u6, laf = lr.five_points()
    n_out = C.c_int(-7)
    args = (tent.ctypes.data_as(C.c_void_p), u6.ctypes.data_as(C.c_void_p), laf.ctypes.data_as(C.c_void_p), len(tent), C.byref(par),
            C.byref(n_out), None, None, None, None)
    assert lib.mods_filter_local_affine(None, *args) == MODS_E_ARG
    assert lib.mods_last_error().decode().startswith("local_affine: " + next(iter(bad)))
    assert lib.mods_ctx_local_affine(None, C.byref(par)) == MODS_E_ARG
    assert lib.mods_last_error().decode().startswith("local_affine: " + next(iter(bad)))
    assert lib.mods_pipeline_local_affine(None, C.byref(par)) == MODS_E_ARG
    assert lib.mods_last_error().decode().startswith("local_affine: " + next(iter(bad)))


def test_null_pointers_and_negative_n(pkg):
    lib = pkg.lib()
    par = _par(pkg)
    tent, u6, laf = lr.five_points()
    n_out = C.c_int()
    ptrs = [tent.ctypes.data_as(C.c_void_p), u6.ctypes.data_as(C.c_void_p), laf.ctypes.data_as(C.c_void_p)]
    fake_ctx = None                      # no context exists without a device: a null one is itself one of the refusals
    assert lib.mods_filter_local_affine(fake_ctx, *ptrs, 5, C.byref(par), C.byref(n_out), None, None, None, None) == MODS_E_ARG
    assert "null" in lib.mods_last_error().decode()
    assert lib.mods_filter_local_affine(fake_ctx, *ptrs, 5, None, C.byref(n_out), None, None, None, None) == MODS_E_ARG
    assert "null parameters" in lib.mods_last_error().decode()
    assert lib.mods_filter_local_affine(fake_ctx, *ptrs, -1, C.byref(par), C.byref(n_out), None, None, None, None) == MODS_E_ARG
    assert "n = -1" in lib.mods_last_error().decode()
    assert lib.mods_ctx_local_affine(None, None) == MODS_E_ARG
    assert lib.mods_local_affine_counts(None, C.byref(n_out), C.byref(n_out)) == MODS_E_ARG
    assert lib.mods_pipeline_local_affine(None, None) == MODS_E_ARG
    with pytest.raises(pkg.ModsError, match="error -2"):
        pkg.filter_local_affine(None, tent, u6, laf, _par(pkg, radius=-3.0))


def test_defaults_and_grid(pkg):
    par = pkg.LocalAffineParams()
    pkg.lib().mods_local_affine_defaults.restype = None
    pkg.lib().mods_local_affine_defaults(C.byref(par))
    for k, v in lr.DEFAULTS.items():
        assert getattr(par, k) == v and getattr(_par(pkg), k) == v, k
    rows, tile = pkg.local_affine_grid()
    assert rows > 0 and tile > 0 and rows % 64 == 0 and tile % 64 == 0
