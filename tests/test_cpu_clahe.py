"""CLAHE ([Matching] doCLAHE, csrc/clahe.hip): worked cases of the numpy restatement (tests/clahe_ref.py), and the argument checks
of mods_clahe_dev / mods_clahe, which run before any device call (ctx = NULL: no GPU needed, each check has its own message)."""
import ctypes as C

import numpy as np
import pytest

import clahe_ref


def test_constant_image_maps_to_108():
    # 64 x 64 at 8 x 8 tiles: 64-pixel tiles, clip max(int(4 * 64 / 256), 1) = 1; 63 clipped counts spread as 0 per bin plus a
    # residual of 63 at step 4 (bins 0, 4, ..., 248); the cumulative count at 100 is 26 + 1 = 27 -> rint(27 * 255 / 64) = 108
    img = np.full((64, 64), 100, np.uint8)
    assert clahe_ref.clip_count(4.0, 64) == 1
    lut = clahe_ref.luts(img)
    assert lut.shape == (64, 256) and np.all(lut[:, 100] == 108)
    assert np.all(clahe_ref.clahe(img) == 108)


@pytest.mark.parametrize("clip", [4.0, 40.0, 1.5, 0.0])
def test_one_tile_grid_is_global_equalisation(clip):
    """with a 1 x 1 grid both interpolation weights only ever meet the same LUT: the output is lut[v] exactly"""
    img = np.random.default_rng(3).integers(0, 256, (37, 53), dtype=np.uint8)
    img[:10] = 17                                            # a peak that the clip limit cuts
    lut = clahe_ref.luts(img, clip, (1, 1))[0]
    assert np.array_equal(clahe_ref.clahe(img, clip, (1, 1)), lut[img])


@pytest.mark.parametrize("clip", [0.0, -1.0])
def test_clip_at_or_below_zero_does_not_clip(clip):
    img = np.random.default_rng(5).integers(0, 256, (40, 48), dtype=np.uint8)
    img[:20] = 200
    assert clahe_ref.clip_count(clip, 40 * 48) == 0
    h = np.bincount(img.ravel(), minlength=256)
    want = np.clip(np.rint(np.cumsum(h).astype(np.float32) * (np.float32(255) / np.float32(img.size))), 0, 255).astype(np.uint8)
    assert np.array_equal(clahe_ref.luts(img, clip, (1, 1))[0], want)
    assert not np.array_equal(clahe_ref.luts(img, 4.0, (1, 1))[0], want)     # the peak at 200 is clipped with a positive limit


def test_padding_quirk():
    """w % 8 == 0 but h % 8 != 0: both dimensions grow by a whole pad, 1000 x 777 -> 1008 x 784, tiles of 126 x 98"""
    assert clahe_ref.tile_size(1000, 777, 8, 8) == (126, 98)
    assert clahe_ref.tile_size(1000, 776, 8, 8) == (125, 97)
    assert clahe_ref.tile_size(5, 3, 16, 9) == (1, 1)
    assert list(clahe_ref.reflect101(np.arange(5, 12), 5)) == [3, 2, 1, 0, 1, 2, 3]      # reflected again past the first pixel
    assert list(clahe_ref.reflect101(np.arange(0, 4), 1)) == [0, 0, 0, 0]
    img = np.random.default_rng(7).integers(0, 256, (777, 1000), dtype=np.uint8)
    lut = clahe_ref.luts(img, 0.0)                                                          # no clip: lut[255] = 255 in every tile
    assert lut.shape == (64, 256) and np.all(lut[:, 255] == 255)
    # a bottom tile counts the 7 reflected rows: its histogram is that of rows 686..776 plus rows 775..769
    ty, tx = 7, 3
    rows = np.concatenate([np.arange(686, 777), 775 - np.arange(7)])
    cols = np.arange(tx * 126, tx * 126 + 126)
    tile = img[np.ix_(rows, cols)]
    want = np.clip(np.rint(np.cumsum(np.bincount(tile.ravel(), minlength=256)).astype(np.float32) *
                           (np.float32(255) / np.float32(126 * 98))), 0, 255).astype(np.uint8)
    assert np.array_equal(lut[ty * 8 + tx], want)


# ---- argument checks of the C ABI: no device call is made before them ----------------------------------------------------------
def _par(clip=4.0, tx=8, ty=8):
    return C.byref(_Par(clip, tx, ty))


class _Par(C.Structure):
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int)]


BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before the context is looked at


def _dev(lib, **kw):
    a = dict(src=BUF, n=2, w=64, h=48, ss=64, par=_par(), dst=BUF, ds=64, f32=1)
    a.update(kw)
    return lib.mods_clahe_dev(None, a["src"], a["n"], a["w"], a["h"], a["ss"], a["par"], a["dst"], a["ds"], a["f32"])


@pytest.mark.parametrize("kw,msg", [
    (dict(src=None), b"null image buffer"), (dict(dst=None), b"null image buffer"), (dict(par=None), b"null CLAHE parameters"),
    (dict(n=0), b"n_img 0 < 1"), (dict(w=0), b"image size 0 x 48"), (dict(h=-1), b"image size 64 x -1"),
    (dict(ss=63), b"source stride 63 < width 64"), (dict(ds=10), b"destination stride 10 < width 64"),
    (dict(par=_par(tx=0)), b"tile grid 0 x 8 outside [1, 64]"), (dict(par=_par(ty=65)), b"tile grid 8 x 65 outside [1, 64]"),
    (dict(), b"null context")])
def test_clahe_dev_argument_errors(pkg, kw, msg):
    lib = pkg.lib()
    assert _dev(lib, **kw) == -2
    err = lib.mods_last_error()
    assert err.startswith(b"mods_clahe_dev: ") and msg in err, err


@pytest.mark.parametrize("args,msg", [
    ((None, 64, 48, True, BUF), b"null image buffer"), ((BUF, 64, 48, True, None), b"null image buffer"),
    ((BUF, 64, 48, False, BUF), b"null CLAHE parameters"), ((BUF, 0, 48, True, BUF), b"image size 0 x 48"),
    ((BUF, 64, 48, "tiles", BUF), b"tile grid 65 x 8 outside [1, 64]"), ((BUF, 64, 48, True, BUF), b"null context")])
def test_clahe_host_argument_errors(pkg, args, msg):
    lib = pkg.lib()
    src, w, h, par, dst = args
    p = _par() if par is True else _par(tx=65) if par == "tiles" else None
    assert lib.mods_clahe(None, src, w, h, p, dst) == -2
    err = lib.mods_last_error()
    assert err.startswith(b"mods_clahe: ") and msg in err, err


def test_python_parameters(pkg):
    p = pkg.ClaheParams.reference()
    assert (p.clip_limit, p.tiles_x, p.tiles_y) == (4.0, 8, 8)
    assert C.sizeof(pkg.ClaheParams) == C.sizeof(_Par) == 16


def test_pipeline_refuses_bad_clahe_grid(pkg):
    """checked before any device is opened"""
    out = C.c_void_p()
    par = pkg.PairParams.default()
    assert pkg.lib().mods_pipeline_create_clahe(0, 64, 48, C.byref(par), 1, 1, 1, _par(tx=0), C.byref(out)) == -2
    assert b"CLAHE tile grid 0 x 8" in pkg.lib().mods_last_error()
