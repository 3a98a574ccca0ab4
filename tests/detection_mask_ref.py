"""The detection-mask rule of include/mods_hip.h in numpy, the masks the tests use, and what a masked call must return given the
unmasked call's lists.

A mask is a 2-D uint8 array of the image's size; a point (x, y) - the doubles a key or a region carries - is on it iff
0 <= ix < w, 0 <= iy < h and mask[iy, ix] != 0 with ix = floor(x + 0.5), iy = floor(y + 0.5), all in double arithmetic."""
import numpy as np


def on_mask(mask, x, y):
    """bool array: the rule for the points (x[i], y[i])"""
    m = np.asarray(mask)
    h, w = m.shape
    fx = np.floor(np.asarray(x, np.float64) + 0.5)
    fy = np.floor(np.asarray(y, np.float64) + 0.5)
    with np.errstate(invalid="ignore"):
        inside = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    ix = np.where(inside, fx, 0).astype(np.int64)
    iy = np.where(inside, fy, 0).astype(np.int64)
    return inside & (m[iy, ix] != 0)


def filter_regions(regs, mask):
    """the entries of a key or region list (a structured array with x, y) whose centre is on the mask, order kept"""
    return regs[on_mask(mask, regs["x"], regs["y"])]


def assert_non_vacuous(regs, mask, least=5):
    """an equivalence test proves something only when the mask both keeps and removes entries"""
    keep = on_mask(mask, regs["x"], regs["y"])
    assert keep.sum() >= least and (~keep).sum() >= least, (int(keep.sum()), int((~keep).sum()))


def assert_same_but_positions(got, want, positions=("id", "parent")):
    """two lists equal byte for byte outside the fields that store list positions"""
    assert got.dtype == want.dtype and len(got) == len(want), (len(got), len(want))
    for f in got.dtype.names:
        if f in positions:
            continue
        assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8), np.ascontiguousarray(want[f]).view(np.uint8)), f


# ---- the masks of the tests
def half_plane(w, h):
    """allowed where x + 0.37 y < 0.55 w"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(xx + 0.37 * yy < 0.55 * w, 255, 0).astype(np.uint8)


def checkerboard(w, h, cell=16):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // cell) + (yy // cell)) % 2 == 0, 255, 0).astype(np.uint8)


def random_pixels(w, h, p=0.5, seed=7):
    """every pixel allowed with probability p on its own: neighbouring pixels differ, so the rounding of the centre decides"""
    rng = np.random.default_rng(seed)
    return np.where(rng.uniform(size=(h, w)) < p, np.uint8(1), np.uint8(0)).astype(np.uint8)


def with_row_padding(mask, pad=13, poison=255):
    """the same mask as a view of a wider array (row stride w + pad) whose padding bytes are `poison`"""
    h, w = mask.shape
    wide = np.full((h, w + pad), poison, np.uint8)
    wide[:, :w] = mask
    return wide[:, :w]
