"""The mutual nearest-neighbour check of the FGINN matcher (include/mods_hip.h: mods_ctx_match_mutual) restated in numpy.  Nothing here
calls the library: this file and csrc/mutual.hip are two statements of the same contract.

A forward search has produced the tentatives (q, t).  d(a, t) = the exact integer squared L2 distance over the 128 descriptor bytes,
d1 = d(q, t); a rival is any query r != q of the same list, d_r = d(r, t).
  mode 1  dropped when some rival has d_r < d1, or d_r == d1 and r < q
  mode 2  also dropped when some rival with (xr-xq)*(xr-xq) + (yr-yq)*(yr-yq) > contradDist*contradDist (fp64, as written) fails
          (double)((float)d1 / (float)d_r) <= ratio*ratio; a quotient that is NaN or infinite fails
Survivors keep their order and every field."""
import numpy as np

CHUNK = 256        # tentatives per block of the distance matrix (memory only)


def sqdist(a, b):
    """[len(a), len(b)] exact integer squared distances of two uint8 descriptor arrays"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)       # (every value below 2^24: the fp64 products and sums are exact)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).astype(np.int64)


def keep_mask(tent, q, t, mode, ratio=0.8, contrad=10.0):
    """bool per tentative: it survives the check of `mode` (0: all do)"""
    n = len(tent)
    keep = np.ones(n, bool)
    if mode == 0 or n == 0:
        return keep
    assert mode in (1, 2)
    qd, td = np.asarray(q["desc"]), np.asarray(t["desc"])
    qx, qy = np.asarray(q["x"], np.float64), np.asarray(q["y"], np.float64)
    idx = np.arange(len(q))
    sqmin = np.float64(ratio) * np.float64(ratio)
    c2 = np.float64(contrad) * np.float64(contrad)
    for b in range(0, n, CHUNK):
        tq = np.asarray(tent["q"][b:b + CHUNK], np.int64)
        tt = np.asarray(tent["t"][b:b + CHUNK], np.int64)
        d = sqdist(td[tt], qd)                                   # [chunk, n_q]: d_r of every query for the tentative's train
        d1 = d[np.arange(len(tq)), tq][:, None]
        rival = idx[None, :] != tq[:, None]
        fail = rival & ((d < d1) | ((d == d1) & (idx[None, :] < tq[:, None])))
        if mode == 2:
            dx = qx[None, :] - qx[tq][:, None]; dy = qy[None, :] - qy[tq][:, None]
            far = dx * dx + dy * dy > c2
            with np.errstate(divide="ignore", invalid="ignore"):
                quot = (d1.astype(np.float32) / d.astype(np.float32)).astype(np.float64)
            ok = quot <= sqmin                                   # False for NaN and for +inf
            fail |= rival & far & ~ok
        keep[b:b + CHUNK] = ~fail.any(1)
    return keep


def mutual_filter(tent, q, t, mode, ratio=0.8, contrad=10.0):
    """the tentatives that survive, in their order, every field untouched"""
    return tent[keep_mask(tent, q, t, mode, ratio, contrad)]


def u6_rows(tent, q, t):
    """the correspondences (x1 y1 1 x2 y2 1) of a tentative list, as the emit stage lays them out"""
    one = np.ones(len(tent))
    return np.c_[q["x"][tent["q"]], q["y"][tent["q"]], one, t["x"][tent["t"]], t["y"][tent["t"]], one].astype(np.float64).reshape(-1, 6)


def laf_rows(tent, q, t):
    """the frames (x y a11 a12 a21 a22 s) of both regions of every tentative"""
    f = ("x", "y", "a11", "a12", "a21", "a22", "s")
    return np.c_[tuple(q[k][tent["q"]] for k in f) + tuple(t[k][tent["t"]] for k in f)].astype(np.float64).reshape(-1, 14)
