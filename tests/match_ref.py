"""The forward FGINN matcher (include/mods_hip.h: mods_match_fginn) restated in numpy.  Nothing here calls the library or the CPU oracle:
this file, oracle/match.cpp and csrc/match.hip are three statements of the same walk.

For every query the trains are ordered by (d, index), d = the exact integer squared L2 distance over the 128 descriptor bytes, and the
first K = min(nn, n_t) of them are walked: neighbour j = 1 .. K-1 is emitted when (double)((float)d0 / (float)dj) <= ratio*ratio (0/0 is
NaN and does not pass); otherwise the walk stops when neighbour j lies further than contradDist from the nearest train,
(x0-xj)*(x0-xj) + (y0-yj)*(y0-yj) > contradDist*contradDist in fp64.  The ratio test comes first."""
import numpy as np

TENT_DTYPE = np.dtype([("q", "i4"), ("t", "i4"), ("t_bad", "i4"), ("t_2nd", "i4"), ("d1", "f4"), ("d2", "f4"),
                       ("d2nd", "f4"), ("pad", "f4"), ("ratio", "f8")])
TF = ("q", "t", "t_bad", "t_2nd", "d1", "d2", "d2nd", "ratio")
CHUNK = 128        # queries per block of the distance matrix (memory only)
IDX_BITS = 24      # train lists are shorter than 2^24, distances below 2^24: (d << 24 | index) orders the neighbours


def sqdist(a, b):
    """[len(a), len(b)] exact integer squared distances of two uint8 descriptor arrays: |a|^2 + |b|^2 - 2 a.b with an fp64 GEMM (every
    value is an integer below 2^24, so the products and sums are exact)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).astype(np.int64)


def ratio_quotient(d0, d):
    """(double)((float)d0 / (float)d) as the reference evaluates it; NaN for 0 / 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(np.float32(d0) / np.float32(d))


def dstar(d0, ratio):
    """the smallest integer distance d >= 1 whose quotient passes, by the definition (the quotient falls as d grows)"""
    sq = np.float64(ratio) * np.float64(ratio)
    d = max(1, int(d0 / sq) - 4)
    while d > 1 and ratio_quotient(d0, d - 1) <= sq:
        d -= 1
    while not ratio_quotient(d0, d) <= sq:
        d += 1
    return d


def neighbours(q, t, k):
    """(dist[n_q, k], index[n_q, k]): the k nearest trains of every query in (d, index) order"""
    qd, td = np.asarray(q["desc"]), np.asarray(t["desc"], np.float64)
    n_q, n_t = len(qd), len(td)
    assert 1 <= k <= n_t < (1 << IDX_BITS)
    t2 = (td * td).sum(1)
    dist = np.empty((n_q, k), np.int64); index = np.empty((n_q, k), np.int64)
    for b in range(0, n_q, CHUNK):
        a = np.asarray(qd[b:b + CHUNK], np.float64)
        d = ((a * a).sum(1)[:, None] + t2[None, :] - 2 * (a @ td.T)).astype(np.int64)
        key = (d << IDX_BITS) | np.arange(n_t, dtype=np.int64)[None, :]
        if k < n_t:
            key = np.partition(key, k - 1, axis=1)[:, :k]
        key = np.sort(key, axis=1)
        dist[b:b + CHUNK] = key >> IDX_BITS
        index[b:b + CHUNK] = key & ((1 << IDX_BITS) - 1)
    return dist, index


def match_fginn(q, t, ratio=0.8, contrad=10.0, nn=50, nb=None):
    """the tentative list of MatchFlannFGINN with an exact linear index, in query order (nb: neighbours(q, t, min(nn, len(t))) where the
    caller has them already)"""
    assert ratio * ratio < 1.0
    n_q, n_t = len(q), len(t)
    out = np.zeros(n_q, TENT_DTYPE)
    if n_q == 0 or n_t == 0:
        return out[:0]
    K = min(int(nn), n_t)
    if K < 2:
        return out[:0]
    sq = np.float64(ratio) * np.float64(ratio)
    c2 = np.float64(contrad) * np.float64(contrad)
    dist, index = nb if nb is not None else neighbours(q, t, K)
    assert dist.shape == (n_q, K)
    tx, ty = np.asarray(t["x"], np.float64), np.asarray(t["y"], np.float64)
    n = 0
    for i in range(n_q):
        d, ix = dist[i], index[i]
        for j in range(1, K):
            quot = ratio_quotient(d[0], d[j])
            if quot <= sq:
                out[n] = (i, ix[0], ix[j], ix[1], np.float32(d[0]), np.float32(d[j]), np.float32(d[1]), 0.0, np.sqrt(quot))
                n += 1
                break
            dx, dy = tx[ix[0]] - tx[ix[j]], ty[ix[0]] - ty[ix[j]]
            if dx * dx + dy * dy > c2:
                break
    return out[:n].copy()


def u6_rows(tent, q, t):
    """the correspondences (x1 y1 1 x2 y2 1) of a tentative list, as the emit stage lays them out"""
    one = np.ones(len(tent))
    return np.c_[q["x"][tent["q"]], q["y"][tent["q"]], one, t["x"][tent["t"]], t["y"][tent["t"]], one].astype(np.float64).reshape(-1, 6)
