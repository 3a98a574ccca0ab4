"""ORSA-H (useF = 3) restated in numpy, operation by operation, after the contract in include/mods_hip.h: the minimal solve, the
error keys, the tables and the NFA scan of one model; and the synthetic planar scenes the ORSA-H tests share.  Python floats are
fp64 with one rounding per operation, np.float32 scalars round every operation to float: the same arithmetic as the C++ code,
which is built without contraction."""
import math

import numpy as np

F32 = np.float32
FLT_MIN = F32(np.finfo(np.float32).tiny)
W, H = 640, 480


def normalise(u6, w, h):
    """u6 (n x 6 pixels) -> p1, p2: n x 2 float32 normalised points of image 1 / 2, and norm"""
    nx, ny = F32(w), F32(h)
    norm = F32(1.0 / float(F32(math.sqrt(float(nx * ny)))))

    def one(v, half):
        return F32((float(F32(v)) - 0.5 * float(half)) * float(norm))
    p1 = np.array([[one(r[0], nx), one(r[1], ny)] for r in u6], F32)
    p2 = np.array([[one(r[3], nx), one(r[4], ny)] for r in u6], F32)
    return p1, p2, norm


def solve_h4(c):
    """c: 4 x (x1, y1, x2, y2) float32 -> (9 float32, valid)"""
    A = []
    for x, y, u, v in ([float(t) for t in row] for row in c):
        A.append([x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, u])
        A.append([0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, v])
    zero = np.zeros(9, F32)
    for k in range(8):
        p, best = k, abs(A[k][k])
        for r in range(k + 1, 8):
            if abs(A[r][k]) > best:
                best, p = abs(A[r][k]), r
        if not best > 0.0:
            return zero, False
        if p != k:
            A[k], A[p] = A[p], A[k]
        for r in range(k + 1, 8):
            f = A[r][k] / A[k][k]
            for j in range(k + 1, 9):
                A[r][j] = A[r][j] - f * A[k][j]
    x = [0.0] * 8
    for k in range(7, -1, -1):
        s = A[k][8]
        for j in range(k + 1, 8):
            s = s - A[k][j] * x[j]
        x[k] = s / A[k][k]
    with np.errstate(over="ignore"):
        h = np.array(x + [1.0], np.float64).astype(F32)
    if not np.all(np.isfinite(h)):
        return zero, False
    return h, True


def errors(Hm, p1, p2):
    """float32 errors of all correspondences under the 9 floats Hm"""
    h = [float(v) for v in Hm]
    out = np.zeros(len(p1), F32)
    with np.errstate(all="ignore"):
        for i in range(len(p1)):
            x1, y1, x2, y2 = (np.float64(p1[i][0]), np.float64(p1[i][1]), np.float64(p2[i][0]), np.float64(p2[i][1]))
            w = h[6] * x1 + h[7] * y1 + h[8]
            X = (h[0] * x1 + h[1] * y1 + h[2]) / w
            Y = (h[3] * x1 + h[4] * y1 + h[5]) / w
            dx, dy = X - x2, Y - y2
            out[i] = F32(dx * dx + dy * dy)
    return out


def logcombi(k, n):
    if k >= n or k <= 0:
        return F32(0.0)
    if n - k < k:
        k = n - k
    r = 0.0
    for i in range(1, k + 1):
        r += math.log10(float(n - i + 1)) - math.log10(float(i))
    return F32(r)


def tables(n):
    return (np.array([logcombi(k, n) for k in range(n + 1)], F32), np.array([logcombi(4, m) for m in range(n + 1)], F32))


def log10_ref(e):
    return F32(math.log10(float(e))) if e > 0 and np.isfinite(e) else (F32(np.inf) if e > 0 else F32(-np.inf))


def score(Hm, valid, p1, p2, tabs=None):
    """(nfa float32, imin, logalpha float32, invalid flag, the n NFA terms) of one model"""
    n = len(p1)
    bad = (F32(10000.0), 0, F32(10000.0), 1, None)
    if not valid:
        return bad
    e = errors(Hm, p1, p2)
    if np.any(np.isnan(e)):
        return bad
    e = np.sort(e)
    logcn, logc4 = tabs if tabs is not None else tables(n)
    logalpha0 = F32(math.log10(math.pi))
    loge0 = F32(math.log10(float(n - 4)))
    best, imin, bla = F32(10000.0), 0, F32(10000.0)
    terms = np.full(n, np.nan, F32)
    with np.errstate(all="ignore"):
        for i in range(4, n):
            la = F32(logalpha0 + log10_ref(max(e[i], FLT_MIN)))
            nfa = F32(F32(F32(loge0 + F32(la * F32(i - 3))) + logcn[i + 1]) + logc4[i + 1])
            terms[i] = nfa
            if nfa < best:
                best, imin, bla = nfa, i, la
    return best, imin, bla, 0, terms


# ---- the synthetic planar scenes --------------------------------------------------------------------------------------------

H_TRUE = np.array([[0.92, 0.11, 28.0], [-0.07, 1.04, -12.0], [1.1e-4, -0.6e-4, 1.0]])


def apply_h(Hm, xy):
    p = np.concatenate([xy, np.ones((len(xy), 1))], 1) @ np.asarray(Hm, np.float64).reshape(3, 3).T
    return p[:, :2] / p[:, 2:3]


def scene(n, inlier_ratio, sigma, seed):
    """u6 (n x 6, float32-representable), inlier flags, the noise-free inlier points (x1, y1, x2, y2)"""
    rng = np.random.default_rng(seed)
    nin = int(round(n * inlier_ratio))
    x1 = np.stack([rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)], 1)
    clean2 = apply_h(H_TRUE, x1)
    x2 = clean2 + rng.normal(0, sigma, clean2.shape)
    x1n = x1 + rng.normal(0, sigma, x1.shape)
    x2[nin:] = np.stack([rng.uniform(0, W, n - nin), rng.uniform(0, H, n - nin)], 1)
    perm = rng.permutation(n)
    inl = (np.arange(n) < nin)[perm]
    a, b = x1n[perm].astype(F32).astype(np.float64), x2[perm].astype(F32).astype(np.float64)
    ones = np.ones(n)
    u6 = np.stack([a[:, 0], a[:, 1], ones, b[:, 0], b[:, 1], ones], 1)
    clean = np.concatenate([x1[perm], clean2[perm]], 1)[inl]
    return u6, inl, clean


# name: (n, inlier ratio, sigma, generator seed, sampler seed)
SCENES = {
    "n200_r05": (200, 0.5, 1.0, 11, 101),
    "n200_r02": (200, 0.2, 1.0, 12, 102),
    "n9_all": (9, 1.0, 0.3, 13, 103),
    "n200_out": (200, 0.0, 1.0, 14, 104),
    "n12_out": (12, 0.0, 1.0, 15, 105),
}
SIGNIFICANT = ("n200_r05", "n200_r02", "n9_all")


def laf_from_u6(u6, scale=3.0):
    n = len(u6)
    laf = np.zeros((n, 14))
    laf[:, 0:2] = u6[:, 0:2]
    laf[:, 7:9] = u6[:, 3:5]
    for o in (0, 7):
        laf[:, o + 2] = 1.0
        laf[:, o + 5] = 1.0
        laf[:, o + 6] = scale
    return laf
