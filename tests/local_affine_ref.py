"""The contract of the local affine consistency filter (include/mods_hip.h: mods_filter_local_affine) restated in numpy: fp64, one
numpy operation per rounding of the header's formulas, in their order.  Chunked over rows so that a few thousand tentatives need no
n x n x dozens of arrays at once.  Never calls the library."""
import numpy as np

DEFAULTS = dict(radius=160.0, minDist=3.0, absTol=4.0, relTol=0.2, areaTol=2.0, minSupport=3, rescue=1, keepSparse=1)
TENT_DTYPE = np.dtype([("q", "i4"), ("t", "i4"), ("t_bad", "i4"), ("t_2nd", "i4"), ("d1", "f4"), ("d2", "f4"), ("d2nd", "f4"),
                       ("pad", "f4"), ("ratio", "f8")])


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        if k not in p:
            raise TypeError(k)
    p.update(kw)
    return p


def frames(laf):
    """(t00, t01, t10, t11, dT, valid) per tentative"""
    laf = np.asarray(laf, np.float64).reshape(-1, 14)
    with np.errstate(all="ignore"):
        s1, s2 = laf[:, 6], laf[:, 13]
        m00 = s1 * laf[:, 2]; m01 = s1 * laf[:, 3]; m10 = s1 * laf[:, 4]; m11 = s1 * laf[:, 5]
        n00 = s2 * laf[:, 9]; n01 = s2 * laf[:, 10]; n10 = s2 * laf[:, 11]; n11 = s2 * laf[:, 12]
        det = m00 * m11 - m01 * m10
        i00 = m11 / det; i01 = (-m01) / det; i10 = (-m10) / det; i11 = m00 / det
        t00 = n00 * i00 + n01 * i10; t01 = n00 * i01 + n01 * i11
        t10 = n10 * i00 + n11 * i10; t11 = n10 * i01 + n11 * i11
        dT = t00 * t11 - t01 * t10
        valid = np.isfinite(t00) & np.isfinite(t01) & np.isfinite(t10) & np.isfinite(t11) & np.isfinite(dT) & (dT != 0)
    return t00, t01, t10, t11, dT, valid


def diagnostics(laf, p=None, chunk=256):
    """dict of keep (bool), neighbours, support, backed (int32), indexed by input position"""
    p = params(**(p or {}))
    laf = np.asarray(laf, np.float64).reshape(-1, 14)
    n = len(laf)
    R2 = np.float64(p["radius"]) * np.float64(p["radius"])
    D2 = np.float64(p["minDist"]) * np.float64(p["minDist"])
    A2 = np.float64(p["absTol"]) * np.float64(p["absTol"])
    L2 = np.float64(p["relTol"]) * np.float64(p["relTol"])
    area = np.float64(p["areaTol"])
    x1, y1, x2, y2 = laf[:, 0], laf[:, 1], laf[:, 7], laf[:, 8]
    t00, t01, t10, t11, dT, valid = frames(laf)
    nbs = np.zeros(n, np.int32)
    sup = np.zeros(n, np.int32)
    ok_rows = []                     # (first row, ok block) for the second pass
    with np.errstate(all="ignore"):
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            dx = x1[None, :] - x1[a:b, None]; dy = y1[None, :] - y1[a:b, None]
            r2 = dx * dx + dy * dy
            gx = x2[None, :] - x2[a:b, None]; gy = y2[None, :] - y2[a:b, None]
            q2 = gx * gx + gy * gy
            nb = (r2 <= R2) & (r2 >= D2) & (q2 >= D2)
            nb[np.arange(b - a), np.arange(a, b)] = False            # j != i
            mx = t00[a:b, None] * dx + t01[a:b, None] * dy
            my = t10[a:b, None] * dx + t11[a:b, None] * dy
            ex = gx - mx; ey = gy - my
            e2 = ex * ex + ey * ey
            m2 = mx * mx + my * my
            ok = nb & valid[a:b, None] & (e2 <= A2 + L2 * m2)
            if area != 0:
                di, dj = dT[a:b, None], dT[None, :]
                lo = np.minimum(np.abs(di), np.abs(dj)); hi = np.maximum(np.abs(di), np.abs(dj))
                ok &= valid[None, :] & (di * dj > 0) & (lo * area >= hi)
            nbs[a:b] = nb.sum(1)
            sup[a:b] = ok.sum(1)
            ok_rows.append((a, np.packbits(ok, axis=1)))
    strong = sup >= p["minSupport"]
    backed = np.zeros(n, np.int64)
    for a, packed in ok_rows:
        ok = np.unpackbits(packed, axis=1, count=n).astype(bool)
        backed += (ok & strong[a:a + len(ok), None]).sum(0)
    backed = backed.astype(np.int32)
    keep = strong.copy()
    if p["rescue"]:
        keep |= backed > 0
    if p["keepSparse"]:
        keep |= nbs < p["minSupport"]
    return {"keep": keep, "neighbours": nbs, "support": sup, "backed": backed}


def filter_lists(tent, u6, laf, p=None):
    """(tent, u6, laf) of the survivors in list order, and the diagnostics"""
    d = diagnostics(laf, p)
    k = d["keep"]
    return np.asarray(tent)[k], np.asarray(u6, np.float64).reshape(-1, 6)[k], np.asarray(laf, np.float64).reshape(-1, 14)[k], d


def make_lists(x1, x2, A1=None, A2=None, s1=None, s2=None):
    """(tent, u6, laf) of tentatives at x1[n][2] -> x2[n][2]; frames default to the identity with s = 1"""
    x1 = np.asarray(x1, np.float64).reshape(-1, 2); x2 = np.asarray(x2, np.float64).reshape(-1, 2)
    n = len(x1)
    eye = np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (n, 1))
    A1 = eye if A1 is None else np.asarray(A1, np.float64).reshape(n, 4)
    A2 = eye if A2 is None else np.asarray(A2, np.float64).reshape(n, 4)
    s1 = np.ones(n) if s1 is None else np.asarray(s1, np.float64)
    s2 = np.ones(n) if s2 is None else np.asarray(s2, np.float64)
    laf = np.zeros((n, 14))
    laf[:, 0:2] = x1; laf[:, 2:6] = A1; laf[:, 6] = s1
    laf[:, 7:9] = x2; laf[:, 9:13] = A2; laf[:, 13] = s2
    u6 = np.ones((n, 6))
    u6[:, 0:2] = x1; u6[:, 3:5] = x2
    tent = np.zeros(n, TENT_DTYPE)
    tent["q"] = np.arange(n); tent["t"] = np.arange(n)[::-1]
    tent["d1"] = np.arange(n) + 1.0; tent["d2"] = 2.0 * np.arange(n) + 3.0; tent["ratio"] = 0.5 + 0.001 * np.arange(n)
    return tent, u6, laf


# ---- the hand-computed scenes of tests/test_cpu_local_affine.py (also sent through the device by tests/test_gpu_local_affine.py)
def five_points():
    x1 = [(0, 0), (10, 0), (0, 10), (10, 10), (5, 5)]
    x2 = [(x + 100, y + 50) for x, y in x1[:4]] + [(300, 300)]
    return make_lists(x1, x2)


def two_points(x2=((50, 50), (56, 58)), s2=(1, 1)):
    return make_lists([(0, 0), (3, 4)], x2, s2=s2)


THRESHOLD = dict(radius=5.0, minDist=5.0, absTol=5.0, relTol=0.0, areaTol=0.0, minSupport=1)


def degenerate_frames():
    """the five points with four more in the square that move with it, each with one broken frame: s1 = 0, a11 a22 = a12 a21,
    s2 = inf, NaN in x2.  Returns (tent, u6, laf, indices of the broken four)"""
    x1 = [(0, 0), (10, 0), (0, 10), (10, 10), (5, 5), (4, 0), (0, 4), (10, 4), (4, 10)]
    x2 = [(x + 100, y + 50) for x, y in x1]
    x2[4] = (300, 300)
    tent, u6, laf = make_lists(x1, x2)
    laf[5, 6] = 0.0                                   # s1 = 0
    laf[6, 2:6] = (1.0, 2.0, 2.0, 4.0)                # singular A1
    laf[7, 13] = np.inf                               # s2 = inf
    laf[8, 7] = np.nan                                # NaN in x2
    u6[8, 3] = np.nan
    return tent, u6, laf, [5, 6, 7, 8]


def rescue_scene():
    """A cluster of four that move together; a fifth next to it that moves with them but whose own frame is broken (supports
    nobody, is confirmed by the four strong ones: kept by rescue only); a sixth far from everybody (no neighbours: kept by
    keepSparse only)."""
    x1 = [(0, 0), (10, 0), (0, 10), (10, 10), (5, 5), (1000, 1000)]
    x2 = [(x + 100, y + 50) for x, y in x1]
    tent, u6, laf = make_lists(x1, x2)
    laf[4, 9:13] = (3.0, 0.0, 0.0, 3.0)               # T_4 = 3 I: its predictions miss; dT = 9
    return tent, u6, laf


def planar_scene(n=2000, inlier_ratio=0.2, w=1920, h=1080, seed=1, laf_noise=0.03, pos_noise=0.3):
    """A synthetic planar scene: inliers follow a homography with mild perspective, their image-2 frames are the image-1 frames mapped
    by the homography's Jacobian with a few percent of multiplicative noise, positions carry sub-pixel noise; outliers are uniform in
    both images with random frames.  Returns (tent, u6, laf, is_true)."""
    rng = np.random.default_rng(seed)
    H = np.array([[0.92, 0.08, 40.0], [-0.06, 0.95, 25.0], [4e-5, -2e-5, 1.0]])
    n_in = int(round(n * inlier_ratio))
    x1 = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    ang = rng.uniform(0, 2 * np.pi, n)
    sc = rng.uniform(0.7, 1.4, n)
    A1 = np.stack([sc * np.cos(ang), -np.sin(ang) / sc, sc * np.sin(ang), np.cos(ang) / sc], 1)
    s1 = rng.uniform(2.0, 12.0, n)
    is_true = np.zeros(n, bool)
    is_true[rng.permutation(n)[:n_in]] = True
    x2 = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    ang2 = rng.uniform(0, 2 * np.pi, n)
    A2 = np.stack([np.cos(ang2), -np.sin(ang2), np.sin(ang2), np.cos(ang2)], 1)
    s2 = rng.uniform(2.0, 12.0, n)
    t = np.flatnonzero(is_true)
    X, Y = x1[t, 0], x1[t, 1]
    den = H[2, 0] * X + H[2, 1] * Y + H[2, 2]
    u = (H[0, 0] * X + H[0, 1] * Y + H[0, 2]) / den
    v = (H[1, 0] * X + H[1, 1] * Y + H[1, 2]) / den
    x2[t] = np.stack([u, v], 1) + rng.normal(0, pos_noise, (len(t), 2))
    J = np.empty((len(t), 2, 2))
    J[:, 0, 0] = (H[0, 0] - u * H[2, 0]) / den; J[:, 0, 1] = (H[0, 1] - u * H[2, 1]) / den
    J[:, 1, 0] = (H[1, 0] - v * H[2, 0]) / den; J[:, 1, 1] = (H[1, 1] - v * H[2, 1]) / den
    M1 = s1[t, None, None] * A1[t].reshape(-1, 2, 2)
    M2 = np.einsum("nij,njk->nik", J, M1) * (1.0 + rng.normal(0, laf_noise, (len(t), 2, 2)))
    s2[t] = np.sqrt(np.abs(np.linalg.det(M2)))
    A2[t] = (M2 / s2[t, None, None]).reshape(-1, 4)
    tent, u6, laf = make_lists(x1, x2, A1, A2, s1, s2)
    return tent, u6, laf, is_true
