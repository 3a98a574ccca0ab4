"""numpy restatement of the overlap-matching contract (include/mods_hip.h: mods_match_overlap) - the reference of
tests/test_cpu_overlap.py and tests/test_gpu_overlap.py.  float64, one numpy operation per rounding in the order the contract writes
them; it never calls the library.  The n_q x n_t errors are formed in blocks of query rows, so 5000 x 4099 stays small in memory."""
from types import SimpleNamespace

import numpy as np

from guided_ref import REGION_DTYPE, _project, invert3, model_entries

OVERLAP_DTYPE = np.dtype([("q", "i4"), ("t", "i4"), ("E", "f8"), ("dist", "f8"), ("diff", "f8")])
CHUNK = 256   # query rows of the error matrix held at once


def params(H, max_error=0.09, oriented=1, one_to_one=1, w1=0, h1=0, w2=0, h2=0):
    """the fields of mods_overlap_params; overlap_ref takes this or the package's OverlapParams"""
    return SimpleNamespace(H=[float(v) for v in np.asarray(H, np.float64).reshape(9)], max_error=float(max_error), oriented=int(oriented),
                           one_to_one=int(one_to_one), w1=int(w1), h1=int(h1), w2=int(w2), h2=int(h2))


def _f(r, name):
    return np.ascontiguousarray(r[name], np.float64)


def query_records(q, H):
    """px, py, C11, C12, C21, C22 of the contract"""
    H = [float(v) for v in np.asarray(H, np.float64).reshape(9)]
    x, y, s = _f(q, "x"), _f(q, "y"), _f(q, "s")
    with np.errstate(all="ignore"):
        X = (H[0] * x + H[1] * y) + H[2]
        Y = (H[3] * x + H[4] * y) + H[5]
        den = (H[6] * x + H[7] * y) + H[8]
        px = X / den; py = Y / den
        den2 = den * den
        n1 = X / den2; n2 = Y / den2
        L11 = H[0] / den - n1 * H[6]; L12 = H[1] / den - n1 * H[7]
        L21 = H[3] / den - n2 * H[6]; L22 = H[4] / den - n2 * H[7]
        ks = 3.0 * s
        B11 = ks * _f(q, "a11"); B12 = ks * _f(q, "a12"); B21 = ks * _f(q, "a21"); B22 = ks * _f(q, "a22")
        C11 = L11 * B11 + L12 * B21; C12 = L11 * B12 + L12 * B22
        C21 = L21 * B11 + L22 * B21; C22 = L21 * B12 + L22 * B22
    return px, py, C11, C12, C21, C22


def train_records(t):
    """x2, y2, I11, I12, I21, I22 of the contract"""
    with np.errstate(all="ignore"):
        ks = 3.0 * _f(t, "s")
        M11 = ks * _f(t, "a11"); M12 = ks * _f(t, "a12"); M21 = ks * _f(t, "a21"); M22 = ks * _f(t, "a22")
        d = 1.0 / (M11 * M22 - M12 * M21)
        return _f(t, "x"), _f(t, "y"), M22 * d, -(M12 * d), -(M21 * d), M11 * d


def _pair(qr, tr, oriented):
    px, py, C11, C12, C21, C22 = (a[:, None] for a in qr)
    x2, y2, I11, I12, I21, I22 = (a[None, :] for a in tr)
    with np.errstate(all="ignore"):
        dx = px - x2; dy = py - y2
        u = I11 * dx + I12 * dy; v = I21 * dx + I22 * dy
        dist = u * u + v * v
        G11 = I11 * C11 + I12 * C21; G12 = I11 * C12 + I12 * C22
        G21 = I21 * C11 + I22 * C21; G22 = I21 * C12 + I22 * C22
        if not oriented:
            det = np.sqrt(np.fabs(G11 * G22 - G12 * G21))
            r = np.sqrt(G12 * G12 + G11 * G11)
            g21 = (G22 * G12 + G21 * G11) / (r * det)
            G11, G12, G21, G22 = r / det, np.zeros_like(det), g21, det / r
        diff = 0.5 * ((((1 - G11) * (1 - G11) + G12 * G12) + G21 * G21) + (1 - G22) * (1 - G22))
        E = diff + dist
    return E, dist, diff


def pair_errors(q, t, H, oriented, rows=None):
    """(E, dist, diff), each [len(rows), n_t], of the queries `rows` (a slice or an index array; None: all) against every train -
    the common area does not enter"""
    qs = q if rows is None else q[rows]
    return _pair(query_records(qs, H), train_records(t), oriented)


def common_masks(q, t, p):
    """which queries / trains take part"""
    n_q, n_t = len(q), len(t)
    if not (p.w1 > 0 and p.h1 > 0 and p.w2 > 0 and p.h2 > 0):
        return np.ones(n_q, bool), np.ones(n_t, bool)
    px, py = query_records(q, list(p.H))[:2]
    Hi = invert3(model_entries(0, list(p.H)))
    with np.errstate(all="ignore"):
        bx, by = _project(Hi, _f(t, "x"), _f(t, "y"))
        mq = (0.0 < px) & (px < float(p.w2)) & (0.0 < py) & (py < float(p.h2))
        mt = (0.0 < bx) & (bx < float(p.w1)) & (0.0 < by) & (by < float(p.h1))
    return mq, mt


def overlap_ref(q, t, p):
    """returns (matches as OVERLAP_DTYPE rows in query order, counts) of the contract; p: params() or an OverlapParams"""
    n_q, n_t = len(q), len(t)
    H = list(p.H)
    mq, mt = common_masks(q, t, p)
    picks = []                                            # (q, t1, E1, dist, diff)
    if n_q and n_t:
        tr = train_records(t)
        qr = query_records(q, H)
        for q0 in range(0, n_q, CHUNK):
            q1 = min(n_q, q0 + CHUNK)
            E, dist, diff = _pair(tuple(a[q0:q1] for a in qr), tr, p.oriented)
            valid = (E < p.max_error) & mq[q0:q1, None] & mt[None, :]
            j = np.argmin(np.where(valid, E, np.inf), axis=1)       # the first minimum: ties go to the lower train index
            for i in np.nonzero(valid.any(axis=1))[0]:
                picks.append((q0 + int(i), int(j[i]), E[i, j[i]], dist[i, j[i]], diff[i, j[i]]))
    if p.one_to_one:
        owner = {}
        for (i, t1, e, _, _) in picks:
            if t1 not in owner or (e, i) < owner[t1]:
                owner[t1] = (e, i)
        picks = [k for k in picks if owner[k[1]][1] == k[0]]
    out = np.zeros(len(picks), OVERLAP_DTYPE)
    for s, (i, t1, e, d, f) in enumerate(picks):
        out[s] = (i, t1, e, d, f)
    lo = min(int(mq.sum()), int(mt.sum()))
    counts = SimpleNamespace(n_q_common=int(mq.sum()), n_t_common=int(mt.sum()), n_matches=len(picks),
                             repeatability=(float(len(picks)) / float(lo)) if lo > 0 else 0.0)
    return out, counts


# ---- the synthetic scene of the tests ------------------------------------------------------------------------------------------

H_PROJ = np.array([[0.93, -0.11, 21.5], [0.07, 1.04, -13.25], [1.1e-4, -6.0e-5, 1.0]])


def regions(xy, s, A):
    """REGION_DTYPE rows from centres [n, 2], scales [n] and frames [n, 2, 2]"""
    n = len(s)
    r = np.zeros(n, REGION_DTYPE)
    if n:
        r["x"], r["y"] = np.asarray(xy, np.float64).reshape(n, 2).T
        r["s"] = s
        A = np.asarray(A, np.float64).reshape(n, 2, 2)
        r["a11"], r["a12"], r["a21"], r["a22"] = A[:, 0, 0], A[:, 0, 1], A[:, 1, 0], A[:, 1, 1]
    r["id"] = np.arange(n)
    return r


def random_frames(rng, n):
    """lower triangular (determinant 1) times a rotation"""
    a = rng.uniform(0.6, 1.6, n)
    L = np.zeros((n, 2, 2)); L[:, 0, 0] = a; L[:, 1, 1] = 1.0 / a; L[:, 1, 0] = rng.uniform(-0.5, 0.5, n)
    th = rng.uniform(-np.pi, np.pi, n)
    R = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    return L @ R


def lin_h(H, xy):
    """the Jacobian of the homography at xy [n, 2] and the mapped points"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = np.c_[xy, np.ones(len(xy))] @ H.T
    w = p[:, 2]
    J = np.empty((len(xy), 2, 2))
    for i in range(2):
        for j in range(2):
            J[:, i, j] = H[i, j] / w - p[:, i] / (w * w) * H[2, j]
    return J, p[:, :2] / w[:, None]


def scene(rng, n_q, n_t, H=H_PROJ, w=400.0, h=300.0):
    """queries anywhere in w x h with random frames, s in 1.5 - 12; two thirds of the trains are H-images of random queries (centre
    noise 0.15 s, relative shape noise 8 %), the rest clutter; trains in random order"""
    qxy = rng.uniform(0, 1, (n_q, 2)) * (w, h)
    qs = rng.uniform(1.5, 12.0, n_q)
    qA = random_frames(rng, n_q)
    q = regions(qxy, qs, qA)
    txy = rng.uniform(0, 1, (n_t, 2)) * (w, h)
    ts = rng.uniform(1.5, 12.0, n_t)
    tA = random_frames(rng, n_t)
    m = min(n_q, (2 * n_t) // 3) if n_q else 0
    if m:
        src = rng.integers(0, n_q, m)
        J, pxy = lin_h(H, qxy[src])
        txy[:m] = pxy + rng.standard_normal((m, 2)) * (0.15 * qs[src])[:, None]
        M = (J @ (qs[src][:, None, None] * qA[src])) * (1.0 + 0.08 * rng.standard_normal((m, 2, 2)))
        ts[:m] = np.sqrt(np.abs(np.linalg.det(M)))
        tA[:m] = M / ts[:m][:, None, None]
    perm = rng.permutation(n_t)
    return q, regions(txy[perm], ts[perm], tA[perm])
