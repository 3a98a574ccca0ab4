"""numpy restatement of the guided-matching contract (include/mods_hip.h: mods_match_guided) - the reference of
tests/test_cpu_guided.py and tests/test_gpu_guided.py.  float64, one numpy operation per rounding in the order the contract writes
them, integer descriptor distances; it never calls the library."""
import numpy as np

REGION_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("s", "f8"), ("a11", "f8"), ("a12", "f8"), ("a21", "f8"),
                         ("a22", "f8"), ("response", "f8"), ("sub_type", "i4"), ("id", "i4"), ("parent", "i4"),
                         ("pad", "i4"), ("desc", "u1", (128,))])
TENT_DTYPE = np.dtype([("q", "i4"), ("t", "i4"), ("t_bad", "i4"), ("t_2nd", "i4"), ("d1", "f4"), ("d2", "f4"),
                       ("d2nd", "f4"), ("pad", "f4"), ("ratio", "f8")])
CHUNK = 256   # query rows of the gate matrix held at once


def model_entries(model_type, model):
    """M[i][j] = entry (i, j): type 0 row-major H, type 1 F as degensac stores it (F[3 * c + r] = entry (r, c))"""
    m = [float(v) for v in np.asarray(model, np.float64).reshape(9)]
    if model_type == 0:
        return [[m[3 * i + j] for j in range(3)] for i in range(3)]
    return [[m[3 * j + i] for j in range(3)] for i in range(3)]


def invert3(M):
    """adjugate times the reciprocal of the determinant, the closed form of cv::invert for 3 x 3; None when singular"""
    S = [M[i][j] for i in range(3) for j in range(3)]
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if d == 0.0 or not np.isfinite(d):
        return None
    d = 1.0 / d
    t = [(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
         (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
         (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d]
    return [t[0:3], t[3:6], t[6:9]]


def _project(M, x, y):
    X = (M[0][0] * x + M[0][1] * y) + M[0][2]
    Y = (M[1][0] * x + M[1][1] * y) + M[1][2]
    W = (M[2][0] * x + M[2][1] * y) + M[2][2]
    return X / W, Y / W


def gate_rows(model_type, model, radius, q, t, q0, q1):
    """boolean gate matrix of the queries [q0, q1) against every train"""
    M = model_entries(model_type, model)
    r2 = float(radius) * float(radius)
    x1 = q["x"][q0:q1].astype(np.float64); y1 = q["y"][q0:q1].astype(np.float64)
    x2 = t["x"].astype(np.float64); y2 = t["y"].astype(np.float64)
    with np.errstate(all="ignore"):
        if model_type == 0:
            Mi = invert3(M)
            px, py = _project(M, x1, y1)
            bx, by = _project(Mi, x2, y2)
            dx = px[:, None] - x2[None, :]; dy = py[:, None] - y2[None, :]
            ex = bx[None, :] - x1[:, None]; ey = by[None, :] - y1[:, None]
            return (dx * dx + dy * dy <= r2) & (ex * ex + ey * ey <= r2)
        a = (M[0][0] * x1 + M[0][1] * y1) + M[0][2]
        b = (M[1][0] * x1 + M[1][1] * y1) + M[1][2]
        c0 = (M[2][0] * x1 + M[2][1] * y1) + M[2][2]
        gq = r2 * (a * a + b * b)
        a2 = (M[0][0] * x2 + M[1][0] * y2) + M[2][0]
        b2 = (M[0][1] * x2 + M[1][1] * y2) + M[2][1]
        gt = r2 * (a2 * a2 + b2 * b2)
        e = (a[:, None] * x2[None, :] + b[:, None] * y2[None, :]) + c0[:, None]
        e2 = e * e
        return (e2 <= gq[:, None]) & (e2 <= gt[None, :])


def _first_min(d, idx):
    """position of the smallest (d, idx) pair; idx ascends, so the first minimum of d is it"""
    return int(np.argmin(d))


def guided_ref(q, t, model_type, model, radius, ratio, contrad, max_dist=0, one_to_one=0):
    """returns (tent, u6, laf) of the contract"""
    n_q, n_t = len(q), len(t)
    rho2 = float(ratio) * float(ratio)
    c2 = float(contrad) * float(contrad)
    dq = q["desc"].astype(np.int64); dt = t["desc"].astype(np.int64)
    x2 = t["x"].astype(np.float64); y2 = t["y"].astype(np.float64)
    picks = []                                            # (q, t1, d1, t_bad, d2)
    for q0 in range(0, n_q, CHUNK):
        q1 = min(n_q, q0 + CHUNK)
        if n_t == 0:
            break
        g = gate_rows(model_type, model, radius, q, t, q0, q1)
        for i in range(q0, q1):
            idx = np.nonzero(g[i - q0])[0]
            if len(idx) == 0:
                continue
            diff = dq[i][None, :] - dt[idx]
            d = (diff * diff).sum(axis=1)
            j = _first_min(d, idx)
            t1, d1 = int(idx[j]), int(d[j])
            cx = x2[idx] - x2[t1]; cy = y2[idx] - y2[t1]
            far = (cx * cx + cy * cy > c2) & (idx != t1)
            t_bad, d2 = -1, 0
            if far.any():
                j2 = _first_min(d[far], idx[far])
                t_bad, d2 = int(idx[far][j2]), int(d[far][j2])
            ok = (max_dist == 0 or d1 <= max_dist) and (t_bad < 0 or float(d1) < rho2 * float(d2))
            if ok:
                picks.append((i, t1, d1, t_bad, d2))
    if one_to_one:
        owner = {}
        for (i, t1, d1, _, _) in picks:
            if t1 not in owner or (d1, i) < owner[t1]:
                owner[t1] = (d1, i)
        picks = [p for p in picks if owner[p[1]][1] == p[0]]
    n = len(picks)
    tent = np.zeros(n, TENT_DTYPE); u6 = np.zeros((n, 6), np.float64); laf = np.zeros((n, 14), np.float64)
    for s, (i, t1, d1, t_bad, d2) in enumerate(picks):
        tent[s]["q"], tent[s]["t"], tent[s]["t_bad"], tent[s]["t_2nd"] = i, t1, t_bad, -1
        tent[s]["d1"], tent[s]["d2"] = np.float32(d1), np.float32(d2)
        tent[s]["ratio"] = np.sqrt(np.float64(d1) / np.float64(d2)) if t_bad >= 0 else 0.0
        a, b = q[i], t[t1]
        u6[s] = [a["x"], a["y"], 1.0, b["x"], b["y"], 1.0]
        laf[s] = [a["x"], a["y"], a["a11"], a["a12"], a["a21"], a["a22"], a["s"],
                  b["x"], b["y"], b["a11"], b["a12"], b["a21"], b["a22"], b["s"]]
    return tent, u6, laf
