"""numpy restatement of the least-squares refinement contract (include/mods_hip.h: mods_refine_matches) - the reference of
tests/test_cpu_lsm.py and tests/test_gpu_lsm.py.  float64 on float32 pixels, the operations in the order the contract writes them;
it never calls the library.

The one thing it does not restate is the order of the window sums (lane-strided partial sums and a butterfly on the device): here a
sum is taken sequentially over k, ascending (order="forward") or descending (order="reverse").  The difference between those two
runs is the yardstick the kernel is held to (tests/test_gpu_lsm.py)."""
import math

import numpy as np

OK, MAXITER, BAD_FRAME, OUTSIDE, FLAT, DIVERGED, LOW_ZNCC = range(7)
STATUS_NAMES = ("OK", "MAXITER", "BAD_FRAME", "OUTSIDE", "FLAT", "DIVERGED", "LOW_ZNCC")
DEFAULTS = dict(radius=10, max_iter=20, eps_shift=0.01, max_shift=3.0, max_scale_change=1.5, max_magnification=8.0, min_zncc=0.8,
                lam=1e-9, affine=1)
FLAT_EPS = 1e-6          # FLAT when sum(T T) <= FLAT_EPS * S


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("no parameter %r" % k)
        p[k] = v
    return p


def _sum(x, order):
    """sequential sum over axis 0 (np.add.accumulate adds one term after the other)"""
    x = np.asarray(x, np.float64)
    if order == "reverse":
        x = x[::-1]
    return np.add.accumulate(x, axis=0)[-1]


def bil(img, x, y):
    """value, gx, gy of the bilinear patch at the positions (x, y) (arrays); ok = False when any tap is outside or not finite"""
    h, w = img.shape
    with np.errstate(invalid="ignore"):
        xf, yf = np.floor(x), np.floor(y)
        inside = (xf >= 0) & (yf >= 0) & (xf <= w - 2) & (yf <= h - 2)
    if not inside.all():
        return None, None, None, False
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    fx, fy = x - xf, y - yf
    ex, ey = 1.0 - fx, 1.0 - fy
    a, b = img[y0, x0].astype(np.float64), img[y0, x0 + 1].astype(np.float64)
    c, d = img[y0 + 1, x0].astype(np.float64), img[y0 + 1, x0 + 1].astype(np.float64)
    v = (a * ex + b * fx) * ey + (c * ex + d * fx) * fy
    gx = (b - a) * ey + (d - c) * fy
    gy = (c - a) * ex + (d - b) * fx
    return v, gx, gy, True


def cholesky_solve(N, g):
    """delta = N^-1 g with N = L L^T, lower, column by column; None when a pivot is not > 0 (NaN included)"""
    P = len(g)
    L = [[0.0] * P for _ in range(P)]
    for j in range(P):
        s = float(N[j][j])
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, P):
            t = float(N[i][j])
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    y = [0.0] * P
    for i in range(P):
        t = float(g[i])
        for k in range(i):
            t = t - L[i][k] * y[k]
        y[i] = t / L[i][i]
    x = [0.0] * P
    for i in range(P - 1, -1, -1):
        t = y[i]
        for k in range(i + 1, P):
            t = t - L[k][i] * x[k]
        x[i] = t / L[i][i]
    return x


def _zncc(Swt, Sww, Stt):
    q = Sww * Stt
    return Swt / math.sqrt(q) if q > 0.0 else 0.0


def roles(row):
    """None (BAD_FRAME without the magnification test), or (swapped, B[4], M_template[4])"""
    f = [float(v) for v in row]
    if not all(math.isfinite(v) for v in f):
        return None
    m00, m01, m10, m11 = f[6] * f[2], f[6] * f[3], f[6] * f[4], f[6] * f[5]
    n00, n01, n10, n11 = f[13] * f[9], f[13] * f[10], f[13] * f[11], f[13] * f[12]
    d1, d2 = m00 * m11 - m01 * m10, n00 * n11 - n01 * n10
    if d1 == 0.0 or d2 == 0.0:
        return None
    i00, i01, i10, i11 = m11 / d1, (-m01) / d1, (-m10) / d1, m00 / d1
    b00, b01 = n00 * i00 + n01 * i10, n00 * i01 + n01 * i11
    b10, b11 = n10 * i00 + n11 * i10, n10 * i01 + n11 * i11
    dB0 = b00 * b11 - b01 * b10
    if not all(math.isfinite(v) for v in (b00, b01, b10, b11, dB0)) or not dB0 > 0.0:
        return None
    if dB0 >= 1.0:
        return False, [b00, b01, b10, b11], [m00, m01, m10, m11]
    return True, [b11 / dB0, (-b01) / dB0, (-b10) / dB0, b00 / dB0], [n00, n01, n10, n11]


def refine_row(img1, img2, row, par=None, order="forward", trace=None):
    """one correspondence: (row_out[14], status, iterations, zncc_before, zncc_after).  trace, a dict, receives N (P x P, damped),
    g, a and delta of the first iteration"""
    p = par if par is not None else DEFAULTS
    f = np.array(row, np.float64)
    rejected = lambda st, it=0, zb=0.0, za=0.0: (np.array(row, np.float64), st, it, zb, za)
    ro = roles(row)
    if ro is None:
        return rejected(BAD_FRAME)
    swapped, B, Mt = ro
    detB0 = B[0] * B[3] - B[1] * B[2]
    if not math.sqrt(detB0) <= p["max_magnification"]:
        return rejected(BAD_FRAME)
    It, Is = (img2, img1) if swapped else (img1, img2)
    ct = (f[7], f[8]) if swapped else (f[0], f[1])
    cs = (f[0], f[1]) if swapped else (f[7], f[8])
    R = int(p["radius"])
    Wd = 2 * R + 1
    S = Wd * Wd
    k = np.arange(S)
    ux, uy = (k % Wd - R).astype(np.float64), (k // Wd - R).astype(np.float64)
    T, _, _, ok = bil(It, ct[0] + ux, ct[1] + uy)
    if not ok:
        return rejected(OUTSIDE)
    T = T - _sum(T, order) / S
    Stt = _sum(T * T, order)
    if Stt <= FLAT_EPS * S:
        return rejected(FLAT)
    P = 6 if p["affine"] else 2
    cx, cy = cs
    B00, B01, B10, B11 = B
    zb = za = 0.0
    iters = 0
    final = maxiter = False
    it = 0
    while True:
        px, py = cx + (B00 * ux + B01 * uy), cy + (B10 * ux + B11 * uy)
        W, gx, gy, ok = bil(Is, px, py)
        if not ok:
            return rejected(OUTSIDE, iters, zb)
        cols = np.stack([W, gx, gy, gx * ux, gx * uy, gy * ux, gy * uy], axis=1)
        mean = _sum(cols, order) / S
        Wc = W - mean[0]
        Swt, Sww = _sum(Wc * T, order), _sum(Wc * Wc, order)
        with np.errstate(all="ignore"):
            z = _zncc(Swt, Sww, Stt)
            if it == 0:
                zb = z
            if final:
                za = z
                break
            a = np.float64(Swt) / np.float64(Sww)
            r = T - a * Wc
            J = a * (cols[:, 1:] - mean[1:])
            N = np.zeros((6, 6))
            g = np.zeros(6)
            for i in range(6):
                for j in range(i + 1):
                    N[i, j] = N[j, i] = _sum(J[:, i] * J[:, j], order)
                g[i] = _sum(J[:, i] * r, order)
        N, g = N[:P, :P].copy(), g[:P].copy()
        tr = N[0, 0]
        for i in range(1, P):
            tr = tr + N[i, i]
        for i in range(P):
            N[i, i] = N[i, i] + p["lam"] * tr
        delta = cholesky_solve(N, g)
        if trace is not None and it == 0:
            trace.update(N=N.copy(), g=g.copy(), a=float(a), delta=None if delta is None else list(delta))
        if delta is None:
            return rejected(FLAT, iters, zb)
        delta = list(delta) + [0.0] * (6 - P)
        cx, cy = cx + delta[0], cy + delta[1]
        B00, B01, B10, B11 = B00 + delta[2], B01 + delta[3], B10 + delta[4], B11 + delta[5]
        iters = it + 1
        conv = math.sqrt(delta[0] * delta[0] + delta[1] * delta[1]) < p["eps_shift"]
        if conv or iters >= p["max_iter"]:
            final, maxiter = True, not conv
        it += 1
    dx, dy = cx - cs[0], cy - cs[1]
    shift = math.sqrt(dx * dx + dy * dy)
    ratio = (B00 * B11 - B01 * B10) / detB0
    q = math.sqrt(ratio) if ratio >= 0 else float("nan")
    lo = 1.0 / p["max_scale_change"]
    if not shift <= p["max_shift"] or not (q >= lo and q <= p["max_scale_change"]):
        return rejected(DIVERGED, iters, zb, za)
    if not za >= p["min_zncc"]:
        return rejected(LOW_ZNCC, iters, zb, za)
    p00, p01 = B00 * Mt[0] + B01 * Mt[2], B00 * Mt[1] + B01 * Mt[3]
    p10, p11 = B10 * Mt[0] + B11 * Mt[2], B10 * Mt[1] + B11 * Mt[3]
    sc = math.sqrt(abs(p00 * p11 - p01 * p10))
    o = 0 if swapped else 7
    out = f.copy()
    out[o:o + 7] = [cx, cy, p00 / sc, p01 / sc, p10 / sc, p11 / sc, sc]
    return out, (MAXITER if maxiter else OK), iters, zb, za


def refine(img1, img2, laf, par=None, order="forward"):
    """the whole list: (laf_out[n][14], u6[n][6], status[n], iterations[n], zncc_before[n], zncc_after[n])"""
    laf = np.asarray(laf, np.float64).reshape(-1, 14)
    n = len(laf)
    out, st, it = np.zeros((n, 14)), np.zeros(n, np.int32), np.zeros(n, np.int32)
    zb, za = np.zeros(n), np.zeros(n)
    for i in range(n):
        out[i], st[i], it[i], zb[i], za[i] = refine_row(img1, img2, laf[i], par, order)
    return out, u6_of(out), st, it, zb, za


def u6_of(laf):
    laf = np.asarray(laf, np.float64).reshape(-1, 14)
    one = np.ones(len(laf))
    return np.stack([laf[:, 0], laf[:, 1], one, laf[:, 7], laf[:, 8], one], axis=1)


def affine_of(row):
    """M2 M1^-1 of a row as a 2 x 2 array"""
    f = np.asarray(row, np.float64)
    M1 = f[6] * f[2:6].reshape(2, 2)
    M2 = f[13] * f[9:13].reshape(2, 2)
    return M2 @ np.linalg.inv(M1)
