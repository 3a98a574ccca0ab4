"""The homography views of include/mods_hip.h ("homography views") restated in numpy: the perspective warp, the geometry rule,
linH and the post-pass that carries a view's regions back into the original frame.

Coordinates are fp64, the bilinear weights and the pixel sum fp32, every operation rounded once and in the order the header
states them (numpy evaluates one ufunc per operation, so nothing is fused)."""
import math

import numpy as np

INT_MIN, INT_MAX = -2147483648.0, 2147483647.0
K_SIGMA = (2 * 3.0) * math.sqrt(3.0)          # synth-detection.cpp:21


def invert3_adjugate(H):
    """(G, det): adj(H) times the reciprocal of det(H), row-major 9 doubles; G is None when det is 0 or not finite"""
    S = [np.float64(v) for v in np.asarray(H, np.float64).reshape(9)]
    with np.errstate(all="ignore"):
        d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
        if d == 0 or not np.isfinite(d):
            return None, d
        r = np.float64(1.0) / d
        G = [(S[4] * S[8] - S[5] * S[7]) * r, (S[2] * S[7] - S[1] * S[8]) * r, (S[1] * S[5] - S[2] * S[4]) * r,
             (S[5] * S[6] - S[3] * S[8]) * r, (S[0] * S[8] - S[2] * S[6]) * r, (S[2] * S[3] - S[0] * S[5]) * r,
             (S[3] * S[7] - S[4] * S[6]) * r, (S[1] * S[6] - S[0] * S[7]) * r, (S[0] * S[4] - S[1] * S[3]) * r]
    return np.array(G, np.float64), d


def inverse_and_d0(H, w, h):
    """(G, d0) of a w x h source; ValueError where the library answers MODS_E_ARG"""
    Hf = np.asarray(H, np.float64).reshape(9)
    if not np.isfinite(Hf).all():
        raise ValueError("H is not finite")
    G, d = invert3_adjugate(Hf)
    if G is None:
        raise ValueError("singular homography")
    cx, cy = np.float64(w - 1) / 2.0, np.float64(h - 1) / 2.0
    d0 = (Hf[6] * cx + Hf[7] * cy) + Hf[8]
    if d0 == 0 or not np.isfinite(d0):
        raise ValueError("the horizon passes through the centre")
    return G, d0


def warp_perspective(src, H, dw, dh, cval=128.0):
    """src (h x w float32; a strided view is fine) through H (original -> view) into dh x dw"""
    src = np.asarray(src, np.float32)
    sh, sw = src.shape
    G, d0 = inverse_and_d0(H, sw, sh)
    cval = np.float32(cval)
    x = np.arange(dw, dtype=np.float64)[None, :]
    y = np.arange(dh, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        W = (G[6] * x + G[7] * y) + G[8]
        ok = (W * d0) > 0
        t = 32.0 / W
        fX = ((G[0] * x + G[1] * y) + G[2]) * t
        fY = ((G[3] * x + G[4] * y) + G[5]) * t
        ok = ok & ~np.isnan(fX) & ~np.isnan(fY)
        X = np.rint(np.clip(np.where(ok, fX, 0.0), INT_MIN, INT_MAX)).astype(np.int64)
        Y = np.rint(np.clip(np.where(ok, fY, 0.0), INT_MIN, INT_MAX)).astype(np.int64)
    sx, sy = X >> 5, Y >> 5
    fx = (X & 31).astype(np.float32) * np.float32(1.0 / 32)
    fy = (Y & 31).astype(np.float32) * np.float32(1.0 / 32)
    one = np.float32(1.0)
    w0, w1, w2, w3 = (one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
        v = src[np.where(inside, yy, 0), np.where(inside, xx, 0)]
        return np.where(inside, v, cval).astype(np.float32)

    v0, v1, v2, v3 = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    out = ((v0 * w0 + v1 * w1) + v2 * w2) + v3 * w3
    assert out.dtype == np.float32
    return np.where(ok, out, cval).astype(np.float32)


def view_geometry_h(w, h, H, clip_w, clip_h, init_sigma):
    """dict(w_new, h_new, ksize, sigma) of mods_view_geometry_h; ValueError where it answers MODS_E_ARG"""
    if w <= 0 or h <= 0 or clip_w <= 0 or clip_h <= 0:
        raise ValueError("bad arguments")
    Hf = np.asarray(H, np.float64).reshape(9)
    _, d0 = inverse_and_d0(Hf, w, h)
    xs, ys = [], []
    for bx, by in ((0.0, 0.0), (0.0, float(h)), (float(w), 0.0), (float(w), float(h))):
        bx, by = np.float64(bx), np.float64(by)
        den = Hf[6] * bx + Hf[7] * by + Hf[8]
        if not den * d0 > 0:
            raise ValueError("corner on or behind the horizon")
        px, py = (Hf[0] * bx + Hf[1] * by + Hf[2]) / den, (Hf[3] * bx + Hf[4] * by + Hf[5]) / den
        if not (np.isfinite(px) and np.isfinite(py)):
            raise ValueError("corner without a finite image")
        xs.append(math.trunc(min(max(px, -1e9), 1e9)))       # a cv::Point holds ints
        ys.append(math.trunc(min(max(py, -1e9), 1e9)))
    dx, dy = max(min(max(xs), clip_w), 0), max(min(max(ys), clip_h), 0)
    sigma = np.float64(init_sigma) / 4.0
    ks = int(math.floor(2.0 * 4.0 * sigma + 1.0))
    if ks % 2 == 0:
        ks += 1
    ks = max(ks, 3)
    return dict(w_new=int(dx), h_new=int(dy), ksize=ks, sigma=float(sigma))


def lin_h(x, y, G):
    """linH (synth-detection.cpp:1498-1516): the 2 x 2 linearisation (a11, a12, a21, a22) of the projective map G at (x, y);
    x, y may be arrays"""
    with np.errstate(all="ignore"):
        den = (G[6] * x + G[7] * y) + G[8]
        den_sq = den * den
        n1 = ((G[0] * x + G[1] * y) + G[2]) / den_sq
        n2 = ((G[3] * x + G[4] * y) + G[5]) / den_sq
        return G[0] / den - n1 * G[6], G[1] / den - n1 * G[7], G[3] / den - n2 * G[6], G[4] / den - n2 * G[7]


def check_borders(img_w, img_h, x, y, a11, a12, a21, a22, box):
    """interpolateCheckBorders (helpers.cpp:527-549) in fp32 for arrays of regions; box: int array (res_w = res_h)"""
    f = np.float32
    x, y, a11, a12, a21, a22 = (np.asarray(v, np.float64).astype(f) for v in (x, y, a11, a12, a21, a22))
    half = np.ceil(np.asarray(box).astype(f).astype(np.float64) / 2.0).astype(f)
    width, height = img_w - 2, img_h - 2
    touch = np.zeros(len(x), bool)
    with np.errstate(all="ignore"):
        for sxn, syn in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
            xs, ys = f(sxn) * half, f(syn) * half
            imx = (x + xs * a11) + ys * a12
            imy = (y + xs * a21) + ys * a22
            touch |= (np.floor(imx) <= 0) | (np.floor(imy) <= 0) | (np.ceil(imx) >= width) | (np.ceil(imy) >= height)
    return touch


def reproject_regions_h(regs, H, ow, oh, mask=None, half=None):
    """the post-pass: regions of a view (structured array with x y s a11 a12 a21 a22 id ...) -> the survivors in the original
    frame, order kept, id = the new position; `half`: the twin list, filtered by the same flags -> (regions, twins)"""
    import detection_mask_ref
    G, d0 = inverse_and_d0(H, ow, oh)
    out = regs.copy()
    x, y = regs["x"].astype(np.float64), regs["y"].astype(np.float64)
    with np.errstate(all="ignore"):
        den = (G[6] * x + G[7] * y) + G[8]
        front = (den * d0) > 0
        rx = ((G[0] * x + G[1] * y) + G[2]) / den
        ry = ((G[3] * x + G[4] * y) + G[5]) / den
        L0, L1, L2, L3 = lin_h(x, y, G)
        a11 = L0 * regs["a11"] + L1 * regs["a21"]
        a12 = L0 * regs["a12"] + L1 * regs["a22"]
        a21 = L2 * regs["a11"] + L3 * regs["a21"]
        a22 = L2 * regs["a12"] + L3 * regs["a22"]
        box = np.trunc(K_SIGMA * regs["s"]).astype(np.int64)
        keep = front & (rx > 0) & (rx < ow) & (ry > 0) & (ry < oh)
        keep &= ~check_borders(ow, oh, rx, ry, a11, a12, a21, a22, box)
    if mask is not None:
        keep &= detection_mask_ref.on_mask(mask, np.where(keep, rx, -10.0), np.where(keep, ry, -10.0))
    for f, v in (("x", rx), ("y", ry), ("a11", a11), ("a12", a12), ("a21", a21), ("a22", a22)):
        out[f] = v
    out = out[keep]
    out["id"] = np.arange(len(out))
    if half is None:
        return out
    oh_ = half.copy()[keep]
    for f in ("x", "y", "a11", "a12", "a21", "a22", "id"):
        oh_[f] = out[f]
    return out, oh_


def apply_h(H, pts):
    """the images of pts [n][2] under the row-major homography H (plain double arithmetic: for error measures, not for parity)"""
    Hm = np.asarray(H, np.float64).reshape(3, 3)
    p = np.c_[pts, np.ones(len(pts))] @ Hm.T
    return p[:, :2] / p[:, 2:3]
