"""numpy restatement of the drawing contract (include/mods_hip.h, "match and region images"): integers for the rasteriser, fp64
with one rounding per operation for the contours and the composition of DrawMatches' two images.  A canvas is a uint8 array
[h][w][3], R G B; an element list is an array of ELEM; a colour is 0xRRGGBB."""
import math

import numpy as np

ELEM = np.dtype([("kind", "i4"), ("ax", "i4"), ("ay", "i4"), ("bx", "i4"), ("by", "i4"), ("t", "i4"), ("rgb", "u4"), ("group", "i4")])
NONE, DISC, LINE, SEG = -1, 0, 1, 2
TABLE_REGIONS, TABLE_MATCHES = 0, 1
COORD_MAX, SEG_MAX, SAT, SEP = 32767, 2047, 40000, 20
COLOUR1, COLOUR2, COLOUR_EPI, COLOUR_REGIONS = 0x0000FF, 0x00FF00, 0x00FFFF, 0xA0FFFF
N_SEGS = 21


def elems(rows):
    """an element list from tuples (kind, ax, ay, bx, by, t, rgb, group)"""
    out = np.zeros(len(rows), ELEM)
    for i, r in enumerate(rows):
        out[i] = tuple(r)
    return out


def disc(cx, cy, r, rgb):
    return (DISC, cx, cy, 0, 0, r, rgb, 0)


def line(ax, ay, bx, by, rgb):
    return (LINE, ax, ay, bx, by, 0, rgb, 0)


def seg(ax, ay, bx, by, t, rgb, group):
    return (SEG, ax, ay, bx, by, t, rgb, group)


def _rgb(c):
    return np.array([(c >> 16) & 255, (c >> 8) & 255, c & 255], np.int64)


def _in_range(*v):
    return all(-COORD_MAX <= int(a) <= COORD_MAX for a in v)


def line_pixels(ax, ay, bx, by):
    """the pixels of LINE a -> b in major order, as a list of (x, y)"""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    xmajor = abs(bx - ax) >= abs(by - ay)
    am, an, bm, bn = (ax, ay, bx, by) if xmajor else (ay, ax, by, bx)
    if bm < am:
        am, an, bm, bn = bm, bn, am, an
    D, dn = bm - am, bn - an
    out = []
    for m in range(am, bm + 1):
        n = an if D == 0 else an + (2 * (m - am) * dn + D) // (2 * D)      # Python's // is the floor division
        out.append((m, n) if xmajor else (n, m))
    return out


def seg_masks(e, x0, x1, y0, y1):
    """[y1 - y0 + 1][x1 - x0 + 1] uint16: the subsamples of the pixels of the box inside the capsule, bit 4 j + i"""
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    Ax, Ay, Bx, By = (8 * int(e[k]) for k in ("ax", "ay", "bx", "by"))
    dx, dy = Bx - Ax, By - Ay
    L2 = dx * dx + dy * dy
    h2 = (4 * int(e["t"])) ** 2
    bit = np.arange(16, dtype=np.int64)[:, None, None]                 # subsample 4 j + i, all sixteen at once
    px, py = 8 * xs[None] + (2 * (bit % 4) - 3), 8 * ys[None] + (2 * (bit // 4) - 3)
    wx, wy = px - Ax, py - Ay
    s = wx * dx + wy * dy
    cap_a = wx * wx + wy * wy <= h2
    cap_b = (px - Bx) ** 2 + (py - By) ** 2 <= h2
    cr = wx * dy - wy * dx
    body = cr * cr <= h2 * L2
    inside = np.where((L2 == 0) | (s <= 0), cap_a, np.where(s >= L2, cap_b, body))
    return (inside.astype(np.int64) << bit).sum(axis=0).astype(np.uint16)


_POP = np.array([bin(v).count("1") for v in range(1 << 16)], np.int64)


def _runs(el):
    """(begin, end) of every element or polyline, in order"""
    i, n = 0, len(el)
    while i < n:
        j = i + 1
        if el[i]["kind"] == SEG:
            while j < n and el[j]["kind"] == SEG and el[j]["group"] == el[i]["group"] and el[j]["rgb"] == el[i]["rgb"]:
                j += 1
        yield i, j
        i = j


def _seg_ok(e):
    return (_in_range(e["ax"], e["ay"], e["bx"], e["by"]) and abs(int(e["bx"]) - int(e["ax"])) <= SEG_MAX
            and abs(int(e["by"]) - int(e["ay"])) <= SEG_MAX)


def draw(canvas, el):
    """draws the list onto the canvas in place; returns n_dropped"""
    h, w = canvas.shape[:2]
    dropped = 0
    for i, j in _runs(el):
        e = el[i]
        kind = int(e["kind"])
        if kind == NONE:
            continue
        col = _rgb(int(e["rgb"]))
        if kind == DISC:
            if not _in_range(e["ax"], e["ay"]):
                dropped += 1
                continue
            cx, cy, r = int(e["ax"]), int(e["ay"]), int(e["t"])
            x0, x1, y0, y1 = max(cx - r, 0), min(cx + r, w - 1), max(cy - r, 0), min(cy + r, h - 1)
            if x0 > x1 or y0 > y1:
                continue
            ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
            canvas[y0:y1 + 1, x0:x1 + 1][(xs - cx) ** 2 + (ys - cy) ** 2 <= r * r] = col
        elif kind == LINE:
            if not _in_range(e["ax"], e["ay"], e["bx"], e["by"]):
                dropped += 1
                continue
            for x, y in line_pixels(e["ax"], e["ay"], e["bx"], e["by"]):
                if 0 <= x < w and 0 <= y < h:
                    canvas[y, x] = col
        elif kind == SEG:
            if not all(_seg_ok(el[k]) for k in range(i, j)):
                dropped += j - i
                continue
            boxes = []
            for k in range(i, j):
                s = el[k]
                m = (int(s["t"]) + 1) // 2 + 1          # beyond this margin of its box no subsample is inside
                x0, x1 = max(min(int(s["ax"]), int(s["bx"])) - m, 0), min(max(int(s["ax"]), int(s["bx"])) + m, w - 1)
                y0, y1 = max(min(int(s["ay"]), int(s["by"])) - m, 0), min(max(int(s["ay"]), int(s["by"])) + m, h - 1)
                if x0 <= x1 and y0 <= y1:
                    boxes.append((k, x0, x1, y0, y1))
            if not boxes:
                continue
            X0, X1 = min(b[1] for b in boxes), max(b[2] for b in boxes)
            Y0, Y1 = min(b[3] for b in boxes), max(b[4] for b in boxes)
            mask = np.zeros((Y1 - Y0 + 1, X1 - X0 + 1), np.uint16)        # the polyline's subsamples, over the union of the boxes
            for k, x0, x1, y0, y1 in boxes:
                mask[y0 - Y0:y1 - Y0 + 1, x0 - X0:x1 - X0 + 1] |= seg_masks(el[k], x0, x1, y0, y1)
            c = _POP[mask][:, :, None]
            part = canvas[Y0:Y1 + 1, X0:X1 + 1]
            part[:] = ((part.astype(np.int64) * (16 - c) + col[None, None, :] * c + 8) >> 4).astype(np.uint8)
        else:
            raise ValueError("kind %d" % kind)
    return dropped


def white(w, h):
    return np.full((h, w, 3), 255, np.uint8)


def blit(canvas, img, x0, y0):
    """an 8-bit image [h][w] or [h][w][3] with its corner at (x0, y0), clipped"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    h, w = canvas.shape[:2]
    sh, sw = img.shape[:2]
    xa, xb, ya, yb = max(x0, 0), min(x0 + sw, w), max(y0, 0), min(y0 + sh, h)
    if xa < xb and ya < yb:
        canvas[ya:yb, xa:xb] = img[ya - y0:yb - y0, xa - x0:xb - x0]


def f32_to_u8(img):
    v = np.asarray(img, np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.rint(np.minimum(np.maximum(v, np.float32(0)), np.float32(255))).astype(np.uint8)


# ---- contours ------------------------------------------------------------------------------------------------------

def tables(table):
    C = [math.cos(l * math.pi / 10) for l in range(22)]
    S = [math.sin(l * math.pi / 10) for l in range(22)]
    if table == TABLE_MATCHES:
        C[21] = S[21] = 0.0
    return C, S


def sat(v):
    """(int)v and floor(v) of the composition: NaN and what lies outside [-40000, 40000] become 40000"""
    v = float(v)
    return int(v) if -SAT <= v <= SAT else SAT


def _floor(v):
    return math.floor(v) if math.isfinite(v) else v


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def contour_points(x, y, a11, a12, a21, a22, s, dx, dy, table):
    C, S = tables(table)
    s3 = 3.0 * float(s)
    A11, A12, A21, A22 = s3 * float(a11), s3 * float(a12), s3 * float(a21), s3 * float(a22)
    px, py = [], []
    for k in range(22):
        px.append(_floor(((A11 * C[k] + A12 * S[k]) + float(x)) + float(dx)))
        py.append(_floor(((A21 * C[k] + A22 * S[k]) + float(y)) + float(dy)))
    return px, py


def regions_elems(reg, dx, dy, thickness, rgb, table):
    """the list mods_canvas_regions_elems returns for the regions `reg`, and its n_dropped"""
    out = np.zeros(N_SEGS * len(reg), ELEM)
    dropped = 0
    for i, r in enumerate(reg):
        px, py = contour_points(r["x"], r["y"], r["a11"], r["a12"], r["a21"], r["a22"], r["s"], dx, dy, table)
        ok = all(-COORD_MAX <= v <= COORD_MAX for v in px + py)       # NaN fails
        if ok:
            px, py = [int(v) for v in px], [int(v) for v in py]
            ok = all(abs(px[k + 1] - px[k]) <= SEG_MAX and abs(py[k + 1] - py[k]) <= SEG_MAX for k in range(N_SEGS))
        for k in range(N_SEGS):
            out[N_SEGS * i + k] = (SEG, px[k], py[k], px[k + 1], py[k + 1], thickness, rgb, i) if ok else (NONE, 0, 0, 0, 0, thickness, rgb, i)
        dropped += 0 if ok else N_SEGS
    return out, dropped


# ---- DrawMatches ---------------------------------------------------------------------------------------------------

def invert3(H):
    H = [float(v) for v in np.asarray(H, np.float64).reshape(9)]
    d = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6])
    r = 1.0 / d
    return [(H[4] * H[8] - H[5] * H[7]) * r, (H[2] * H[7] - H[1] * H[8]) * r, (H[1] * H[5] - H[2] * H[4]) * r,
            (H[5] * H[6] - H[3] * H[8]) * r, (H[0] * H[8] - H[2] * H[6]) * r, (H[2] * H[3] - H[0] * H[5]) * r,
            (H[3] * H[7] - H[4] * H[6]) * r, (H[1] * H[6] - H[0] * H[7]) * r, (H[0] * H[4] - H[1] * H[3]) * r]


class _List:
    def __init__(self):
        self.rows, self.group = [], 0

    def polyline(self, px, py, t, rgb):
        for k in range(N_SEGS):
            self.rows.append(seg(px[k], py[k], px[k + 1], py[k + 1], t, rgb, self.group))
        self.group += 1


def _plain(l, f, dx, dy, t, rgb):
    px, py = contour_points(f[0], f[1], f[2], f[3], f[4], f[5], f[6], dx, dy, TABLE_MATCHES)
    l.polyline([sat(v) for v in px], [sat(v) for v in py], t, rgb)


def _through(l, G, f, t, rgb):
    C, S = tables(TABLE_MATCHES)
    f = [float(v) for v in f]
    s3 = 3.0 * f[6]
    B = [s3 * f[2], s3 * f[3], f[0], s3 * f[4], s3 * f[5], f[1], 0.0, 0.0, 1.0]
    P = [(G[3 * r] * B[c] + G[3 * r + 1] * B[3 + c]) + G[3 * r + 2] * B[6 + c] for r in range(3) for c in range(3)]
    px, py = [], []
    for k in range(22):
        X = [(P[3 * r] * C[k] + P[3 * r + 1] * S[k]) + P[3 * r + 2] * 1.0 for r in range(3)]
        px.append(sat(_floor(_div(X[0], X[2]))))
        py.append(sat(_floor(_div(X[1], X[2]))))
    l.polyline(px, py, t, rgb)


def _project(G, x, y):
    den = (G[6] * x + G[7] * y) + G[8]
    return _div((G[0] * x + G[1] * y) + G[2], den), _div((G[3] * x + G[4] * y) + G[5], den)


def epipolar_kb(G, px, py):
    l = [(px * G[j] + py * G[3 + j]) + G[6 + j] for j in range(3)]
    xc = _div(-l[2], l[0])
    b = _div(-l[2], l[1])
    with np.errstate(all="ignore"):
        k = _div(np.float64(0.0) - np.float64(b), np.float64(xc) - np.float64(0.0))
    return k, b


def _clipped(l, ax, ay, bx, by, rx, ry, rw, rh, rgb):
    if not _in_range(ax, ay, bx, by):
        l.rows.append(line(ax, ay, bx, by, rgb))
        return
    inside = [(x, y) for x, y in line_pixels(ax, ay, bx, by) if rx <= x < rx + rw and ry <= y < ry + rh]
    if inside:
        l.rows.append(line(inside[0][0], inside[0][1], inside[-1][0], inside[-1][1], rgb))


def _mul_add(k, w, b):
    with np.errstate(all="ignore"):
        return float(np.float64(k) * np.float64(w) + np.float64(b))


def matches_elems(which, w1, h1, w2, h2, laf14, M, centers_only=0, reproject=0, epipolar=0, r1=5, r2=4):
    """the element list of image `which` (0, 1) of mods_draw_matches"""
    laf = np.asarray(laf14, np.float64).reshape(-1, 14)
    M = [float(v) for v in np.asarray(M, np.float64).reshape(9)]
    l = _List()
    if reproject:
        G = invert3(M) if which == 0 else M
        own, other = (0, 7) if which == 0 else (7, 0)
        if not centers_only:
            for f in laf:
                _plain(l, f[own:own + 7], 0, 0, r1, COLOUR1)
                _through(l, G, f[other:other + 7], r2, COLOUR2)
        for f in laf:
            cx, cy = sat(f[own]), sat(f[own + 1])
            xa, ya = _project(G, float(f[other]), float(f[other + 1]))
            l.rows += [disc(cx, cy, r1 + 2, COLOUR1), disc(sat(xa), sat(ya), r2, COLOUR2), line(sat(xa), sat(ya), cx, cy, COLOUR2)]
        return elems(l.rows)
    ox, oy = (w1 + SEP, 0) if which == 0 else (0, h1 + SEP)
    if not centers_only:
        for f in laf:
            _plain(l, f[0:7], 0, 0, r1, COLOUR2)
            _plain(l, f[7:14], ox, oy, r2, COLOUR2)
    Mt = [M[3 * c + r] for r in range(3) for c in range(3)]
    for f in laf:
        f = [float(v) for v in f]
        cx, cy = sat(f[0]), sat(f[1])
        xa, ya = sat(float(ox) + f[7]), sat(float(oy) + f[8])
        l.rows += [disc(cx, cy, r1 + 2, COLOUR1), disc(xa, ya, r1 + 2, COLOUR1)]
        if epipolar:
            k, b = epipolar_kb(M, f[7], f[8])
            k2, b2 = epipolar_kb(Mt, f[0], f[1])
            _clipped(l, 0, sat(b), w1, sat(_mul_add(k, w1, b)), 0, 0, w1, h1, COLOUR_EPI)
            _clipped(l, ox, sat(b2) + oy, ox + w2, sat(_mul_add(k2, w2, b2)) + oy, ox, oy, w2, h2, COLOUR_EPI)
        l.rows.append(line(xa, ya, cx, cy, COLOUR2))
    return elems(l.rows)


def draw_matches(img1, img2, laf14, M, centers_only=0, reproject=0, epipolar=0, r1=5, r2=4):
    """(out1, out2, [n_dropped1, n_dropped2]) of mods_draw_matches for two 8-bit images ([h][w] or [h][w][3])"""
    h1, w1 = img1.shape[:2]
    h2, w2 = img2.shape[:2]
    outs, dropped = [], []
    for which in (0, 1):
        if reproject:
            cv = np.zeros(((h1, h2)[which], (w1, w2)[which], 3), np.uint8)
            blit(cv, (img1, img2)[which], 0, 0)
        else:
            cv = white(w1 + w2 + SEP, max(h1, h2)) if which == 0 else white(max(w1, w2), h1 + h2 + SEP)
            blit(cv, img1, 0, 0)
            blit(cv, img2, w1 + SEP if which == 0 else 0, 0 if which == 0 else h1 + SEP)
        el = matches_elems(which, w1, h1, w2, h2, laf14, M, centers_only, reproject, epipolar, r1, r2)
        dropped.append(draw(cv, el))
        outs.append(cv)
    return outs[0], outs[1], dropped
