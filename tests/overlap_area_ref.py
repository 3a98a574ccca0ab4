"""numpy restatement of the area-overlap contract (include/mods_hip.h: mods_match_overlap_area) - the reference of
tests/test_cpu_overlap_area.py and tests/test_gpu_overlap_area.py.  float64, one numpy operation per rounding in the order the
contract writes them; it never calls the library.  The gates of the n_q x n_t pairs are formed in blocks of query rows; the lattice of
an evaluated pair (at most 513 x 513 points) is one numpy grid."""
from types import SimpleNamespace

import numpy as np

from overlap_ref import CHUNK, _f, common_masks, query_records

AREA_DTYPE = np.dtype([("q", "i4"), ("t", "i4"), ("E", "f8"), ("n_q_px", "i4"), ("n_t_px", "i4"), ("n_both", "i4"), ("pad", "i4")])
CAP = 256.0


def params(H, max_error=0.4, one_to_one=2, w1=0, h1=0, w2=0, h2=0):
    """the fields of mods_overlap_area_params; the functions below take this or the package's OverlapAreaParams"""
    return SimpleNamespace(H=[float(v) for v in np.asarray(H, np.float64).reshape(9)], max_error=float(max_error),
                           one_to_one=int(one_to_one), w1=int(w1), h1=int(h1), w2=int(w2), h2=int(h2))


def train_records(t):
    """x2, y2, M11, M12, M21, M22 of the contract"""
    with np.errstate(all="ignore"):
        ks = 3.0 * _f(t, "s")
        return _f(t, "x"), _f(t, "y"), ks * _f(t, "a11"), ks * _f(t, "a12"), ks * _f(t, "a21"), ks * _f(t, "a22")


def _min(a, b):
    return np.where(a < b, a, b)          # a < b ? a : b, as the contract defines min (NaN in a: b)


def _max(a, b):
    return np.where(a > b, a, b)


def _setup(qr, tr, max_error):
    """the set-up of the pairs qr x tr (broadcast) and which of them are evaluated"""
    px, py, C11, C12, C21, C22 = qr
    x2, y2, M11, M12, M21, M22 = tr
    with np.errstate(all="ignore"):
        detC = C11 * C22 - C12 * C21
        f = 30.0 / np.sqrt(np.fabs(detC))
        Q11 = f * C11; Q12 = f * C12; Q21 = f * C21; Q22 = f * C22
        T11 = f * M11; T12 = f * M12; T21 = f * M21; T22 = f * M22
        dx = f * (px - x2); dy = f * (py - y2)
        qex = np.sqrt(Q11 * Q11 + Q12 * Q12); qey = np.sqrt(Q21 * Q21 + Q22 * Q22)
        tex = np.sqrt(T11 * T11 + T12 * T12); tey = np.sqrt(T21 * T21 + T22 * T22)
        at = np.fabs(T11 * T22 - T12 * T21)
        g = 0.9 * (1.0 - max_error)
        x0 = np.floor(_min(dx - qex, -tex)); x1 = np.ceil(_max(dx + qex, tex))
        y0 = np.floor(_min(dy - qey, -tey)); y1 = np.ceil(_max(dy + qey, tey))
        ev = (at >= g * 900.0) & (900.0 >= g * at) & (np.fabs(dx) <= qex + tex) & (np.fabs(dy) <= qey + tey)
        ev = ev & (-x0 <= CAP) & (x1 <= CAP) & (-y0 <= CAP) & (y1 <= CAP)
    Q = tuple(np.broadcast_to(m, ev.shape) for m in (Q11, Q12, Q21, Q22))
    return SimpleNamespace(Q=Q, T=(T11, T12, T21, T22), dx=dx, dy=dy, box=(x0, x1, y0, y1), ev=ev)


def _inverse(m11, m12, m21, m22):
    with np.errstate(all="ignore"):
        d = 1.0 / (m11 * m22 - m12 * m21)
        return m22 * d, -(m12 * d), -(m21 * d), m11 * d


def lattice(Q, T, dx, dy, box):
    """(n_q_px, n_t_px, n_both) of one evaluated pair: scalars in, python ints out"""
    QI11, QI12, QI21, QI22 = _inverse(*[np.float64(v) for v in Q])
    TI11, TI12, TI21, TI22 = _inverse(*[np.float64(v) for v in T])
    x0, x1, y0, y1 = (int(v) for v in box)
    X = np.arange(x0, x1 + 1, dtype=np.float64)[None, :]
    Y = np.arange(y0, y1 + 1, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        a = X - dx; b = Y - dy
        u = QI11 * a + QI12 * b; v = QI21 * a + QI22 * b
        inQ = u * u + v * v <= 1.0
        u2 = TI11 * X + TI12 * Y; v2 = TI21 * X + TI22 * Y
        inT = u2 * u2 + v2 * v2 <= 1.0
    return int(inQ.sum()), int(inT.sum()), int((inQ & inT).sum())


def pair_error(n_q_px, n_t_px, n_both):
    """E of the contract; None when the union is empty"""
    uni = n_q_px + n_t_px - n_both
    return None if uni == 0 else 1.0 - float(n_both) / float(uni)


def evaluated_pairs(q, t, p):
    """every evaluated pair of the lists, in (q, t) order, as AREA_DTYPE rows (E = NaN where the union is empty) - the common area
    included.  The assignment modes share this table"""
    n_q, n_t = len(q), len(t)
    rows = []
    if n_q and n_t:
        mq, mt = common_masks(q, t, p)
        tr = tuple(a[None, :] for a in train_records(t))
        qr = query_records(q, list(p.H))
        for q0 in range(0, n_q, CHUNK):
            q1 = min(n_q, q0 + CHUNK)
            s = _setup(tuple(a[q0:q1, None] for a in qr), tr, p.max_error)
            ev = s.ev & mq[q0:q1, None] & mt[None, :]
            for i, j in zip(*np.nonzero(ev)):
                c = lattice([m[i, j] for m in s.Q], [m[i, j] for m in s.T], s.dx[i, j], s.dy[i, j], [m[i, j] for m in s.box])
                e = pair_error(*c)
                rows.append((q0 + int(i), int(j), np.nan if e is None else e) + c + (0,))
    return np.array(rows, AREA_DTYPE) if rows else np.zeros(0, AREA_DTYPE)


def assign(pairs, max_error, one_to_one):
    """the accepted pairs (E < max_error) through the assignment rule of the mode; AREA_DTYPE rows in query order"""
    with np.errstate(all="ignore"):
        acc = pairs[pairs["E"] < max_error]              # NaN fails
    if one_to_one == 2:
        acc = acc[np.lexsort((acc["t"], acc["q"], acc["E"]))]
        used_q, used_t, keep = set(), set(), []
        for k, (qi, ti) in enumerate(zip(acc["q"].tolist(), acc["t"].tolist())):
            if qi not in used_q and ti not in used_t:
                used_q.add(qi); used_t.add(ti); keep.append(k)
        out = acc[keep]
        return out[np.argsort(out["q"], kind="stable")]
    best = {}
    for k, (qi, ti, e) in enumerate(zip(acc["q"].tolist(), acc["t"].tolist(), acc["E"].tolist())):
        if qi not in best or (e, ti) < best[qi][:2]:
            best[qi] = (e, ti, k)
    picks = [best[qi] for qi in sorted(best)]
    if one_to_one == 1:
        owner = {}
        for (e, ti, k) in picks:
            qi = int(acc["q"][k])
            if ti not in owner or (e, qi) < owner[ti]:
                owner[ti] = (e, qi)
        picks = [pk for pk in picks if owner[pk[1]][1] == int(acc["q"][pk[2]])]
    return acc[[pk[2] for pk in picks]]


def counts_of(q, t, p, n_matches):
    mq, mt = common_masks(q, t, p)
    lo = min(int(mq.sum()), int(mt.sum()))
    return SimpleNamespace(n_q_common=int(mq.sum()), n_t_common=int(mt.sum()), n_matches=int(n_matches),
                           repeatability=(float(n_matches) / float(lo)) if lo > 0 else 0.0)


def overlap_area_ref(q, t, p, pairs=None):
    """returns (matches as AREA_DTYPE rows in query order, counts) of the contract; p: params() or an OverlapAreaParams;
    pairs: evaluated_pairs(q, t, p) when the caller has it already"""
    if pairs is None:
        pairs = evaluated_pairs(q, t, p)
    m = assign(pairs, p.max_error, p.one_to_one)
    return m, counts_of(q, t, p, len(m))


def circle_overlap_error(r, d):
    """1 - |A n B| / |A u B| of two circles of radius r with centres d apart, in closed form"""
    if d >= 2 * r:
        return 1.0
    inter = 2 * r * r * np.arccos(d / (2 * r)) - 0.5 * d * np.sqrt(4 * r * r - d * d)
    return 1.0 - inter / (2 * np.pi * r * r - inter)
