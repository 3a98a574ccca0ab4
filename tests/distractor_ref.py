"""The distractor-database veto of the FGINN matcher (include/mods_hip.h: mods_ctx_distractor_db, csrc/distractor.hip) restated in
numpy on top of match_ref.py.  Nothing here calls the library.

For a forward tentative (q, t) with d0 = d(q, t) (field d1) and dj the distance it was emitted with (field d2), and a database B of
M >= 1 descriptors: dDB = min_b d(q, b), rDB = quot(d0, dDB), r = quot(d0, dj), r' = (r < rDB) ? rDB : r; the tentative is dropped
when not r' <= ratio^2 and otherwise kept with ratio = sqrt(r'), every other field as the forward search wrote it.  M = 0: nothing
changes."""
import numpy as np

import match_ref as ref

INT_MAX = 2 ** 31 - 1
CHUNK = 256


def min_dist(desc, db):
    """int64 [len(desc)]: the exact squared distance of every descriptor to its nearest database row, INT_MAX for an empty database"""
    desc = np.asarray(desc).reshape(-1, 128)
    out = np.full(len(desc), INT_MAX, np.int64)
    if len(db) == 0:
        return out
    for b in range(0, len(desc), CHUNK):
        for c in range(0, len(db), 1 << 14):
            out[b:b + CHUNK] = np.minimum(out[b:b + CHUNK], ref.sqdist(desc[b:b + CHUNK], db[c:c + (1 << 14)]).min(1))
    return out


def veto(fwd, q, db, ratio=0.8):
    """(kept list with the new ratios, keep mask over fwd, dDB of every forward tentative) for the forward list fwd of queries q"""
    ddb = min_dist(q["desc"][fwd["q"]], db)
    keep = np.ones(len(fwd), bool)
    out = fwd.copy()
    if len(db) == 0:
        return out, keep, ddb
    sq = np.float64(ratio) * np.float64(ratio)
    for i in range(len(fwd)):
        d0 = fwd["d1"][i]
        r = ref.ratio_quotient(d0, fwd["d2"][i])
        rdb = ref.ratio_quotient(d0, np.float32(ddb[i]))
        r2 = rdb if r < rdb else r
        if not r2 <= sq:
            keep[i] = False
        else:
            out["ratio"][i] = np.sqrt(r2)
    return out[keep].copy(), keep, ddb


def match_fginn_db(q, t, db, ratio=0.8, contrad=10.0, nn=50):
    """the vetoed list of a whole search: (kept, forward list, keep mask, dDB of the forward list)"""
    fwd = ref.match_fginn(q, t, ratio, contrad, nn)
    kept, keep, ddb = veto(fwd, q, db, ratio)
    return kept, fwd, keep, ddb


def laf_rows(tent, q, t):
    """the frames (x y a11 a12 a21 a22 s) of both regions of a tentative list, as the emit stage lays them out"""
    f = ("x", "y", "a11", "a12", "a21", "a22", "s")
    a, b = q[tent["q"]], t[tent["t"]]
    return np.stack([a[k] for k in f] + [b[k] for k in f], axis=1).astype(np.float64).reshape(-1, 14)


def four_squares(d):
    """d <= 4 * 255^2 as a sum of four squares of integers <= 255 (Lagrange), largest first"""
    top = int(np.sqrt(d))
    for a in range(min(top, 255), -1, -1):
        ra = d - a * a
        if ra > 3 * a * a:
            break
        for b in range(min(int(np.sqrt(ra)), a), -1, -1):
            rb = ra - b * b
            if rb > 2 * b * b:
                break
            for c in range(min(int(np.sqrt(rb)), b), -1, -1):
                rc = rb - c * c
                if rc > c * c:
                    break
                e = int(np.sqrt(rc))
                if e * e == rc:
                    return a, b, c, e
    raise ValueError("no four squares for %d" % d)


def at_distance(base, d, start=0):
    """a copy of the constant-byte descriptor `base` (bytes 100 .. 155) at squared distance d <= 40000: four bytes from `start` move"""
    out = np.asarray(base, np.int64).copy()
    for n, v in enumerate(four_squares(d)):
        out[start + n] += v if out[start + n] + v <= 255 else -v
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
