"""numpy restatement of the match propagation contract (include/mods_hip.h: mods_propagate_matches) - the reference of
tests/test_cpu_propagate.py and tests/test_gpu_propagate.py.  float64 in the order the contract writes its operations; every LSM
step is lsm_ref.refine_row, so `order` ("forward" / "reverse": the order of the window sums) is the one thing left open, and the
difference between the two runs is the yardstick the kernels are held to.  It never calls the library."""
import math

import numpy as np

import lsm_ref as L

OFF_MODEL = 7
STATUS_COUNT = 8
STATUS_NAMES = L.STATUS_NAMES + ("OFF_MODEL",)
NOKEY = (1 << 64) - 1
FREE, OCCUPIED, CLOSED = 0, 1, 2
DEFAULTS = dict(cell=4, reach=1, rounds=8, model_type=-1, model=None, model_thr=2.0)


def params(**kw):
    """the defaults of mods_propagate_defaults with fields replaced; a field of the LSM parameters goes to the nested set"""
    p = dict(DEFAULTS)
    p["lsm"] = L.params(radius=5)
    for k, v in kw.items():
        if k in p:
            p[k] = v
        elif k in p["lsm"]:
            p["lsm"][k] = v
        else:
            raise TypeError("no parameter %r" % k)
    return p


def lattice(w1, h1, cell):
    return w1 // cell, h1 // cell


def centre(g, cell):
    return float(g * cell) + float(cell - 1) * 0.5


def own_cell(row, cell):
    return int(math.floor(row[0] / float(cell))), int(math.floor(row[1] / float(cell)))


def propose(front_rows, front_cells, state, cell, reach):
    """one proposal pass: key[Gy][Gx] (uint64, NOKEY: not proposed), winner[Gy][Gx] (-1: not proposed).  front_cells[k] = (gx, gy)
    or None for a row that does not propagate"""
    Gy, Gx = state.shape
    key = np.full((Gy, Gx), NOKEY, np.uint64)
    for k, (row, c) in enumerate(zip(front_rows, front_cells)):
        if c is None:
            continue
        for oy in range(-reach, reach + 1):
            for ox in range(-reach, reach + 1):
                gx, gy = c[0] + ox, c[1] + oy
                if gx < 0 or gy < 0 or gx >= Gx or gy >= Gy or state[gy, gx] != FREE:
                    continue
                dx, dy = centre(gx, cell) - float(row[0]), centre(gy, cell) - float(row[1])
                d2 = np.float32(dx * dx + dy * dy)
                kk = (int(d2.view(np.uint32)) << 32) | k
                if kk < int(key[gy, gx]):
                    key[gy, gx] = kk
    winner = np.where(key == NOKEY, -1, (key & np.uint64(0xffffffff)).astype(np.int64)).astype(np.int32)
    return key, winner


def candidate_row(f, px, py):
    """the candidate at the cell centre (px, py) predicted by the winner's output row f"""
    f = np.asarray(f, np.float64)
    with np.errstate(all="ignore"):
        m00, m01, m10, m11 = f[6] * f[2], f[6] * f[3], f[6] * f[4], f[6] * f[5]
        n00, n01, n10, n11 = f[13] * f[9], f[13] * f[10], f[13] * f[11], f[13] * f[12]
        d1 = m00 * m11 - m01 * m10
        i00, i01, i10, i11 = m11 / d1, (-m01) / d1, (-m10) / d1, m00 / d1
        b00, b01 = n00 * i00 + n01 * i10, n00 * i01 + n01 * i11
        b10, b11 = n10 * i00 + n11 * i10, n10 * i01 + n11 * i11
        dB = b00 * b11 - b01 * b10
        s = np.sqrt(dB)
        dx, dy = np.float64(px) - f[0], np.float64(py) - f[1]
        qx, qy = f[7] + (b00 * dx + b01 * dy), f[8] + (b10 * dx + b11 * dy)
        return np.array([px, py, 1.0, 0.0, 0.0, 1.0, 1.0, qx, qy, b00 / s, b01 / s, b10 / s, b11 / s, s], np.float64)


def candidates(key, front_rows, cell):
    """the candidate list of a proposal pass: (cell index gy Gx + gx, winner k, row) in raster order"""
    Gy, Gx = key.shape
    out = []
    for idx in np.nonzero(key.reshape(-1) != NOKEY)[0]:
        k = int(key.reshape(-1)[idx]) & 0xffffffff
        out.append((int(idx), k, candidate_row(front_rows[k], centre(int(idx) % Gx, cell), centre(int(idx) // Gx, cell))))
    return out


def model_d2(model_type, m, x1, y1, x2, y2):
    """the squared distance the gate compares with model_thr^2; None: the test fails whatever the threshold"""
    m = [float(v) for v in np.asarray(m, np.float64).reshape(9)]
    x1, y1, x2, y2 = float(x1), float(y1), float(x2), float(y2)
    if model_type == 0:
        X, Y, W = (m[0] * x1 + m[1] * y1) + m[2], (m[3] * x1 + m[4] * y1) + m[5], (m[6] * x1 + m[7] * y1) + m[8]
        if not math.isfinite(W) or W == 0.0:
            return None
        ex, ey = X / W - x2, Y / W - y2
        return ex * ex + ey * ey
    l0, l1, l2 = (m[0] * x1 + m[3] * y1) + m[6], (m[1] * x1 + m[4] * y1) + m[7], (m[2] * x1 + m[5] * y1) + m[8]
    m0, m1 = (m[0] * x2 + m[1] * y2) + m[2], (m[3] * x2 + m[4] * y2) + m[5]
    e = (l0 * x2 + l1 * y2) + l2
    den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
    if den == 0.0:
        return None
    return (e * e) / den


def propagate(img1, img2, seeds, par=None, max_out=None, order="forward"):
    """the whole call.  Returns a dict with the keys of Context.propagate_matches, and "tried": one dict per candidate row ever
    registered (round, cell, parent, row_in, row_out, status, lsm_status, iterations, zncc_before, zncc_after, d2) in the order
    they were tried"""
    p = par if par is not None else params()
    seeds = np.asarray(seeds, np.float64).reshape(-1, 14)
    n = len(seeds)
    cell, reach, rounds = int(p["cell"]), int(p["reach"]), int(p["rounds"])
    h1, w1 = img1.shape
    Gx, Gy = lattice(w1, h1, cell)
    cap = Gx * Gy if max_out is None else int(max_out)
    state = np.zeros((Gy, Gx), np.uint8)
    stats = np.zeros((rounds + 1, STATUS_COUNT), np.int32)
    tried_status, tried_iters = np.full((Gy, Gx), -1, np.int32), np.full((Gy, Gx), -1, np.int32)
    seed_status = np.zeros(n, np.int32)
    front = []                                  # (output row, own cell, index in the combined list)
    for k in range(n):
        row, st, _, _, _ = L.refine_row(img1, img2, seeds[k], p["lsm"], order)
        seed_status[k] = st
        stats[0, st] += 1
        if st == L.OK:
            c = own_cell(row, cell)
            if 0 <= c[0] < Gx and 0 <= c[1] < Gy:
                state[c[1], c[0]] = OCCUPIED
            front.append((row, c, k))
    out = dict(laf=[], zncc=[], iterations=[], round=[], cell=[], parent=[])
    tried = []
    truncated = False
    thr2 = float(p["model_thr"]) * float(p["model_thr"])
    for r in range(1, rounds + 1):
        rows = [f[0] for f in front]
        key, _ = propose(rows, [f[1] for f in front], state, cell, reach)
        cands = candidates(key, rows, cell)
        if not cands:
            break
        accepted = []
        for idx, k, row_in in cands:
            row, st, it, zb, za = L.refine_row(img1, img2, row_in, p["lsm"], order)
            lsm_st, d2 = st, None
            if st == L.OK and p["model_type"] >= 0:
                d2 = model_d2(p["model_type"], p["model"], row[0], row[1], row[7], row[8])
                if d2 is None or not d2 <= thr2:
                    st = OFF_MODEL
            gx, gy = idx % Gx, idx // Gx
            state[gy, gx] = OCCUPIED if st == L.OK else CLOSED
            tried_status[gy, gx], tried_iters[gy, gx] = st, it
            stats[r, st] += 1
            tried.append(dict(round=r, cell=(gx, gy), parent=front[k][2], row_in=row_in, row_out=row, status=st, lsm_status=lsm_st,
                              iterations=it, zncc_before=zb, zncc_after=za, d2=d2))
            if st == L.OK:
                accepted.append((row, (gx, gy), za, it, front[k][2]))
        front = []
        for row, c, za, it, parent in accepted:
            if len(out["laf"]) >= cap:
                truncated = True
                break
            front.append((row, c, n + len(out["laf"])))
            out["laf"].append(row); out["zncc"].append(za); out["iterations"].append(it); out["round"].append(r)
            out["cell"].append(c); out["parent"].append(parent)
        if truncated:
            break
    m = len(out["laf"])
    laf = np.array(out["laf"], np.float64).reshape(m, 14)
    return {"laf": laf, "u6": L.u6_of(laf), "zncc": np.array(out["zncc"], np.float64), "iterations": np.array(out["iterations"], np.int32),
            "round": np.array(out["round"], np.int32), "cell": np.array(out["cell"], np.int32).reshape(m, 2),
            "parent": np.array(out["parent"], np.int32), "truncated": truncated, "seed_status": seed_status, "stats": stats,
            "tried_status": tried_status, "tried_iterations": tried_iters, "tried": tried}


def margins(img1, img2, res, par, rel=1e-6):
    """the deciding quantities of a run's tried rows against their thresholds: the rows that lie within `rel` (absolute for the
    zncc, relative for the shift, the scale change and the model's d2) of a threshold, as (round, cell, what) - an input of the
    GPU tests has none.  OK rows: from their rows in and out.  DIVERGED / LOW_ZNCC rows: the status must survive all four
    thresholds tightened and loosened by `rel` (they are read only at the end of the LSM contract)"""
    lsm = par["lsm"]
    near = []
    thr2 = float(par["model_thr"]) ** 2
    for t in res["tried"]:
        tag = (t["round"], t["cell"])
        st = t["lsm_status"]
        if st in (L.OK, L.MAXITER):
            if abs(t["zncc_after"] - lsm["min_zncc"]) <= rel:
                near.append(tag + ("zncc",))
            swapped = L.roles(t["row_in"])[0]
            o = 0 if swapped else 7
            shift = math.hypot(*(t["row_out"][o:o + 2] - t["row_in"][o:o + 2]))
            if abs(shift - lsm["max_shift"]) <= rel * lsm["max_shift"]:
                near.append(tag + ("shift",))
            B0, B1 = L.affine_of(t["row_in"]), L.affine_of(t["row_out"])
            q = math.sqrt(abs(np.linalg.det(B1) / np.linalg.det(B0)))
            q = 1.0 / q if swapped else q
            for lim in (lsm["max_scale_change"], 1.0 / lsm["max_scale_change"]):
                if abs(q - lim) <= rel * lim:
                    near.append(tag + ("scale",))
            if t["d2"] is not None and abs(t["d2"] - thr2) <= rel * thr2:
                near.append(tag + ("model",))
        elif st in (L.DIVERGED, L.LOW_ZNCC):
            for sgn in (-1.0, 1.0):
                q = dict(lsm)
                q["max_shift"] = lsm["max_shift"] * (1 + sgn * rel)
                q["max_scale_change"] = max(1.0, lsm["max_scale_change"] * (1 + sgn * rel))
                q["min_zncc"] = lsm["min_zncc"] - sgn * rel
                if L.refine_row(img1, img2, t["row_in"], q)[1] != st:
                    near.append(tag + ("perturbed",))
    return near
