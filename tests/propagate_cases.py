"""Inputs of the match propagation tests (tests/test_cpu_propagate.py, tests/test_gpu_propagate.py): the analytic pairs of
tests/lsm_cases.py, a window of their image 1 whose four borders all map inside image 2, seeds and parameter sets.  Pure numpy.
Every case is examined on the CPU (forward and reversed restatement agree, no deciding quantity near its threshold) before the
GPU test uses it."""
import numpy as np

import lsm_cases as K

WIN = (22, 4, 52, 72)           # x0, y0, w, h of the window of image 1 ("up"): neither side a multiple of the cells used on it
WIN_STRIDE = 57
GROUND = dict(cell=4, reach=1, rounds=6)


def affine_h(kind="up", x0=0.0, y0=0.0, shift=(0.0, 0.0)):
    """the true map image 1 -> image 2 as a row-major homography; (x0, y0): the origin of a window of image 1"""
    A, t = K.A_OF[kind], K.T_OF[kind]
    t = t + A @ np.array([x0, y0]) + np.array(shift)
    return np.array([A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1], 0.0, 0.0, 1.0])


def epipolar_f(H, e=(400.0, -250.0, 1.0)):
    """F = [e]x H as the library takes it (model[3 j + i] = F_ij): every pair x2 = H x1 lies on it"""
    ex = np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])
    F = ex @ np.asarray(H, np.float64).reshape(3, 3)
    return (F / np.abs(F).max()).T.reshape(9).copy()


def window_pair():
    """(the window WIN of image 1 of the "up" pair, image 2): strided float32 views"""
    a, b = K.analytic_pair("up")
    x0, y0, w, h = WIN
    return K.strided(np.array(a)[y0:y0 + h, x0:x0 + w], WIN_STRIDE), b


def window_rows(centres, scale=1.0):
    """exact rows of window_pair() at the given centres (window coordinates)"""
    x0, y0 = WIN[:2]
    A, t = K.A_OF["up"], K.T_OF["up"]
    rows = []
    for c in centres:
        c = np.asarray(c, np.float64)
        rows.append(K.frame_row(c, scale * np.eye(2), A @ (c + [x0, y0]) + t, scale * A))
    return np.array(rows)


def window_error(rows):
    """|A x1 + t - x2| of rows of window_pair()"""
    rows = np.asarray(rows, np.float64).reshape(-1, 14)
    p = (rows[:, 0:2] + WIN[:2]) @ K.A_OF["up"].T + K.T_OF["up"]
    return np.hypot(*(p - rows[:, 7:9]).T)


def occluded_pair():
    """the "up" pair with the rectangle OCC of image 2 taken from an unrelated scene"""
    a, b = K.analytic_pair("up")
    b = np.array(b)
    x0, y0, x1, y1 = OCC
    yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float64)
    b[y0:y1, x0:x1] = K.scene(seed=2)(xx + 300.0, yy + 300.0).astype(np.float32)
    return a, K.strided(b, K.STRIDE2)


OCC = (30, 60, 64, 112)         # x0, y0, x1, y1 of image 2


def ground_seeds(kind):
    return K.displaced(K.true_rows(2, 3, kind, spread=20, scale=1), 5, shift=1.0, rel=0.05)


def images_of(name):
    return {"up": lambda: K.analytic_pair("up"), "down": lambda: K.analytic_pair("down"), "window": window_pair,
            "occluded": occluded_pair}[name]()


def cases():
    """(name, images, seeds, parameter overrides, max_out or None): the whole runs of the CPU and the GPU test"""
    up, dn = ground_seeds("up"), ground_seeds("down")
    many = K.displaced(K.true_rows(300, 11, "up", spread=35, scale=1), 12, shift=0.5, rel=0.03)
    bad = np.array([up[0], up[1], up[0]])
    bad[2, 4] = np.nan                                                           # BAD_FRAME
    tie = np.array([K.true_rows(1, 1, "up", scale=1)[0]] * 3)
    for r, c1 in zip(tie, ((41.5, 37.5), (49.5, 37.5), (40.3, 37.2))):           # cells (10, 9), (12, 9) of cell 4; the third shares (10, 9)
        r[:] = K.frame_row(c1, np.eye(2), K.A_OF["up"] @ np.array(c1) + K.T_OF["up"], K.A_OF["up"])
    H = affine_h("up")
    out = [
        ("up", "up", up, dict(GROUND), None),
        ("down", "down", dn, dict(GROUND), None),
        ("one round", "up", up, dict(GROUND, rounds=1), None),
        ("cap", "up", up, dict(GROUND), 30),
        ("cap 0", "up", up, dict(GROUND, rounds=2), 0),
        ("tie", "up", tie, dict(GROUND, rounds=2), None),
        ("bad seeds", "up", bad, dict(GROUND, rounds=2), None),
        ("maxiter seed", "up", np.array([K.true_rows(1, 4, "up", scale=1)[0], up[0]]), dict(GROUND, rounds=2, max_iter=2), None),
        ("big round", "up", many, dict(cell=2, reach=4, rounds=2), None),
        ("borders", "window", window_rows([(26.0, 36.0), (25.2, 35.1)]), dict(cell=5, reach=2, rounds=8), None),
        ("partial", "window", window_rows([(46.5, 30.0), (20.0, 67.5)]), dict(cell=11, reach=1, rounds=2, radius=3), None),
        ("occluded", "occluded", up, dict(GROUND, rounds=10), None),
        ("H gate", "up", up, dict(GROUND, model_type=0, model=H, model_thr=2.0), None),
        ("H gate off", "up", up, dict(GROUND, model_type=0, model=affine_h("up", shift=(5.0, 0.0)), model_thr=2.0), None),
        ("F gate", "up", up, dict(GROUND, model_type=1, model=epipolar_f(H), model_thr=2.0), None),
        ("F gate down", "down", dn, dict(GROUND, model_type=1, model=epipolar_f(affine_h("down")), model_thr=2.0), None),
    ]
    return out


# The yardstick of tests/test_gpu_propagate.py: the restatement run with its window sums forward and reversed differs, over the whole
# runs of cases(), by at most SPREAD in a coordinate, a frame entry or a zncc value (measured on the CPU: 2.13e-14, the "down" pair,
# six rounds deep; one round: 7.1e-15), with equal cells, parents, statuses and iteration counts.  tests/test_cpu_propagate.py holds
# the figure against the restatement.
SPREAD = 2.14e-14


def propose_cases():
    """(name, w1, h1, cell, reach, front rows, front cells or None (the rows' own), state[Gy][Gx]) of the one-pass proposal test"""
    def occupied(rows, w, h, cell, closed=0, seed=0):
        st = np.zeros((h // cell, w // cell), np.uint8)
        for r in rows:
            gx, gy = int(r[0] // cell), int(r[1] // cell)
            if gx < st.shape[1] and gy < st.shape[0]:
                st[gy, gx] = 1
        if closed:
            rng = np.random.default_rng(seed)
            free = np.nonzero(st.reshape(-1) == 0)[0]
            st.reshape(-1)[rng.choice(free, closed, replace=False)] = 2
        return st
    tie = cases()[5][2]
    many = K.true_rows(300, 11, "up", spread=35, scale=1)
    corner_cells = [(0, 0), (23, 0), (0, 19), (23, 19), (24, 10), (12, 20), (-1, 5), (12, 12), (12, 12)]
    corner_rows = np.array([K.frame_row((4 * c[0] + 1.3, 4 * c[1] + 2.2), np.eye(2), (10, 10), np.eye(2)) for c in corner_cells])
    corner_rows[8] = corner_rows[7]                                             # two identical rows: ties everywhere, the lower wins
    return [
        ("tie", K.W1, K.H1, 4, 1, tie, None, occupied(tie, K.W1, K.H1, 4)),
        ("grid 48 x 40", K.W1, K.H1, 2, 4, many, None, occupied(many, K.W1, K.H1, 2, closed=200, seed=1)),
        ("collide", K.W1, K.H1, 4, 2, many, None, occupied(many, K.W1, K.H1, 4, closed=40, seed=2)),
        ("corners", K.W1 + 3, K.H1 + 2, 4, 4, corner_rows, corner_cells, np.zeros((20, 24), np.uint8)),
        ("all free", K.W1, K.H1, 8, 1, many[:5], None, np.zeros((10, 12), np.uint8)),
    ]
