"""Inputs of the least-squares refinement tests (tests/test_cpu_lsm.py, tests/test_gpu_lsm.py): a scene in closed form, image pairs
of it related by an exact affine map with gain and offset, and correspondence rows with displaced starts.  Pure numpy."""
import numpy as np

W1, H1, W2, H2 = 96, 80, 64, 112                # the GPU tests' image sizes: different from each other
STRIDE1, STRIDE2 = 104, 67                      # ... and their row strides, larger than the widths
# image 1 -> image 2 is x2 = A x1 + t.  "up": det A = 1.1598, image 1 holds the template; "down": det A = 0.7955, image 2 does
A_OF = {"up": np.array([[1.05, 0.08], [-0.06, 1.10]]), "down": np.array([[0.90, -0.07], [0.05, 0.88]])}
C1, C2 = np.array([48.0, 40.0]), np.array([32.0, 56.0])
T_OF = {k: C2 - A @ C1 for k, A in A_OF.items()}
A_TRUE, T_TRUE = A_OF["up"], T_OF["up"]
GAIN, OFFSET = 0.85, 9.0


def scene(seed=1):
    """f(x, y): Gaussians and sinusoids, evaluated in closed form anywhere in the plane"""
    rng = np.random.default_rng(seed)
    nb, ns = 160, 10
    bx, by = rng.uniform(-40, 140, nb), rng.uniform(-40, 140, nb)
    bs, ba = rng.uniform(1.6, 4.0, nb), rng.uniform(15, 50, nb) * rng.choice([-1.0, 1.0], nb)
    kx, ky = rng.uniform(-0.55, 0.55, ns), rng.uniform(-0.55, 0.55, ns)
    ph, sa = rng.uniform(0, 2 * np.pi, ns), rng.uniform(3, 9, ns)

    def f(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        out = np.full(np.broadcast(x, y).shape, 128.0)
        for i in range(nb):
            out = out + ba[i] * np.exp(-((x - bx[i]) ** 2 + (y - by[i]) ** 2) / (2 * bs[i] * bs[i]))
        for j in range(ns):
            out = out + sa[j] * np.sin(kx[j] * x + ky[j] * y + ph[j])
        return out
    return f


def strided(img, stride):
    """the image as a view of a wider array (row stride `stride` floats), the padding filled with NaN: nothing may read it"""
    h, w = img.shape
    buf = np.full((h, stride), np.nan, np.float32)
    buf[:, :w] = img
    return buf[:, :w]


_cache = {}


def analytic_pair(kind="up", seed=1):
    """(img1 96 x 80, img2 64 x 112), img2(x) = GAIN f(A^-1 (x - t)) + OFFSET evaluated in closed form - exact, not interpolated;
    both float32 views with the strides above"""
    if (kind, seed) not in _cache:
        f = scene(seed)
        A_TRUE, T_TRUE = A_OF[kind], T_OF[kind]
        yy, xx = np.mgrid[0:H1, 0:W1].astype(np.float64)
        img1 = f(xx, yy).astype(np.float32)
        yy, xx = np.mgrid[0:H2, 0:W2].astype(np.float64)
        Ai = np.linalg.inv(A_TRUE)
        sx = Ai[0, 0] * (xx - T_TRUE[0]) + Ai[0, 1] * (yy - T_TRUE[1])
        sy = Ai[1, 0] * (xx - T_TRUE[0]) + Ai[1, 1] * (yy - T_TRUE[1])
        img2 = (GAIN * f(sx, sy) + OFFSET).astype(np.float32)
        for im in (img1, img2):
            im.setflags(write=False)
        _cache[(kind, seed)] = (strided(img1, STRIDE1), strided(img2, STRIDE2))
    return _cache[(kind, seed)]


def frame_row(c1, M1, c2, M2):
    """a laf row from two centres and two 2 x 2 frames (stored as s = sqrt(|det|), A = M / s)"""
    out = []
    for c, M in ((c1, M1), (c2, M2)):
        M = np.asarray(M, np.float64)
        s = np.sqrt(abs(np.linalg.det(M)))
        out += [c[0], c[1], M[0, 0] / s, M[0, 1] / s, M[1, 0] / s, M[1, 1] / s, s]
    return np.array(out, np.float64)


def true_rows(n, seed, kind="up", spread=6.0, scale=3.0):
    """n exact correspondences of the analytic pair: centres within +-spread of the images' centres, frame 1 = scale I"""
    rng = np.random.default_rng(seed)
    A_TRUE, T_TRUE = A_OF[kind], T_OF[kind]
    rows = []
    for _ in range(n):
        c1 = C1 + rng.uniform(-spread, spread, 2)
        rows.append(frame_row(c1, scale * np.eye(2), A_TRUE @ c1 + T_TRUE, scale * A_TRUE))
    return np.array(rows)


def displaced(rows, seed, shift=1.5, rel=0.10):
    """the rows with the second centre moved by up to `shift` px (uniform in the disc) and every entry of the second frame
    changed by up to +-rel of itself"""
    rng = np.random.default_rng(seed)
    out = np.array(rows, np.float64)
    for r in out:
        ang, rad = rng.uniform(0, 2 * np.pi), shift * np.sqrt(rng.uniform())
        r[7] += rad * np.cos(ang); r[8] += rad * np.sin(ang)
        M = r[13] * r[9:13] * (1.0 + rng.uniform(-rel, rel, 4))
        s = np.sqrt(abs(M[0] * M[3] - M[1] * M[2]))
        r[9:13], r[13] = M / s, s
    return out


def swap_sides(rows):
    """the rows of the pair (img2, img1): the two halves exchanged"""
    rows = np.asarray(rows, np.float64).reshape(-1, 14)
    return np.concatenate([rows[:, 7:], rows[:, :7]], axis=1)


def transfer_error(rows, kind="up"):
    """|A x1 + t - x2| of rows of the pair (img1, img2)"""
    rows = np.asarray(rows, np.float64).reshape(-1, 14)
    A_TRUE, T_TRUE = A_OF[kind], T_OF[kind]
    p = rows[:, 0:2] @ A_TRUE.T + T_TRUE
    return np.hypot(*(p - rows[:, 7:9]).T)


PAIR_SEED, PAIR_SEED_TIME = 7, 777      # the synthetic planar pair (synth.pair at 400 x 300) of the end-to-end tests ...
PAIR_REJECTED = 0                       # ... and how many of its verified rows the restatement rejects (tests/test_cpu_lsm.py)
MIXED_PAR = dict(max_iter=3, min_zncc=0.95)


def mixed_pair():
    """the "up" pair with a constant block in the corner of image 1 (dense copies with the same strides)"""
    a, b = analytic_pair("up")
    a = np.array(a)
    a[0:30, 0:30] = 77.0
    return strided(a, STRIDE1), b


def mixed_rows():
    """rows of mixed_pair() that end, with the parameters MIXED_PAR, in every status of the contract - so the waves of one
    workgroup leave at different iterations"""
    eye3 = 3 * np.eye(2)
    good = displaced(true_rows(8, 5), 6)
    rows = list(good)
    rows.append(frame_row((14, 14), eye3, (30, 50), 3 * A_TRUE))                       # FLAT: a constant template
    rows.append(frame_row((9.5, 40), eye3, (30, 50), 3 * A_TRUE))                      # OUTSIDE: the template
    rows.append(frame_row((48, 40), eye3, (57, 56), 3 * A_TRUE))                       # OUTSIDE: the search window
    bad = good[0].copy(); bad[4] = np.nan
    rows.append(bad)                                                                   # BAD_FRAME: not finite
    rows.append(frame_row((48, 40), eye3, (32, 56), np.array([[3.0, 0], [0, -3.0]])))  # BAD_FRAME: det B0 < 0
    rows.append(frame_row((48, 40), eye3, (32, 56), 27 * np.eye(2)))                   # BAD_FRAME: magnification 9
    true = true_rows(6, 9)
    for r, off in zip(true, ((6, 0), (0, 6), (5, 4), (-6, 3), (8, 0), (4, -7))):       # far off: DIVERGED or LOW_ZNCC
        r = r.copy(); r[7] += off[0]; r[8] += off[1]
        rows.append(r)
    c, sn = np.cos(np.deg2rad(30)), np.sin(np.deg2rad(30))
    M = 3 * A_TRUE @ np.array([[c, -sn], [sn, c]])
    for r in true[:3]:                                                                 # a frame 30 degrees off: MAXITER or LOW_ZNCC
        rows.append(np.r_[r[:7], frame_row((0, 0), M, (r[7], r[8]), M)[7:]])
    return np.array(rows)


# The yardstick of tests/test_gpu_lsm.py.  The restatement run with its window sums forward and reversed differs, over the groups
# below, by at most SPREAD in a coordinate, a frame entry or a zncc value (measured on the CPU: 3.05e-12, from the 3 x 3 windows, whose
# normal equations are the worst conditioned; 21 x 21 windows: 7.1e-15; the mixed list: 1.1e-14), with equal statuses and iteration
# counts; N, g, a and delta of a first iteration differ by at most SEAM_SPREAD of their largest entry (measured: delta 1.3e-14, g
# 4.3e-15, N 2.1e-15, a 1.1e-15).  tests/test_cpu_lsm.py holds both figures against the restatement.
SPREAD = 3.05e-12
SEAM_SPREAD = 1.3e-14


def groups():
    """(name, pair kind or "mixed", rows, parameter overrides): the cases of the GPU test"""
    up = displaced(true_rows(65, 5, "up"), 6)
    dn = displaced(true_rows(8, 7, "down"), 8)
    g = [("r10", "up", up, {})]
    g += [("r%d" % R, "up", up[:8], dict(radius=R)) for R in (1, 3, 4, 15)]
    g += [("down r10", "down", dn, {}), ("down r4", "down", dn, dict(radius=4)), ("translation", "up", up[:8], dict(affine=0)),
          ("one iteration", "up", up[:8], dict(max_iter=1)), ("mixed", "mixed", mixed_rows(), MIXED_PAR)]
    return g


def images_of(kind):
    return mixed_pair() if kind == "mixed" else analytic_pair(kind)


def seam_cases():
    """(name, pair kind, row, parameter overrides) of the one-iteration seam"""
    up = displaced(true_rows(65, 5, "up"), 6)
    dn = displaced(true_rows(8, 7, "down"), 8)
    return [("r10", "up", up[0], {}), ("r4", "up", up[1], dict(radius=4)), ("r15", "up", up[2], dict(radius=15)), ("r1", "up", up[3], dict(radius=1)),
            ("down", "down", dn[0], {}), ("translation", "up", up[4], dict(affine=0))]


def homography_error(H, rows):
    """|H x1 - x2| of rows under a homography image 1 -> image 2"""
    rows = np.asarray(rows, np.float64).reshape(-1, 14)
    p = np.c_[rows[:, 0:2], np.ones(len(rows))] @ np.asarray(H, np.float64).reshape(3, 3).T
    return np.hypot(*(p[:, :2] / p[:, 2:] - rows[:, 7:9]).T)
