"""Inputs of the direct tests of the RANSAC scoring and counting kernels (test_cpu_ransac_score_ref.py anchors the reference on
them, test_gpu_ransac_score.py judges the kernels with them).  Nothing here calls the library.

Correspondences are in pixels, made by make_corr (test_gpu_ransac.py) and fsynth.two_view, with a few planted ones in front so
that every threshold band and every exact case occurs by construction instead of by luck.  With P planted correspondences that
fit (len >= P), relative to the generating model:

  0  the anchor: x1 = x2 = (256, 512), exactly representable.  The horizon of the `horizon` models passes through it, the
     identity homography and the pure-translation F have error exactly 0 on it (th = 0 rounds count it).
  1  exact: x2 on the model (error about 0)
  2, 3, 4  displaced by 3.5, 4.5 and 7 px from the model: a displacement r gives about r^2 / 2 (Sampson), r^2 (symmetric max) and
     2 r^2 (symmetric sum, symmetric epipolar), so for th = 16 one of the three lies in (th, th 9/4) = (16, 36) under every error
     type, and r = 4.5 lies in (d, d 9/4) of r = 3.5 (ratio 1.65) when th is set to the error of correspondence 2
  5  displaced by 100 px: beyond th 9/4
The threshold bands can all be occupied only from len = 6 on; below that the rounds keep what fits (len 1: the anchor alone)."""
import numpy as np

import fsynth
from test_gpu_ransac import make_corr

TH = 16.0                 # squared pixels, as LORANSACFiltering passes it for a 4 px threshold
H_CHECK_COEF = 9.0        # th_check = 9 th, exp_ranH.c
F_CHECK_COEF = 16.0       # th_check = 16 th, exp_ranF.c
PLANTED = 6
OFFSETS = (0.0, 3.5, 4.5, 7.0, 100.0)     # correspondences 1 .. 5

# the generating homography of make_corr (image 1 -> image 2)
H12 = np.array([[1.05, 0.08, 12.0], [-0.06, 0.97, -7.0], [8e-5, -4e-5, 1.0]])

# shapes (len, n) of the score + gain rounds: every len with n in {1, 16, 17}, every n with len in {129, 385}
LENS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 769, 1000)
H_NS = (1, 8, 16, 17, 63, 64, 65, 130)
F_NS = (1, 24, 64, 65, 288)


def shapes(ns):
    out = [(ln, n) for ln in LENS for n in (1, 16, 17)]
    out += [(ln, n) for n in ns for ln in (129, 385) if (ln, n) not in out]
    return out


def h_of(H_1to2):
    """a homography image 1 -> image 2 in the layout exp_ransacHcustom carries: column-major, image 2 -> image 1"""
    M = np.linalg.inv(H_1to2)
    return np.ascontiguousarray(M.T.ravel() / M[2, 2])


def _transfer(H, x):
    p = np.c_[x, np.ones(len(x))] @ H.T
    return p[:, :2] / p[:, 2:]


def h_corr(ln, seed):
    """ln correspondences: inliers of H12 with 0.5 px noise plus 50 % uniform outliers, the planted ones in front"""
    u = make_corr(max(ln, 8), 0.5, 0.5, seed)[:ln].copy()
    u[0, 0:2] = u[0, 3:5] = (256.0, 512.0)
    k = min(ln, PLANTED)
    if k > 1:
        x2 = _transfer(H12, u[1:k, 0:2])
        x2[:, 0] += np.array(OFFSETS[:k - 1])
        u[1:k, 3:5] = x2
    return np.ascontiguousarray(u)


def _dlt(u, idx):
    """minimal solution x1 ~ M x2 of 4 correspondences (null vector of the 8 x 9 system), in the column-major layout"""
    A = []
    for i in idx:
        x, y, X, Y = u[i, 3], u[i, 4], u[i, 0], u[i, 1]
        A.append([x, y, 1, 0, 0, 0, -X * x, -X * y, -X])
        A.append([0, 0, 0, x, y, 1, -Y * x, -Y * y, -Y])
    m = np.linalg.svd(np.array(A))[2][-1].reshape(3, 3)
    return np.ascontiguousarray(m.T.ravel() / np.abs(m).max())


IDENTITY_H = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])
# rank 2, small integers: Hinv's third row is zero (b = 0 for every correspondence: the symmetric parts divide by it) and
# a e = b d with c = 0 in pinvJ (N = 0: HDs is 0 / 0), so every error type is non-finite on it
RANK2_H = np.array([1.0, 2, 0, 2, 4, 0, 3, 5, 0])


def horizon_h(both_zero):
    """the generating model with the third row of Hinv replaced so that b = Hinv6 x2 + Hinv7 y2 + Hinv8 is exactly 0 at the anchor
    (2^-10 256 + 2^-10 512 - 0.75): d2 = (finite / 0)^2 = inf there.  both_zero: the numerator of xa vanishes there as well
    (1 x2 + 0 y2 - 256), so d2 = NaN while d1 stays finite - the case in which MAX(d1, d2) of Htools.c:15 and a max written
    the other way round differ."""
    h = h_of(H12)
    h[2], h[5], h[8] = 2.0 ** -10, 2.0 ** -10, -0.75
    if both_zero:
        h[0], h[3], h[6] = 1.0, 0.0, -256.0
    return h


def h_models(u, n, seed):
    """n models of a round and the indices of the degenerate ones.  0: the generating H; 1: rank 2; 2: the identity;
    n - 2, n - 1: the two horizon models; between them perturbations of the generating H and minimal 4-point solutions."""
    g = np.random.default_rng(1000 + seed)
    base = h_of(H12)
    models, degenerate = [base], []
    fixed = [(RANK2_H, True), (IDENTITY_H, False)]
    tail = [(horizon_h(True), True), (horizon_h(False), True)]
    while len(models) < n and fixed and len(models) + len(tail) < n:
        m, deg = fixed.pop(0)
        if deg:
            degenerate.append(len(models))
        models.append(m)
    n_mid = max(0, n - len(models) - len(tail))
    for j in range(n_mid):
        if j % 2 == 0 or len(u) < 8:
            models.append(base * (1 + g.normal(0, (1e-5, 1e-4, 1e-3)[(j // 2) % 3], 9)))
        else:
            models.append(_dlt(u, g.choice(len(u), 4, replace=False)))
    for m, deg in tail:
        if len(models) < n:
            degenerate.append(len(models))
            models.append(m)
    return np.ascontiguousarray(np.array(models[:n])), [k for k in degenerate if k < n]


def true_f(seed, size=(1920, 1080)):
    """the fundamental matrix of fsynth.two_view(seed=seed) (its camera pair is the generator's first draws), as the 3 x 3 matrix
    Fm with x2^T Fm x1 = 0, norm 1"""
    rng = np.random.default_rng(seed)
    w, h = size
    K = np.array([[1.2 * w, 0, w / 2], [0, 1.2 * w, h / 2], [0, 0, 1]])
    R = fsynth._rot(rng, 12)
    t = np.array([rng.uniform(0.4, 0.9) * rng.choice([-1, 1]), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    Fm = Ki.T @ tx @ R @ Ki
    return Fm / np.linalg.norm(Fm), (K, R, t)


def f_of(Fm):
    """Fm (x2^T Fm x1 = 0) in the layout exp_ransacFcustom carries: F[i + 3 j] multiplies x1_i x2_j"""
    return np.ascontiguousarray(np.asarray(Fm, np.float64).ravel())


def f_corr(ln, seed):
    """ln correspondences of a general scene (60 % inliers, 0.5 px noise), the planted ones in front; returns (u, F true)"""
    u = fsynth.two_view(max(ln, 16), 0.6, 0.0, 0.5, seed=seed)[0][:ln].copy()
    Fm, _ = true_f(seed)
    u[0, 0:2] = u[0, 3:5] = (256.0, 512.0)
    k = min(ln, PLANTED)
    for i in range(1, k):
        x1 = np.array([u[i, 0], u[i, 1], 1.0])
        l = Fm @ x1                                   # the epipolar line of x1 in image 2
        nrm = l[:2] / np.hypot(l[0], l[1])
        x2 = np.array([960.0 + 37.0 * i, 540.0 - 23.0 * i])
        x2 = x2 - ((l[0] * x2[0] + l[1] * x2[1] + l[2]) / np.hypot(l[0], l[1])) * nrm      # onto the line
        u[i, 3:5] = x2 + OFFSETS[i - 1] * nrm
    return np.ascontiguousarray(u), f_of(Fm)


# x2^T Fm x1 = y1 - y2: exactly 0 at the anchor, with the denominator 2
TRANSLATION_F = f_of(np.array([[0.0, 0, 0], [0, 0, -1], [0, 1, 0]]))
# rank 1, e3 e3^T: every line term is 0 and the residual is 1, so FDs = 1 / 0 = inf and FDsSym = 0 / 0
RANK1_F = f_of(np.array([[0.0, 0, 0], [0, 0, 0], [0, 0, 1]]))


def f_models(F, n, seed):
    """n candidates and the indices of the degenerate ones.  0: the true F; 1: rank 1; 2: the pure translation; n - 1: the zero
    matrix; the rest entry-wise perturbations of the true F, as the roots of a 7-point sample near it would be (rank not enforced)."""
    g = np.random.default_rng(2000 + seed)
    models, degenerate = [F], []
    if n >= 3:
        degenerate.append(len(models)); models.append(RANK1_F)
    if n >= 4:
        models.append(TRANSLATION_F)
    n_tail = 1 if n >= 2 else 0
    j = 0
    while len(models) < n - n_tail:
        models.append(F * (1 + g.normal(0, (1e-4, 1e-3, 1e-2)[j % 3], 9)))
        j += 1
    if n_tail:
        degenerate.append(len(models)); models.append(np.zeros(9))
    return np.ascontiguousarray(np.array(models)), degenerate


def rounds(ln, n, err_types):
    """(err_type, do_sym, th kind) of the rounds of one shape: every error type with and without the symmetric check at th = 16,
    then one round whose th is the reference's own error of correspondence min(2, len - 1) under model 0 (d <= th met with
    equality), one with th = 0, and one with th = 1e308, where th 9/4 overflows to infinity: every finite error gains exactly 1
    and an infinite one (a degenerate model's) meets truncQuad's `>=` with equality - the only place where `>=` and `>` differ,
    since 1 - x / x is 0 for a finite bound.  That round uses the error type under which the degenerate models are infinite and
    not NaN: the symmetric sum for H (the horizon model's d2), Sampson for F (the rank-1 matrix)."""
    out = [(e, s, "fixed") for e in err_types for s in (1, 0)]
    out.append((err_types[(ln + n) % len(err_types)], 1, "equal"))
    out.append((err_types[(ln + n + 1) % len(err_types)], 1, "zero"))
    out.append((1 if len(err_types) == 3 else 0, 1, "huge"))
    return out


def round_th(th_kind, d_ref, ln):
    """th of a round; "equal" takes it from the reference's errors d_ref [n][len] of the round's error type"""
    if th_kind == "equal":
        return float(d_ref[0, min(2, ln - 1)])
    return {"zero": 0.0, "huge": 1e308, "fixed": TH}[th_kind]


def off_plane_scene(n, seed):
    """rFtH's inputs for a scene with a dominant plane: the n off-plane correspondences uN, their plane-transferred form us
    (DegUtils.c:300-308), H (the plane's homography in degensac's layout) and Ht = H transposed"""
    big = fsynth.two_view(4 * n + 64, 0.7, 0.4, 0.5, seed=seed)
    u, on_plane = big[0], big[2]
    uN = np.ascontiguousarray(u[~on_plane][:n])
    assert len(uN) == n
    _, (K, R, t) = true_f(seed)
    nrm = np.array([0.15, -0.1, 1.0])
    H_1to2 = K @ (R + np.outer(t, nrm) / 5.0) @ np.linalg.inv(K)
    H = h_of(H_1to2)
    us = uN.copy()
    us[:, 3] = H[0] * uN[:, 3] + H[3] * uN[:, 4] + H[6] * uN[:, 5]
    us[:, 4] = H[1] * uN[:, 3] + H[4] * uN[:, 4] + H[7] * uN[:, 5]
    us[:, 5] = H[2] * uN[:, 3] + H[5] * uN[:, 4] + H[8] * uN[:, 5]
    Ht = np.ascontiguousarray(H.reshape(3, 3).T.ravel())
    return uN, np.ascontiguousarray(us), H, Ht


def pair_block(n, k, seed, with_equal):
    """k index pairs below n (two distinct indices, as rFtH draws them); with_equal: one pair of equal indices in the middle"""
    g = np.random.default_rng(seed)
    p0 = g.integers(0, n, k)
    p1 = (p0 + g.integers(1, max(n, 2), k)) % n if n > 1 else p0.copy()
    pairs = np.stack([p0, p1], axis=1).astype(np.uint32)
    if with_equal:
        pairs[k // 2, 1] = pairs[k // 2, 0]
    return np.ascontiguousarray(pairs)
