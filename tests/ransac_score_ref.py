"""fp64 restatement, in numpy, of what the scoring and counting kernels behind LO-RANSAC and DEGENSAC compute
(csrc/ransac.hip, csrc/ransac_f.hip), written from the formulas of degensac:

  pinvJ, HDs                Htools.c:134-199      (the design rows of lin_hg, Htools.c:19-57, written out)
  the halves of HDsSym      Htools.c:222-238      (Hinv and H1 are inputs: H1 = minv(Hinv) is not restated)
  truncQuad, inlidxs        rtools.c:160-171, 228-236
  FDs, FDsSym               Ftools.c:83-124
  the candidate of rFtH     DegUtils.c:246-250, 353-371 (crossp x 3, the norm, three divisions, skew_sym, mmul, mattr)

Every operation stands once, in the C code's order, and is rounded once (numpy's element-wise fp64 arithmetic); sums that the C
code forms left to right are formed left to right; the MSAC score is a strictly sequential sum in correspondence order
(np.add.accumulate, never np.sum, which adds pairwise).  The functions work on all correspondences of one model at a time: the
vector axis runs over correspondences, never over the terms of a sum.

Layouts as degensac carries them: u is len x 6 (x1 y1 1 x2 y2 1); a homography is h[9] with h[r + 3 c] = M[r][c], M mapping
image 2 to image 1; a fundamental matrix is F[9] with the residual sum_ij x1_i F[i + 3 j] x2_j."""
import numpy as np

_QUIET = dict(divide="ignore", invalid="ignore", over="ignore")


def pinvJ(a, b, c, d, e):
    """Htools.c:134-158 -> pJ[8]"""
    a2, b2, c2, d2, e2 = a * a, b * b, c * c, d * d, e * e
    c2pd2, ab, de = c2 + d2, a * b, d * e
    Q = c * (c2pd2 + e2)
    pJ = [None] * 8
    pJ[0] = (-b) * de + a * (c2 + e2)
    pJ[1] = b * c2pd2 - a * de
    pJ[2] = Q
    pJ[3] = (-c) * (a * d + b * e)
    pJ[4] = d * (b2 + c2) - ab * e
    pJ[5] = (-ab) * d + e * (a2 + c2)
    pJ[6] = pJ[3]
    pJ[7] = c * ((a2 + b2) + c2)
    N = (a * pJ[0] + b * pJ[1]) + c * pJ[2]
    return [p / N for p in pJ]


def hds(u, H):
    """HDs, Htools.c:160-198: the Sampson error of every correspondence under one model"""
    u = np.asarray(u, np.float64)
    H = [np.float64(x) for x in H]
    u0, u1, u3, u4, u5 = u[:, 0], u[:, 1], u[:, 3], u[:, 4], u[:, 5]
    zero = np.zeros(len(u))
    with np.errstate(**_QUIET):
        # the two rows of lin_hg per correspondence, column by column (Htools.c:33-54)
        z0 = [u3, zero, (-u0) * u3, u4, zero, (-u0) * u4, u5, zero, (-u0) * u5]
        z1 = [zero, u3, (-u1) * u3, zero, u4, (-u1) * u4, zero, u5, (-u1) * u5]
        r1, r2 = np.zeros(len(u)), np.zeros(len(u))
        for j in range(9):
            r1 = r1 + H[j] * z0[j]
            r2 = r2 + H[j] * z1[j]
        a = H[0] - H[2] * u0
        b = H[3] - H[5] * u0
        c = ((-H[8]) - H[2] * u3) - H[5] * u4
        d = H[1] - H[2] * u1
        e = H[4] - H[5] * u1
        pJ = pinvJ(a, b, c, d, e)
        p = np.zeros(len(u))
        for j in range(4):
            t = pJ[j] * r1 + pJ[j + 4] * r2
            p = p + t * t
    return p


def hsym_parts(u, Hinv, H1):
    """the two halves d1, d2 of HDsSym / HDsSymMax, Htools.c:222-238, for the operands Hinv and H1 = minv(Hinv) as given"""
    u = np.asarray(u, np.float64)
    Hinv = [np.float64(x) for x in Hinv]
    H1 = [np.float64(x) for x in H1]
    u0, u1, u3, u4 = u[:, 0], u[:, 1], u[:, 3], u[:, 4]
    with np.errstate(**_QUIET):
        a = (H1[6] * u0 + H1[7] * u1) + H1[8]
        b = (Hinv[6] * u3 + Hinv[7] * u4) + Hinv[8]
        xa = ((H1[0] * u0 + H1[1] * u1) + H1[2]) / a
        ya = ((H1[3] * u0 + H1[4] * u1) + H1[5]) / a
        xdiff, ydiff = u3 - xa, u4 - ya
        d1 = xdiff * xdiff + ydiff * ydiff
        xa = ((Hinv[0] * u3 + Hinv[1] * u4) + Hinv[2]) / b
        ya = ((Hinv[3] * u3 + Hinv[4] * u4) + Hinv[5]) / b
        xdiff, ydiff = u0 - xa, u1 - ya
        d2 = xdiff * xdiff + ydiff * ydiff
    return d1, d2


def hinv_of(h):
    """Hinv of HDsSym, Htools.c:208-216: h transposed as stored"""
    h = np.asarray(h, np.float64)
    return h[[0, 3, 6, 1, 4, 7, 2, 5, 8]].copy()


def c_max(d1, d2):
    """MAX(d1, d2) of Htools.c:15: (d1 < d2) ? d2 : d1"""
    return np.where(d1 < d2, d2, d1)


def h_error(u, h, Hinv, H1, err_type):
    """d of one model: err_type 0 HDs, 1 HDsSym (d1 + d2), 2 HDsSymMax; also returns d1 + d2 (the symmetric check's operand)"""
    d1, d2 = hsym_parts(u, Hinv, H1)
    with np.errstate(**_QUIET):
        s = d1 + d2
    if err_type == 0:
        return hds(u, h), s
    return (s if err_type == 1 else c_max(d1, d2)), s


def _f_terms(u, F):
    F = [np.float64(x) for x in F]
    u0, u1, u3, u4 = u[:, 0], u[:, 1], u[:, 3], u[:, 4]
    rxc = (F[0] * u3 + F[3] * u4) + F[6]
    ryc = (F[1] * u3 + F[4] * u4) + F[7]
    rwc = (F[2] * u3 + F[5] * u4) + F[8]
    r = (u0 * rxc + u1 * ryc) + rwc
    rx = (F[0] * u0 + F[1] * u1) + F[2]
    ry = (F[3] * u0 + F[4] * u1) + F[5]
    return r, rxc, ryc, rx, ry


def fds(u, F):
    """FDs, Ftools.c:83-101: Sampson's error"""
    u = np.asarray(u, np.float64)
    with np.errstate(**_QUIET):
        r, rxc, ryc, rx, ry = _f_terms(u, F)
        return (r * r) / (((rxc * rxc + ryc * ryc) + rx * rx) + ry * ry)


def fds_sym(u, F):
    """FDsSym, Ftools.c:103-124: the symmetric epipolar distance"""
    u = np.asarray(u, np.float64)
    with np.errstate(**_QUIET):
        r, rxc, ryc, rx, ry = _f_terms(u, F)
        a = rxc * rxc + ryc * ryc
        b = rx * rx + ry * ry
        return ((r * r) * (a + b)) / (a * b)


def trunc_quad(eps, thr):
    """truncQuad, rtools.c:228-236, of a vector of errors"""
    eps = np.asarray(eps, np.float64)
    thr = np.float64(thr)
    if thr == 0:
        return np.zeros(len(eps))
    with np.errstate(**_QUIET):
        lim = thr * 9 / 4
        return np.where(eps >= lim, 0.0, 1 - (eps / lim))


def msac_sum(gains):
    """s.J of inlidxs (rtools.c:160-171): 0, then += one gain after the other"""
    return np.add.accumulate(np.concatenate([[0.0], np.asarray(gains, np.float64)]))[-1]


def errors_h(u, records, err_type):
    """(d, s) [n][len] of the models of a round: records = (h, Hinv, H1), n x 9 each, as the kernel saw them; s = d1 + d2"""
    u = np.asarray(u, np.float64)
    h, Hinv, H1 = records
    d, s = np.zeros((len(h), len(u))), np.zeros((len(h), len(u)))
    for k in range(len(h)):
        d[k], s[k] = h_error(u, h[k], Hinv[k], H1[k], err_type)
    return d, s


def errors_f(u, F, err_type):
    """(d, s) [n][len] of the candidates of a round: err_type 0 FDs, 1 FDsSym; s = FDsSym, the symmetric check's operand"""
    u = np.asarray(u, np.float64)
    F = np.asarray(F, np.float64).reshape(-1, 9)
    d, s = np.zeros((len(F), len(u))), np.zeros((len(F), len(u)))
    for k in range(len(F)):
        s[k] = fds_sym(u, F[k])
        d[k] = s[k] if err_type == 1 else fds(u, F[k])
    return d, s


def scores(d, s, do_sym, th, th_check):
    """What a scoring round reports per model besides d: J = the sequential sum of truncQuad(d_i, th), I = #(d <= th),
    Isym = #(s <= th_check) when the symmetric check is on, else 0"""
    n = len(d)
    J, I, Isym = np.zeros(n), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k in range(n):
        J[k] = msac_sum(trunc_quad(d[k], th))
        I[k] = int(np.count_nonzero(d[k] <= np.float64(th)))
        Isym[k] = int(np.count_nonzero(s[k] <= np.float64(th_check))) if do_sym else 0
    return dict(d=d, J=J, I=I, Isym=Isym, s=s)


def _crossp(u, v):
    """crossp, DegUtils.c:246-250, of k vectors side by side (k x 3)"""
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1],
                     u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def rfth_candidates(us, pairs, Ht):
    """The plane-and-parallax candidates of rFtH, DegUtils.c:353-371, for k index pairs into us (n x 6): k x 9 matrices aFt."""
    us = np.asarray(us, np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    Ht = [np.float64(x) for x in np.asarray(Ht, np.float64).reshape(9)]
    a0, a1 = us[pairs[:, 0]], us[pairs[:, 1]]
    k = len(pairs)
    with np.errstate(**_QUIET):
        c1 = _crossp(a0[:, 0:3], a0[:, 3:6])
        c2 = _crossp(a1[:, 0:3], a1[:, 3:6])
        ec = _crossp(c1, c2)
        norm = np.sqrt((ec[:, 0] * ec[:, 0] + ec[:, 1] * ec[:, 1]) + ec[:, 2] * ec[:, 2])
        e0, e1, e2 = ec[:, 0] / norm, ec[:, 1] / norm, ec[:, 2] / norm
        zero = np.zeros(k)
        sk = [zero, -e2, e1, e2, zero, -e0, -e1, e0, zero]                 # skew_sym
        prod = [None] * 9
        for i in range(3):                                                 # mmul(aFtH, aFt, Ht, 3): s = 0; s += a[i][q] b[q][j]
            for j in range(3):
                s = np.zeros(k)
                for q in range(3):
                    s = s + sk[3 * i + q] * Ht[3 * q + j]
                prod[3 * i + j] = s
        return np.stack([prod[3 * j + i] for i in range(3) for j in range(3)], axis=1)   # mattr: the transpose


def count_below(u, F, limit):
    """#{i : FDs(u_i, F) < limit}, DegUtils.c:373-382"""
    return int(np.count_nonzero(fds(u, F) < np.float64(limit)))


def count_pairs(uN, us, pairs, Ht, limit):
    return np.array([count_below(uN, F, limit) for F in rfth_candidates(us, pairs, Ht)], np.uint32)


def count_models(u, Fs, limit):
    return np.array([count_below(u, F, limit) for F in np.asarray(Fs, np.float64).reshape(-1, 9)], np.uint32)
