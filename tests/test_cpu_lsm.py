"""The least-squares refinement of correspondences (csrc/refine.hip) without a device: the numpy restatement of its contract
(tests/lsm_ref.py) held against ground truth that does not come from it, every status, the role rule, the model refit against
numpy.linalg, and the refusals.

Measured with the restatement on the analytic pairs of tests/lsm_cases.py (image 2 evaluated in closed form at A^-1 (x - t) with gain
0.85 and offset 9; 24 rows per pair, starts up to 1.5 px off, every frame entry changed by up to +-10 %), defaults (21 x 21 window):
    pair "up"   (image 1 holds the template): position error 1.021 px mean at the start -> 0.0086 mean, 0.0201 max;
                                              largest entry error of the refined affinity 0.0033; 3.2 iterations on average
    pair "down" (image 2 holds the template): 0.0083 mean, 0.0202 max; affinity 0.0026
    translation only: 0.186 / 0.165 mean, 0.478 / 0.324 max (the affinity stays 10 % off: the bound is the start's)
All 96 cases converge (status OK).  The assertions are these maxima with a margin of two: 0.04 px and 0.007 for the affine
mode, 1.0 px for translation only."""
import ctypes as C
import os

import numpy as np
import pytest

import lsm_cases as K
import lsm_ref as L
import refdeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read
E_ARG = -2
POS_BOUND, AFF_BOUND, POS_BOUND_TRANSLATION = 0.04, 0.007, 1.0
NAMES = ("mods_lsm_defaults", "mods_refine_matches_dev", "mods_refine_matches", "mods_refit_model", "mods_test_lsm_iteration")


# ---- recovery on analytic images

@pytest.mark.parametrize("kind", ["up", "down"])
@pytest.mark.parametrize("affine", [1, 0])
def test_restatement_recovers_the_analytic_map(kind, affine):
    a, b = K.analytic_pair(kind)
    true = K.true_rows(24, 5, kind)
    start = K.displaced(true, 6)
    out, u6, st, it, zb, za = L.refine(a, b, start, L.params(affine=affine))
    assert (st == L.OK).all(), st
    err = K.transfer_error(out, kind)
    print("\n%s affine=%d: start %.3f px mean, refined %.4f mean %.4f max, %.2f iterations" % (kind, affine, K.transfer_error(start, kind).mean(),
                                                                                            err.mean(), err.max(), it.mean()))
    assert K.transfer_error(start, kind).mean() > 0.9
    if affine:
        aff = max(np.abs(L.affine_of(r) - K.A_OF[kind]).max() for r in out)
        assert err.max() < POS_BOUND and aff < AFF_BOUND, (err.max(), aff)
        assert (za > 0.9999).all() and (zb < za).all()
    else:
        assert err.max() < POS_BOUND_TRANSLATION and err.mean() < 0.25 * K.transfer_error(start, kind).mean()
    # the template side is untouched, the search side moved; u6 is the centres of the rows
    tmpl, srch = (slice(0, 7), slice(7, 14)) if kind == "up" else (slice(7, 14), slice(0, 7))
    assert np.array_equal(out[:, tmpl], start[:, tmpl]) and (out[:, srch] != start[:, srch]).any(axis=1).all()
    assert np.array_equal(u6, np.c_[out[:, 0:2], np.ones(24), out[:, 7:9], np.ones(24)])


# ---- statuses

def _grating():
    yy, xx = np.mgrid[0:80, 0:96].astype(np.float64)
    return (128 + 50 * np.sin(2 * np.pi * xx / 12) + 50 * np.sin(2 * np.pi * yy / 12)).astype(np.float32)


def status_cases():
    """(name, img1, img2, row, parameters, expected status): every status of the contract"""
    a, b = K.analytic_pair("up")
    good = K.displaced(K.true_rows(1, 5), 6)[0]
    flat = np.array(a)
    flat[20:60, 20:70] = 77.0
    g = _grating()
    eye3 = 3 * np.eye(2)
    nan_row = good.copy(); nan_row[4] = np.nan
    inf_row = good.copy(); inf_row[13] = np.inf
    return [
        ("converges", a, b, good, L.params(), L.OK),
        ("constant window", flat, flat, K.frame_row((45, 40), eye3, (45.4, 40.2), eye3), L.params(), L.FLAT),
        ("template over the border", a, b, K.frame_row((9.5, 40), eye3, (30, 50), 3 * K.A_TRUE), L.params(), L.OUTSIDE),
        ("search window over the border", a, b, K.frame_row((48, 40), eye3, (57, 56), 3 * K.A_TRUE), L.params(), L.OUTSIDE),
        ("mirrored frame", a, b, K.frame_row((48, 40), eye3, (32, 56), np.array([[3.0, 0], [0, -3.0]])), L.params(), L.BAD_FRAME),
        ("NaN frame", a, b, nan_row, L.params(), L.BAD_FRAME),
        ("infinite scale", a, b, inf_row, L.params(), L.BAD_FRAME),
        ("singular frame", a, b, K.frame_row((48, 40), eye3, (32, 56), eye3) * np.r_[np.ones(6), 0.0, np.ones(7)], L.params(), L.BAD_FRAME),
        ("magnification", a, b, K.frame_row((48, 40), eye3, (32, 56), 27 * np.eye(2)), L.params(), L.BAD_FRAME),
        ("half a period off", g, g, K.frame_row((48, 40), eye3, (54, 40), eye3), L.params(), L.DIVERGED),
        ("half a period off in both", g, g, K.frame_row((48, 40), eye3, (54, 46), eye3), L.params(), L.LOW_ZNCC),
        ("one iteration", a, b, good, L.params(max_iter=1), L.MAXITER),
    ]


@pytest.mark.parametrize("case", status_cases(), ids=lambda c: c[0])
def test_every_status_is_reachable(case):
    name, a, b, row, par, want = case
    out, st, it, zb, za = L.refine_row(a, b, row, par)
    assert st == want, (name, L.STATUS_NAMES[st])
    if st in (L.OK, L.MAXITER):
        assert not np.array_equal(out, row) and np.array_equal(out[:7], row[:7])
        assert it == (1 if st == L.MAXITER else it) and it >= 1
    else:
        assert np.array_equal(out, row, equal_nan=True)          # a rejected row comes back as it went in


def test_rejections_report_what_was_computed():
    cases = {c[0]: c for c in status_cases()}
    _, a, b, row, par, _ = cases["half a period off"]
    _, st, it, zb, za = L.refine_row(a, b, row, par)
    assert st == L.DIVERGED and it > 1 and zb < 0 and za != 0
    _, a, b, row, par, _ = cases["NaN frame"]
    assert L.refine_row(a, b, row, par)[2:] == (0, 0.0, 0.0)


# ---- the role rule

@pytest.mark.parametrize("k,swapped", [(1 - 1e-9, True), (1.0, False), (1 + 1e-9, False)])
def test_roles_at_the_boundary(k, swapped):
    """det B0 just below 1, exactly 1 and just above: the template is taken where the region is smaller, image 1 on a tie"""
    a, _ = K.analytic_pair("up")
    row = K.frame_row((48.0, 40.0), 3 * np.eye(2), (48.3, 40.2), 3 * k * np.eye(2))
    assert L.roles(row)[0] == swapped
    out, st, it, zb, za = L.refine_row(a, a, row)
    assert st == L.OK
    moved, kept = (out[:7], out[7:]) if swapped else (out[7:], out[:7])
    assert np.array_equal(kept, row[7:] if swapped else row[:7]) and not np.array_equal(moved, row[:7] if swapped else row[7:])
    # the same image twice: the refined centres coincide
    assert np.hypot(out[0] - out[7], out[1] - out[8]) < 0.01


# ---- the yardstick of the GPU test

def _max_diff(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.nanmax(np.abs(x - y))) if x.size else 0.0


def test_summation_spread_is_what_the_gpu_test_assumes():
    """forward against reversed window sums over every group of the GPU test: equal statuses and iteration counts (no case sits on
    the eps_shift boundary), and a spread of at most lsm_cases.SPREAD - and not ten times less, so the figure is not a loose one"""
    worst = 0.0
    seen = set()
    for name, kind, rows, kw in K.groups():
        a, b = K.images_of(kind)
        f, r = L.refine(a, b, rows, L.params(**kw)), L.refine(a, b, rows, L.params(**kw), "reverse")
        assert np.array_equal(f[2], r[2]) and np.array_equal(f[3], r[3]), name
        worst = max(worst, _max_diff(f[0], r[0]), _max_diff(f[4], r[4]), _max_diff(f[5], r[5]))
        seen |= set(f[2].tolist())
    print("\nspread %.3g" % worst)
    assert seen == set(range(7))                    # every status occurs in the GPU test's lists
    assert K.SPREAD / 10 < worst <= K.SPREAD
    worst = 0.0
    for name, kind, row, kw in K.seam_cases():
        a, b = K.images_of(kind)
        t1, t2 = {}, {}
        L.refine_row(a, b, row, L.params(**kw), "forward", t1)
        L.refine_row(a, b, row, L.params(**kw), "reverse", t2)
        for q in ("N", "g", "a", "delta"):
            worst = max(worst, _max_diff(t1[q], t2[q]) / np.abs(t1[q]).max())
    print("seam spread %.3g" % worst)
    assert K.SEAM_SPREAD / 10 < worst <= K.SEAM_SPREAD


# ---- the synthetic planar pair of the GPU test

@pytest.mark.skipif(not refdeg.available(), reason="oracle/_ref not built")
def test_synthetic_pair_seed_meets_the_conditions():
    """synth.pair at 400 x 300 through the oracle pipeline: the restatement lowers the median ground-truth transfer error of the
    verified rows it accepts, and rejects few.  Measured: 216 verified rows, 1 MAXITER, none rejected; median 0.234 -> 0.042 px"""
    import orc
    import pipeline_oracle as po
    import synth
    a, b, H = synth.pair(400, 300, seed=K.PAIR_SEED)
    want = po.match_pair(a, b, seed_time=K.PAIR_SEED_TIME)
    ra, rb = want["regions"]
    un = orc.duplicate_filter(po.match_fginn_par(ra, rb, 0.8), ra, rb, 2.0, 1)
    laf = po.laf_of(ra, rb, un)[want["mask"]]
    assert len(laf) == want["n_inliers"] > 100
    out, u6, st, it, zb, za = L.refine(a, b, laf)
    acc = st <= L.MAXITER
    e0, e1 = K.homography_error(H, laf[acc]), K.homography_error(H, out[acc])
    print("\n%d verified rows, statuses %s, median transfer error %.3f -> %.3f px" % (len(laf), np.bincount(st, minlength=7), np.median(e0), np.median(e1)))
    assert np.median(e1) < np.median(e0)
    assert (~acc).sum() == K.PAIR_REJECTED
    assert np.array_equal(out[~acc], laf[~acc])


# ---- the model refit

def test_refit_homography_is_the_least_squares_fit(pkg):
    rng = np.random.default_rng(11)
    H = np.array([[0.9, 0.12, 14.0], [-0.08, 1.05, -6.0], [2e-4, -1e-4, 1.0]])
    p1 = rng.uniform(0, 400, (30, 2))
    q = np.c_[p1, np.ones(30)] @ H.T
    p2 = q[:, :2] / q[:, 2:]
    u6 = np.c_[p1, np.ones(30), p2, np.ones(30)]
    got = pkg.refit_model(u6, 0).reshape(3, 3)
    # numpy: the DLT's least-squares solution (smallest right singular vector of the normalised design matrix)
    def norm(p):
        c, s = p.mean(0), np.sqrt(2) / np.hypot(*(p - p.mean(0)).T).mean()
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    T1, T2 = norm(p1), norm(p2)
    a1, a2 = np.c_[p1, np.ones(30)] @ T1.T, np.c_[p2, np.ones(30)] @ T2.T
    rows = []
    for (x, y, w), (u, v, _) in zip(a1, a2):
        rows += [[x, y, w, 0, 0, 0, -u * x, -u * y, -u * w], [0, 0, 0, x, y, w, -v * x, -v * y, -v * w]]
    h = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    want = np.linalg.inv(T2) @ h @ T1
    for M in (got, want):
        assert np.abs(M / M[2, 2] - H).max() < 1e-8
    assert np.abs(got / got[2, 2] - want / want[2, 2]).max() < 1e-8
    # four rows: the exact solution
    got4 = pkg.refit_model(u6[[0, 7, 13, 22]], 0).reshape(3, 3)
    assert np.abs(got4 / got4[2, 2] - H).max() < 1e-6


def test_refit_fundamental_matrix_is_the_least_squares_fit(pkg):
    rng = np.random.default_rng(3)
    X = np.c_[rng.uniform(-1, 1, (40, 2)), rng.uniform(4, 8, 40)]
    Kc = np.array([[500, 0, 200], [0, 500, 150], [0, 0, 1.0]])
    ca, sa, cb, sb = np.cos(0.1), np.sin(0.1), np.cos(-0.05), np.sin(-0.05)
    Rm = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    t = np.array([0.5, 0.1, 0.2])
    h1, h2 = (Kc @ X.T).T, (Kc @ (Rm @ X.T + t[:, None])).T
    h1, h2 = h1 / h1[:, 2:], h2 / h2[:, 2:]
    got = pkg.refit_model(np.c_[h1, h2], 1).reshape(3, 3)         # read row-major: x2^T M x1 = 0
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(Kc).T @ tx @ Rm @ np.linalg.inv(Kc)
    # numpy: the 8-point least-squares solution, projected to rank 2
    D = np.array([np.outer(b, a).ravel() for a, b in zip(h1, h2)])
    f = np.linalg.svd(D)[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(f)
    want = U @ np.diag([S[0], S[1], 0]) @ Vt
    unit = lambda M: M / np.linalg.norm(M) * np.sign(M[2, 2])
    assert np.abs(np.einsum("ni,ij,nj->n", h2, got, h1)).max() < 1e-9 * np.abs(got).max() * 500 * 500
    assert np.abs(unit(got) - unit(F)).max() < 1e-7 and np.abs(unit(got) - unit(want)).max() < 1e-7
    assert abs(np.linalg.det(unit(got))) < 1e-12


def test_refit_refusals(pkg):
    u = np.zeros((8, 6))
    for args, part in (((None, 8, 0, BUF), "null"), ((BUF, 8, 0, None), "null"), ((BUF, 8, 2, BUF), "model_type"), ((BUF, 3, 0, BUF), "3 rows"),
                       ((BUF, 7, 1, BUF), "7 rows")):
        rc = pkg.lib().mods_refit_model(*args)
        err = pkg.lib().mods_last_error().decode()
        assert rc == E_ARG and err.startswith("refit_model: ") and part in err, (rc, err)
    with pytest.raises(pkg.ModsError):
        pkg.refit_model(u[:3], 0)


# ---- symbols, defaults and the refusals that need no device

def test_symbols_defaults_and_stage(pkg):
    header = open(os.path.join(ROOT, "include", "mods_hip.h")).read()
    for name in NAMES:
        assert hasattr(pkg.lib(), name) and name + "(" in header, name
    assert header.index("MODS_STAGE_DISTRACTOR_SWEEP,") < header.index("MODS_STAGE_REFINE,") < header.index("MODS_STAGE_COUNT")
    assert pkg.stage_index("refine") == pkg.stage_index("distractor_sweep") + 1
    p = pkg.lsm_defaults()
    got = dict(radius=p.radius, max_iter=p.max_iter, eps_shift=p.eps_shift, max_shift=p.max_shift, max_scale_change=p.max_scale_change,
               max_magnification=p.max_magnification, min_zncc=p.min_zncc, lam=p.lam, affine=p.affine)
    assert got == L.DEFAULTS
    assert pkg.LSM_STATUS == L.STATUS_NAMES
    assert C.sizeof(pkg.LsmParams) == 64


REFUSED = [
    (dict(radius=0), {}, "radius"), (dict(radius=16), {}, "radius"), (dict(max_iter=0), {}, "max_iter"),
    (dict(eps_shift=0.0), {}, "eps_shift"), (dict(eps_shift=float("nan")), {}, "eps_shift"), (dict(max_shift=-1.0), {}, "max_shift"),
    (dict(max_shift=float("inf")), {}, "max_shift"), (dict(lam=0.0), {}, "lambda"), (dict(max_scale_change=0.5), {}, "max_scale_change"),
    (dict(max_magnification=float("nan")), {}, "max_magnification"), (dict(min_zncc=1.5), {}, "min_zncc"),
    (dict(min_zncc=float("nan")), {}, "min_zncc"), (dict(affine=2), {}, "affine"),
    ({}, dict(n=-1), "n = -1"), ({}, dict(stride1=95), "stride"), ({}, dict(stride2=63), "stride"), ({}, dict(w1=1), "image size"),
    ({}, dict(img1=None), "null"), ({}, dict(img2=None), "null"), ({}, dict(laf=None), "null"), ({}, dict(ctx=None), "null"),
]


@pytest.mark.parametrize("entry", ["mods_refine_matches", "mods_refine_matches_dev"])
@pytest.mark.parametrize("par_kw,arg_kw,part", REFUSED, ids=[r[2] + str(i) for i, r in enumerate(REFUSED)])
def test_refusals_before_any_device_call(pkg, entry, par_kw, arg_kw, part):
    """no context exists in this process and no pointer is valid: a call that got past its checks would crash"""
    a = dict(ctx=BUF, img1=BUF, w1=96, h1=80, stride1=96, img2=BUF, w2=64, h2=112, stride2=64, laf=BUF, n=3)
    a.update(arg_kw)
    par = pkg.lsm_defaults(**par_kw)
    rc = getattr(pkg.lib(), entry)(a["ctx"], a["img1"], a["w1"], a["h1"], a["stride1"], a["img2"], a["w2"], a["h2"], a["stride2"], a["laf"],
                                   a["n"], C.byref(par), None, None, None, None, None, None)
    err = pkg.lib().mods_last_error().decode()
    assert rc == E_ARG and err.startswith("refine_matches: ") and part in err, (rc, err)


def test_an_empty_list_launches_nothing(pkg):
    """n == 0 with arguments that would crash if they were used: MODS_OK"""
    for entry in ("mods_refine_matches", "mods_refine_matches_dev"):
        assert getattr(pkg.lib(), entry)(BUF, BUF, 96, 80, 96, BUF, 64, 112, 64, None, 0, None, None, None, None, None, None, None) == 0
    rc = pkg.lib().mods_test_lsm_iteration(None, BUF, 96, 80, 96, BUF, 64, 112, 64, BUF, None, BUF, BUF, BUF, BUF, BUF)
    assert rc == E_ARG
