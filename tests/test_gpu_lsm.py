"""-m gpu: the least-squares refinement kernel (csrc/refine.hip) against the numpy restatement of its contract (tests/lsm_ref.py), on
images of 96 x 80 and 64 x 112 with row strides of 104 and 67 floats (tests/lsm_cases.py).

Yardstick.  numpy's summation order is not the kernel's, so the restatement is run with its window sums forward and reversed; the
largest difference between the two runs over the cases of this file is lsm_cases.SPREAD = 3.05e-12 (measured on the CPU and held
there by tests/test_cpu_lsm.py; it comes from the 3 x 3 windows, the 21 x 21 ones give 7.1e-15).  The kernel may differ from the
forward run by ten times that in a coordinate, a frame entry or a zncc value; statuses and iteration counts must be equal, and a
rejected row must come back to the bit.  The seam's N, g, a and delta: ten times lsm_cases.SEAM_SPREAD = 1.3e-14 of the largest
entry of each."""
import ctypes as C

import numpy as np
import pytest

import lsm_cases as K
import lsm_ref as L

pytestmark = pytest.mark.gpu
TOL = 10 * K.SPREAD
SEAM_TOL = 10 * K.SEAM_SPREAD
KEYS = ("laf", "u6", "status", "iterations", "zncc_before", "zncc_after")


@pytest.fixture(scope="module")
def ref():
    """the restatement's forward run of every group, computed once: name -> (img1, img2, rows, parameter overrides, result)"""
    out = {}
    for name, kind, rows, kw in K.groups():
        a, b = K.images_of(kind)
        out[name] = (a, b, rows, kw, L.refine(a, b, rows, L.params(**kw)))
    return out


def check(got, want, rows, n=None, tag=""):
    laf, u6, st, it, zb, za = (w[:n] for w in want)
    assert np.array_equal(got["status"], st), (tag, got["status"], st)
    assert np.array_equal(got["iterations"], it), (tag, got["iterations"], it)
    acc = st <= L.MAXITER
    worst = 0.0
    if acc.any():
        worst = max(np.abs(got["laf"][acc] - laf[acc]).max(), np.abs(got["u6"][acc] - u6[acc]).max())
    worst = max(worst, np.abs(got["zncc_before"] - zb).max(), np.abs(got["zncc_after"] - za).max())
    print("%s: %d rows, largest difference %.3g (allowed %.3g)" % (tag, len(st), worst, TOL))
    assert worst <= TOL, (tag, worst)
    assert got["laf"][~acc].tobytes() == laf[~acc].tobytes(), tag           # rejected: exactly as it went in
    for i in np.nonzero(acc)[0]:                                            # accepted: the template side is untouched
        s = slice(7, 14) if L.roles(rows[i])[0] else slice(0, 7)
        assert got["laf"][i, s].tobytes() == rows[i, s].tobytes(), (tag, i)
    assert np.array_equal(got["u6"], L.u6_of(got["laf"]))


def run(pkg, ctx, name, ref, n=None):
    a, b, rows, kw, want = ref[name]
    got = ctx.refine_matches(a, b, rows[:n], pkg.lsm_defaults(**kw))
    check(got, want, rows, n, "%s n=%s" % (name, n))
    return got


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_list_lengths(pkg, gpu_ctx, ref, n):
    """one wave, the workgroup edge (four rows per workgroup), the grid tail"""
    run(pkg, gpu_ctx, "r10", ref, n)


@pytest.mark.parametrize("name", ["r1", "r3", "r4", "r15"])
def test_radii(pkg, gpu_ctx, ref, name):
    """9 and 49 samples leave lanes idle, 81 is the first to give lanes two samples, 15 is the cap (16 samples per lane)"""
    run(pkg, gpu_ctx, name, ref)


@pytest.mark.parametrize("name", ["down r10", "down r4", "translation", "one iteration"])
def test_roles_and_modes(pkg, gpu_ctx, ref, name):
    got = run(pkg, gpu_ctx, name, ref)
    rows = ref[name][2]
    if name.startswith("down"):               # image 2 holds the template: side 1 moved
        ok = got["status"] <= L.MAXITER
        assert ok.any() and (got["laf"][ok, :7] != rows[ok, :7]).any(axis=1).all()
    if name == "one iteration":
        assert (got["status"] == L.MAXITER).all() and (got["iterations"] == 1).all()


def test_mixed_statuses_in_one_list(pkg, gpu_ctx, ref):
    """every status of the contract in one list: the waves of a workgroup leave at different iterations"""
    got = run(pkg, gpu_ctx, "mixed", ref)
    assert set(got["status"].tolist()) == set(range(7))


@pytest.mark.parametrize("case", K.seam_cases(), ids=lambda c: c[0])
def test_one_iteration_through_the_seam(pkg, gpu_ctx, case):
    name, kind, row, kw = case
    a, b = K.images_of(kind)
    t = {}
    L.refine_row(a, b, row, L.params(**kw), "forward", t)
    N, g, gain, delta, st = pkg.test_lsm_iteration(gpu_ctx, a, b, row, pkg.lsm_defaults(**kw))
    P = len(t["g"])
    assert st not in (L.BAD_FRAME, L.OUTSIDE, L.FLAT)
    assert not N[P:, :].any() and not N[:, P:].any() and not g[P:].any() and not delta[P:].any()
    for q, got, want in (("N", N[:P, :P], t["N"]), ("g", g[:P], t["g"]), ("a", gain, t["a"]), ("delta", delta[:P], t["delta"])):
        d = np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max()
        print("%s %s: relative difference %.3g (allowed %.3g)" % (name, q, d, SEAM_TOL))
        assert d <= SEAM_TOL, (name, q, d)
    assert np.array_equal(N, N.T)


def _bits(got):
    return tuple(got[k].tobytes() for k in KEYS)


@pytest.mark.parametrize("name", ["mixed", "r10", "r15"])
def test_determinism_to_the_bit(pkg, gpu_ctx, ref, name):
    """a row's result with the list refined as a whole, reversed, one row at a time, and twice in a row on one context"""
    a, b, rows, kw, _ = ref[name]
    rows = rows[:24]
    par = pkg.lsm_defaults(**kw)
    whole = gpu_ctx.refine_matches(a, b, rows, par)
    again = gpu_ctx.refine_matches(a, b, rows, par)
    assert _bits(whole) == _bits(again)
    rev = gpu_ctx.refine_matches(a, b, rows[::-1], par)
    assert _bits({k: rev[k][::-1].copy() for k in KEYS}) == _bits(whole)
    for i in range(len(rows)):
        one = gpu_ctx.refine_matches(a, b, rows[i:i + 1], par)
        assert _bits(one) == _bits({k: whole[k][i:i + 1].copy() for k in KEYS}), i


def test_device_images_with_strides_and_null_outputs(pkg, gpu_ctx, ref):
    """mods_refine_matches_dev on strided device images gives the host entry point's bits; any output may be null"""
    import torch
    a, b, rows, kw, _ = ref["mixed"]
    par = pkg.lsm_defaults(**kw)
    want = gpu_ctx.refine_matches(a, b, rows, par)
    ta = torch.full((K.H1, K.STRIDE1), float("nan")); ta[:, :K.W1] = torch.from_numpy(np.array(a))
    tb = torch.full((K.H2, K.STRIDE2), float("nan")); tb[:, :K.W2] = torch.from_numpy(np.array(b))
    ta, tb = ta.cuda(), tb.cuda()
    torch.cuda.synchronize()
    got = gpu_ctx.refine_matches_dev(ta.data_ptr(), K.W1, K.H1, K.STRIDE1, tb.data_ptr(), K.W2, K.H2, K.STRIDE2, rows, par)
    assert _bits(got) == _bits(want)
    st = np.full(len(rows), -1, np.int32)
    rc = pkg.lib().mods_refine_matches_dev(gpu_ctx.h, C.c_void_p(ta.data_ptr()), K.W1, K.H1, K.STRIDE1, C.c_void_p(tb.data_ptr()), K.W2, K.H2,
                                           K.STRIDE2, rows.ctypes.data_as(C.c_void_p), len(rows), None, None, None,
                                           st.ctypes.data_as(C.c_void_p), None, None, None)
    dflt = gpu_ctx.refine_matches(a, b, rows)
    assert rc == 0 and np.array_equal(st, dflt["status"]) and not np.array_equal(st, want["status"])    # par == NULL: the defaults
    assert len(gpu_ctx.refine_matches(a, b, rows[:0])["status"]) == 0       # n == 0


def test_stage_timer(pkg, gpu_ctx, ref):
    a, b, rows, kw, _ = ref["r10"]
    try:
        gpu_ctx.timing_enable(["refine"]); gpu_ctx.timing_reset()
        gpu_ctx.refine_matches(a, b, rows, pkg.lsm_defaults(**kw))
        gpu_ctx.refine_matches(a, b, rows[:0], pkg.lsm_defaults(**kw))       # launches nothing
        ms, n, _ = gpu_ctx.timing_read("refine")
        assert n == 1 and ms > 0
    finally:
        gpu_ctx.timing_enable([])


def test_a_search_made_before_is_fetched_unchanged_after(pkg, gpu_ctx, ref):
    rng = np.random.default_rng(5)
    q = np.zeros(300, pkg.REGION_DTYPE)
    q["x"], q["y"] = rng.uniform(0, 600, 300), rng.uniform(0, 400, 300)
    q["s"], q["a11"], q["a22"] = rng.uniform(2, 6, 300), 1.0, 1.0
    q["desc"] = rng.integers(0, 256, (300, 128))
    t = q.copy()
    t["x"] += 3.0
    t["desc"] = np.clip(q["desc"].astype(np.int32) + rng.integers(-3, 4, (300, 128)), 0, 255)
    tent, u6 = gpu_ctx.match_fginn(q, t, 0.9)
    laf = gpu_ctx.last_laf.copy()
    assert len(tent) > 100
    run(pkg, gpu_ctx, "mixed", ref)
    cap = len(q)
    tent2 = np.zeros(cap, pkg.TENT_DTYPE); u62 = np.zeros((cap, 6)); laf2 = np.zeros((cap, 14))
    n = C.c_int(-1)
    assert pkg.lib().mods_match_fetch_internal(gpu_ctx.h, tent2.ctypes.data_as(C.c_void_p), u62.ctypes.data_as(C.c_void_p),
                                               laf2.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    assert n.value == len(tent) and tent2[:n.value].tobytes() == tent.tobytes()
    assert np.array_equal(u62[:n.value], u6) and np.array_equal(laf2[:n.value], laf)


def test_synthetic_planar_pair_end_to_end(pkg):
    """synth.pair at 400 x 300 (the seed tests/test_cpu_lsm.py examines with the oracle pipeline): the verified frames of
    mods_match_pair_dev refined on the device images.  Conditions, not accuracy figures: the median ground-truth transfer error of the
    refined rows is below that of the same rows unrefined, and no more rows are rejected than the restatement rejects"""
    import torch
    import synth
    w, h = 400, 300
    a, b, H = synth.pair(w, h, seed=K.PAIR_SEED)
    ctx = pkg.Context(0, w, h, 2)
    try:
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        pkg.ransac_pin_seed(K.PAIR_SEED_TIME)
        res, m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, max_matches=100000)
        laf = ctx.verified_lafs()
        assert len(laf) == res.n_inliers > 100 and np.array_equal(laf[:, [0, 1, 7, 8]], m)
        got = ctx.refine_matches_dev(t.data_ptr(), w, h, w, t.data_ptr() + 4 * w * h, w, h, w, laf)
        acc = got["status"] <= L.MAXITER
        e0, e1 = K.homography_error(H, laf[acc]), K.homography_error(H, got["laf"][acc])
        print("%d verified rows, statuses %s, median transfer error %.3f -> %.3f px, zncc %.3f -> %.3f"
              % (len(laf), np.bincount(got["status"], minlength=7), np.median(e0), np.median(e1), got["zncc_before"][acc].mean(),
                 got["zncc_after"][acc].mean()))
        assert np.median(e1) < np.median(e0)
        assert (~acc).sum() <= K.PAIR_REJECTED
        assert len(got["laf"]) == len(laf) and np.array_equal(got["laf"][~acc], laf[~acc])
        # refined matches + refit model, without another RANSAC run
        Hr = pkg.refit_model(got["u6"], 0)
        assert np.isfinite(Hr).all() and abs(Hr[8]) > 0
    finally:
        pkg.ransac_pin_seed(-1)
        ctx.close()
