"""-m gpu: guided matching (mods_match_guided / mods_match_guided_reps, csrc/guided.hip) against the numpy restatement of its
contract (tests/guided_ref.py).  Every case demands equality to the bit of q, t, t_bad, d1, d2, the ratio's bits, u6, laf and the
count."""
import os
import subprocess

import numpy as np
import pytest

import guided_ref as gr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
H_PROJ = np.array([[0.93, -0.11, 21.5], [0.07, 1.04, -13.25], [1.1e-4, -6.0e-5, 1.0]])


def regions(rng, xy, desc=None):
    n = len(xy)
    r = np.zeros(n, gr.REGION_DTYPE)
    if n:
        r["x"], r["y"] = np.asarray(xy, np.float64).T
    r["s"] = rng.uniform(1.5, 30.0, n)
    for f in ("a11", "a12", "a21", "a22", "response"):
        r[f] = rng.standard_normal(n)
    r["id"] = np.arange(n); r["sub_type"] = rng.integers(0, 3, n)
    r["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8) if desc is None else desc
    return r


def near_desc(rng, desc, amp):
    return np.clip(desc.astype(np.int64) + rng.integers(-amp, amp + 1, desc.shape), 0, 255).astype(np.uint8)


def apply_h(H, xy):
    p = np.c_[xy, np.ones(len(xy))] @ np.asarray(H).T
    return p[:, :2] / p[:, 2:]


def scene(rng, n_q, n_t, transfer, w=400.0, h=300.0, noise=3.0):
    """queries anywhere in w x h; the first trains are partners of queries (transfer(xy) plus noise, descriptors nearby), some
    queries with two partners (the same structure seen in two views), the rest are clutter; trains in random order"""
    if not callable(transfer):
        H = transfer
        transfer = lambda xy: apply_h(H, xy)
    qxy = rng.uniform(0, 1, (n_q, 2)) * (w, h)
    q = regions(rng, qxy)
    txy = rng.uniform(0, 1, (n_t, 2)) * (w, h)
    tdesc = rng.integers(0, 256, (n_t, 128), dtype=np.uint8)
    m = min(n_q, (2 * n_t) // 3)
    if m:
        src = rng.integers(0, n_q, m)
        txy[:m] = transfer(qxy[src]) + rng.uniform(-noise, noise, (m, 2))
        tdesc[:m] = near_desc(rng, q["desc"][src], 12)
    perm = rng.permutation(n_t)
    return q, regions(rng, txy[perm], tdesc[perm])


def fundamental(rng):
    """a random rank-2 F = [e]x A (x2^T F x1 = 0 whenever x2 ~ A x1 + lambda e), its layout for the library - degensac's
    F[3 * c + r] = entry (r, c) - and the transfer that puts a partner on its epipolar line"""
    e = np.array([rng.uniform(500, 900), rng.uniform(-400, -100), 1.0])
    ex = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    A = np.eye(3) + 0.05 * rng.standard_normal((3, 3)); A[:2, 2] = rng.uniform(-10, 10, 2); A[2] = (1e-4, -2e-4, 1.0)
    F = ex @ A
    F /= np.abs(F).max()

    def transfer(xy):
        p = np.c_[xy, np.ones(len(xy))] @ A.T + rng.uniform(-0.1, 0.1, (len(xy), 1)) * e[None, :]
        return p[:, :2] / p[:, 2:]
    return np.ascontiguousarray(F.T).reshape(9), transfer


def params(pkg, model, **kw):
    a = dict(model_type=0, radius=4.0, ratio=0.9, contrad=2.5, max_dist=0, one_to_one=0)
    a.update(kw)
    return pkg.GuidedParams.default(model, **a), a


def ref_of(q, t, model, a):
    return gr.guided_ref(q, t, a["model_type"], model, a["radius"], a["ratio"], a["contrad"], a["max_dist"], a["one_to_one"])


def assert_same(got, want, what=""):
    (gt, gu, gl), (wt, wu, wl) = got, want
    assert len(gt) == len(wt), (what, len(gt), len(wt))
    for f in ("q", "t", "t_bad", "t_2nd", "d1", "d2", "d2nd"):
        assert np.array_equal(gt[f], wt[f]), (what, f)
    assert np.array_equal(gt["ratio"].view(np.uint64), wt["ratio"].view(np.uint64)), (what, "ratio bits")
    assert np.array_equal(gu.view(np.uint64), wu.view(np.uint64)), (what, "u6")
    assert np.array_equal(gl.view(np.uint64), wl.view(np.uint64)), (what, "laf")


def check(pkg, ctx, q, t, model, what="", **kw):
    p, a = params(pkg, model, **kw)
    got = ctx.match_guided(q, t, p)
    want = ref_of(q, t, model, a)
    assert_same(got, want, what)
    return got


@pytest.mark.parametrize("n_q,n_t", [(0, 5), (5, 0), (1, 1), (63, 65), (300, 257), (5000, 4099)])
@pytest.mark.parametrize("mode", [0, 1])
def test_tile_tails(pkg, gpu_ctx, n_q, n_t, mode):
    """list lengths around the 256-wide query blocks and train tiles; (5000, 4099) spans 20 query blocks and several train splits"""
    rng = np.random.default_rng(100 + n_q + n_t)
    model, transfer = (H_PROJ.reshape(9), H_PROJ) if mode == 0 else fundamental(rng)
    q, t = scene(rng, n_q, n_t, transfer)
    got = check(pkg, gpu_ctx, q, t, model, model_type=mode, radius=6.0 if mode == 0 else 3.0, one_to_one=n_q % 2)
    if n_q >= 300:
        assert len(got[0]) > 10 and (got[0]["t_bad"] >= 0).any() and (got[0]["t_bad"] < 0).any()
    if (n_q, n_t) == (1, 1):
        q1 = regions(rng, [(50.0, 60.0)]); t1 = regions(rng, apply_h(H_PROJ, [(50.0, 60.0)]))
        if mode == 0:
            assert len(check(pkg, gpu_ctx, q1, t1, H_PROJ.reshape(9), radius=0.5)[0]) == 1


def _same_bits(got, want, what):
    """two answers of one search, part by part: every field of every row to the bit, and the counts of the overlap searches"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if not isinstance(g, np.ndarray):
            assert (g.n_q_common, g.n_t_common, g.n_matches) == (w.n_q_common, w.n_t_common, w.n_matches), what
            assert np.float64(g.repeatability).view(np.uint64) == np.float64(w.repeatability).view(np.uint64), (what, "repeatability bits")
            continue
        assert g.shape == w.shape, (what, g.shape, w.shape)
        for f in g.dtype.names or (slice(None),):
            assert g[f].dtype == w[f].dtype and g[f].tobytes() == w[f].tobytes(), (what, f)


def test_searches_interleaved_on_one_context(pkg):
    """the three searches of two host lists alternate on one context, with list lengths that grow and shrink: they stage their lists
    in one buffer (csrc/list_search.hpp), which is so reallocated and reused between different searches.  Every answer equals the
    answer of the same call alone on a fresh context and the numpy reference"""
    import overlap_area_ref as oar
    import overlap_ref as orf

    def guided(n_q, n_t):
        q, t = scene(np.random.default_rng(100 + n_q + n_t), n_q, n_t, H_PROJ)        # (the scenes of test_tile_tails)
        p, a = params(pkg, H_PROJ.reshape(9), radius=6.0, one_to_one=1)
        return (lambda ctx: ctx.match_guided(q, t, p)), ref_of(q, t, H_PROJ.reshape(9), a), 0 if n_q < 300 else 10

    def overlap(n_q, n_t):
        q, t = orf.scene(np.random.default_rng(100 + n_q + n_t), n_q, n_t)
        p = pkg.OverlapParams.default(H_PROJ, one_to_one=1, w1=400, h1=300, w2=400, h2=300)
        want = orf.overlap_ref(q, t, orf.params(H_PROJ, one_to_one=1, w1=400, h1=300, w2=400, h2=300))
        return (lambda ctx: ctx.match_overlap(q, t, p)), want, 0

    def area(seed, n_q, n_t, mode):
        q, t = orf.scene(np.random.default_rng(seed), n_q, n_t)
        p = pkg.OverlapAreaParams.default(H_PROJ, one_to_one=mode)
        return (lambda ctx: ctx.match_overlap_area(q, t, p)), oar.overlap_area_ref(q, t, oar.params(H_PROJ, 0.4, mode)), 10

    first = [guided(300, 257), overlap(63, 65), area(7, 257, 131, 1)]
    calls = first + [guided(5000, 4099), overlap(1, 1), area(11, 300, 301, 2)] + first
    alone = []
    for call, want, least in calls[:6]:
        ctx = pkg.Context(0, 640, 480, 1)
        try:
            alone.append(call(ctx))
        finally:
            ctx.close()
        assert len(alone[-1][0]) >= least                            # (an empty answer cannot pass)
        _same_bits(alone[-1], want, "call %d alone against the reference" % len(alone))
    ctx = pkg.Context(0, 640, 480, 1)
    try:
        for i, (call, want, _) in enumerate(calls):
            _same_bits(call(ctx), alone[i % 6], "call %d of the sequence" % i)
    finally:
        ctx.close()


def test_h_exact_boundaries(pkg, gpu_ctx):
    """translation by (3, 4) or (-5, 12) on a quarter-pixel lattice: every product and sum of the gate is exact, so many pairs sit
    exactly at distance r (3-4-5 and 5-12-13 offsets) - the <= of the forward and of the backward test decides them"""
    rng = np.random.default_rng(7)
    cases = (((3.0, 4.0), 5.0, [(3, 4), (-3, 4), (4, -3), (5, 0), (0, -5), (-4, -3), (5.25, 0), (3, 4.25)]),
             ((-5.0, 12.0), 3.25, [(3.25, 0), (0, -3.25), (1.25, 3), (-3, 1.25), (3.5, 0), (1.25, 3.25)]))
    for (tx, ty), r, ring in cases:
        H = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
        qxy = np.round(rng.uniform(0, 60, (700, 2)) * 4) / 4
        txy = np.round(rng.uniform(0, 60, (900, 2)) * 4) / 4 + (tx, ty)
        # partners exactly on the circle of radius r around the transferred point, and just outside it on the lattice
        ring = np.array(ring)
        src = rng.integers(0, 700, 400)
        txy[:400] = qxy[src] + (tx, ty) + ring[rng.integers(0, len(ring), 400)]
        q = regions(rng, qxy); t = regions(rng, txy)
        t["desc"][:400] = near_desc(rng, q["desc"][src], 10)
        g = gr.gate_rows(0, H.reshape(9), r, q, t, 0, len(q))
        dx = (q["x"][:, None] + tx) - t["x"][None, :]; dy = (q["y"][:, None] + ty) - t["y"][None, :]
        on = (dx * dx + dy * dy == r * r)
        assert on.sum() > 150 and g[on].all()                      # pairs exactly on the radius exist and are inside
        got = check(pkg, gpu_ctx, q, t, H.reshape(9), radius=r, ratio=1.0, contrad=0.0)
        assert on[got[0]["q"], got[0]["t"]].sum() > 20             # ... and some of them are chosen
        check(pkg, gpu_ctx, q, t, H.reshape(9), radius=float(np.nextafter(r, 0.0)), ratio=1.0, contrad=0.0)


def test_h_projective(pkg, gpu_ctx):
    rng = np.random.default_rng(11)
    q, t = scene(rng, 1500, 1700, H_PROJ, noise=2.0)
    for kw in (dict(radius=3.0), dict(radius=7.5, ratio=0.8, one_to_one=1), dict(radius=1e-3), dict(radius=1e4, ratio=1.0, contrad=0.0)):
        check(pkg, gpu_ctx, q, t, H_PROJ.reshape(9), str(kw), **kw)
    # a query and a train on the line W = 0 of H / Hinv gate nothing (inf or NaN never pass)
    Hs = np.array([[1, 0, 0], [0, 1, 0], [0.01, 0, -1.0]])         # W = 0.01 x - 1: zero on x = 100
    q2 = q.copy(); q2["x"][:200] = 100.0
    got = check(pkg, gpu_ctx, q2, t, Hs.reshape(9), radius=50.0)
    assert not np.isin(got[0]["q"], np.arange(200)).any()


def test_f_mode_and_layout(pkg, gpu_ctx):
    rng = np.random.default_rng(13)
    F, transfer = fundamental(rng)
    q, t = scene(rng, 1200, 1300, transfer, noise=0.7)
    a = check(pkg, gpu_ctx, q, t, F, model_type=1, radius=1.0)
    b = check(pkg, gpu_ctx, q, t, np.ascontiguousarray(F.reshape(3, 3).T).reshape(9), model_type=1, radius=1.0)
    assert len(a[0]) > 50 and len(b[0]) > 5
    assert len(a[0]) != len(b[0]) or not np.array_equal(a[0]["t"], b[0]["t"])      # the transposed matrix is another model
    check(pkg, gpu_ctx, q, t, F, model_type=1, radius=4.0, ratio=0.7, one_to_one=1)
    check(pkg, gpu_ctx, q, t, np.zeros(9), model_type=1, radius=1.0)               # F = 0: e*e <= 0 holds everywhere, all gated


def test_ties(pkg, gpu_ctx):
    """two gated trains with one descriptor (the lower index wins, on both neighbours), two trains at one position (never each
    other's inconsistent second)"""
    rng = np.random.default_rng(17)
    H = np.eye(3).reshape(9)
    q = regions(rng, [(50, 50), (120, 50), (200, 80)])
    d = q["desc"]
    txy = [(51, 50), (49, 51), (50, 50), (50, 50), (121, 50), (121, 50), (140, 50), (141, 50), (200, 81), (230, 80), (231, 81)]
    t = regions(rng, txy)
    t["desc"][0] = t["desc"][1] = near_desc(rng, d[0:1], 3)[0]      # q0: tie between trains 0 and 1
    t["desc"][2] = t["desc"][3] = near_desc(rng, d[0:1], 40)[0]
    t["desc"][4] = t["desc"][5] = near_desc(rng, d[1:2], 3)[0]      # q1: the two best at one position, then a tie among the far ones
    t["desc"][6] = t["desc"][7] = near_desc(rng, d[1:2], 60)[0]
    t["desc"][8] = near_desc(rng, d[2:3], 3)[0]
    t["desc"][9] = t["desc"][10] = near_desc(rng, d[2:3], 50)[0]
    for contrad in (0.0, 1.0, 10.0, 25.0):
        got = check(pkg, gpu_ctx, q, t, H, radius=40.0, ratio=1.0, contrad=contrad)
    got = check(pkg, gpu_ctx, q, t, H, radius=40.0, ratio=1.0, contrad=10.0)
    assert got[0]["t"].tolist() == [0, 4, 8] and got[0]["t_bad"].tolist() == [-1, 6, 9]
    got = check(pkg, gpu_ctx, q, t, H, radius=40.0, ratio=1.0, contrad=0.0)
    # train 1 ties with the first of q0 from another position: d1 < d2 fails; train 5 shares train 4's position, so q1 keeps 6
    assert got[0]["q"].tolist() == [1, 2] and got[0]["t_bad"].tolist() == [6, 9]


def test_fginn_rule_and_max_dist(pkg, gpu_ctx):
    """candidates nearer than and farther than contradDist from t1, the ratio on either side of the decision, the cap at exactly d1"""
    rng = np.random.default_rng(19)
    H = np.eye(3).reshape(9)
    q = regions(rng, [(100, 100)], np.full((1, 128), 100, np.uint8))
    t = regions(rng, [(100, 101), (103, 100), (100, 112)], np.array([[101] * 128, [102] * 128, [104] * 128], np.uint8))
    # d = 128, 512, 2048; train 1 is 3.16 px from t1, train 2 is 11 px from it
    for contrad, bad, d2 in ((3.0, 1, 512.0), (3.5, 2, 2048.0), (11.0, -1, 0.0), (10.99, 2, 2048.0)):
        got = check(pkg, gpu_ctx, q, t, H, radius=20.0, ratio=1.0, contrad=contrad)
        assert got[0]["t_bad"].tolist() == [bad] and got[0]["d2"].tolist() == [d2] and got[0]["d1"].tolist() == [128.0]
    # d1 / d2 = 1 / 4 = 0.5^2: rho = 0.5 is the boundary (strict <), a hair above passes
    assert len(check(pkg, gpu_ctx, q, t, H, radius=20.0, ratio=0.5, contrad=3.0)[0]) == 0
    assert len(check(pkg, gpu_ctx, q, t, H, radius=20.0, ratio=float(np.nextafter(0.5, 1.0)), contrad=3.0)[0]) == 1
    assert len(check(pkg, gpu_ctx, q, t, H, radius=20.0, ratio=0.25, contrad=3.5)[0]) == 0     # 128 < 2048 / 16 is false
    assert len(check(pkg, gpu_ctx, q, t, H, radius=20.0, ratio=0.26, contrad=3.5)[0]) == 1
    for cap, n in ((128, 1), (127, 0), (129, 1), (1, 0)):
        assert len(check(pkg, gpu_ctx, q, t, H, radius=20.0, ratio=1.0, contrad=3.0, max_dist=cap)[0]) == n
    rng = np.random.default_rng(23)
    q, t = scene(rng, 900, 1000, H_PROJ)
    ref = check(pkg, gpu_ctx, q, t, H_PROJ.reshape(9), radius=8.0)
    cap = int(np.median(ref[0]["d1"]))
    got = check(pkg, gpu_ctx, q, t, H_PROJ.reshape(9), radius=8.0, max_dist=cap)
    assert 0 < len(got[0]) < len(ref[0])


def test_one_to_one(pkg, gpu_ctx):
    rng = np.random.default_rng(29)
    H = np.eye(3).reshape(9)
    base = rng.integers(20, 200, (1, 128), dtype=np.uint8)
    qd = np.repeat(base, 5, axis=0); qd[0, 0] += 3; qd[1, 0] += 1; qd[2, 0] += 1; qd[3, 0] += 2; qd[4] = 255 - base[0]
    q = regions(rng, [(10, 10), (11, 10), (10, 11), (11, 11), (300, 300)], qd)
    t = regions(rng, [(10.5, 10.5), (300, 300)], np.r_[base, 255 - base])
    got = check(pkg, gpu_ctx, q, t, H, radius=5.0, one_to_one=1)
    assert got[0]["q"].tolist() == [1, 4] and got[0]["d1"].tolist() == [1.0, 0.0]      # queries 1 and 2 tie at d1 = 1: the lower stays
    assert check(pkg, gpu_ctx, q, t, H, radius=5.0, one_to_one=0)[0]["q"].tolist() == [0, 1, 2, 3, 4]
    q, t = scene(np.random.default_rng(31), 2500, 600, H_PROJ)
    a = check(pkg, gpu_ctx, q, t, H_PROJ.reshape(9), radius=8.0, ratio=1.0, one_to_one=0)
    b = check(pkg, gpu_ctx, q, t, H_PROJ.reshape(9), radius=8.0, ratio=1.0, one_to_one=1)
    assert len(np.unique(a[0]["t"])) == len(b[0]) < len(a[0]) and len(np.unique(b[0]["t"])) == len(b[0])


def test_launch_independence(pkg, gpu_ctx):
    """the same call twice, and with the trains in reverse order (another split of the work, other ties): mapped back, the same
    answer wherever the (d, t) order does not depend on the train index"""
    rng = np.random.default_rng(37)
    q, t = scene(rng, 3000, 2100, H_PROJ)
    p, a = params(pkg, H_PROJ.reshape(9), radius=6.0, one_to_one=1)
    one = gpu_ctx.match_guided(q, t, p)
    two = gpu_ctx.match_guided(q, t, p)
    assert_same(one, two, "repeat")
    assert_same(one, ref_of(q, t, H_PROJ.reshape(9), a), "reference")
    rev = gpu_ctx.match_guided(q, t[::-1].copy(), p)
    assert_same(rev, ref_of(q, t[::-1].copy(), H_PROJ.reshape(9), a), "reversed reference")
    n_t = len(t)
    # random 128-byte descriptors: no two gated trains of a query are at one distance, so the choice does not lean on the index
    assert len(rev[0]) == len(one[0])
    assert np.array_equal(rev[0]["q"], one[0]["q"]) and np.array_equal(n_t - 1 - rev[0]["t"], one[0]["t"])
    back = np.where(rev[0]["t_bad"] >= 0, n_t - 1 - rev[0]["t_bad"], -1)
    assert np.array_equal(back, one[0]["t_bad"])
    for f in ("d1", "d2", "ratio"):
        assert np.array_equal(rev[0][f], one[0][f])
    assert np.array_equal(rev[1], one[1]) and np.array_equal(rev[2], one[2])


def test_banks_equal_host_lists(pkg, gpu_ctx):
    rng = np.random.default_rng(41)
    q, t = scene(rng, 1300, 1100, H_PROJ)
    rq, rt = pkg.ImgRep(gpu_ctx, 4096), pkg.ImgRep(gpu_ctx, 4096)
    try:
        rq.append_host(q[:700]); rq.append_host(q[700:]); rt.append_host(t)
        for kw in (dict(radius=6.0), dict(radius=6.0, one_to_one=1, ratio=0.8)):
            p, a = params(pkg, H_PROJ.reshape(9), **kw)
            host = gpu_ctx.match_guided(q, t, p)
            bank = pkg.match_guided_reps(gpu_ctx, rq, rt, p)
            assert len(host[0]) > 100
            assert_same(bank, host, "banks")
            assert_same(bank, ref_of(q, t, H_PROJ.reshape(9), a), "banks vs reference")
        # a result longer than the room given: the full length, MODS_E_CAPACITY, as mods_match_fginn answers
        with pytest.raises(pkg.ModsError, match="overflow"):
            pkg.match_guided_reps(gpu_ctx, rq, rt, p, cap=5)
    finally:
        rq.close(); rt.close()


def _grey(fn):
    import orc
    from PIL import Image
    return orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB")))


def test_end_to_end_graf(pkg, gpu_ctx, capsys):
    """graf1 / graf6 through the pair entry point for H, the context's regions into banks, the guided search on them: equal to the
    reference on the fetched regions.  The counts are printed (profiles/guided_timing.txt records them), not compared."""
    import torch
    a, b = _grey(G1), _grey(G6)
    h, w = a.shape
    img = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    pkg.ransac_pin_seed(4242)
    try:
        res, _ = pkg.match_pair_dev(gpu_ctx, img.data_ptr(), w, h, pkg.PairParams.default())
    finally:
        pkg.ransac_pin_seed(-1)
    assert res.n_inliers >= 15
    H = np.array(list(res.H))
    r1, r2 = gpu_ctx.regions_fetch(0), gpu_ctx.regions_fetch(1)
    rq, rt = pkg.ImgRep(gpu_ctx, len(r1) + 1), pkg.ImgRep(gpu_ctx, len(r2) + 1)
    try:
        rq.append_ctx(0); rt.append_ctx(1)
        p, a = params(pkg, H, radius=4.0, ratio=0.9, contrad=10.0, one_to_one=1)
        got = pkg.match_guided_reps(gpu_ctx, rq, rt, p)
        assert_same(got, ref_of(r1, r2, H, a), "graf")
        dd = pkg.duplicate_filter_gpu(gpu_ctx, got[0], got[1], got[2], 2.0, 1)
        with capsys.disabled():
            print("\ngraf1/graf6 one view: regions %d | %d, RANSAC inliers %d, guided %d, guided de-duplicated %d"
                  % (len(r1), len(r2), res.n_inliers, len(got[0]), len(dd[0])))
    finally:
        rq.close(); rt.close()


def test_cli_guided_matches_pass_the_gate(pkg, tmp_path):
    """[Matching] guidedMatching = 1 on the classic configuration: every row of the matches file passes the symmetric transfer gate
    under the H file of the same run.  Both files carry six significant digits (coordinates below 1000: 5e-4 px per value, the
    entries of H 5e-6 relative), which moves a transfer by less than 0.01 px: the radius is tested with that slack."""
    ini = open(os.path.join(CFG, "classic.ini")).read()
    (tmp_path / "c.ini").write_text(ini.replace("[Matching]\n", "[Matching]\nguidedMatching = 1\n"))
    env = dict(os.environ, MODS_RANSAC_SEED="4242")
    args = [MODS, G1, G6, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", str(tmp_path / "c.ini"),
            os.path.join(CFG, "iters_one_view.ini")]
    p = subprocess.run(args, cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err
    assert "Guided matching (radius 4, ratio 0.9): " in err
    m = np.loadtxt(tmp_path / "m.txt").reshape(-1, 4)
    log = (tmp_path / "log.txt").read_text().split()
    assert len(log) == 7 and int(log[1]) >= 15                       # the log row is the verification's, as without the key
    n_unique = int(err.split(" correspondences, ")[1].split(" after duplicate filtering")[0])
    assert len(m) == n_unique > 0
    H = np.loadtxt(tmp_path / "H.txt")
    fwd = apply_h(H, m[:, :2]) - m[:, 2:]
    bwd = apply_h(np.linalg.inv(H), m[:, 2:]) - m[:, :2]
    r = 4.0 + 0.01
    assert ((fwd ** 2).sum(1) <= r * r).all() and ((bwd ** 2).sum(1) <= r * r).all()
    # the same run without the key writes the verified list
    p = subprocess.run(args[:12] + [os.path.join(CFG, "classic.ini")] + args[13:], cwd=tmp_path, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and "Guided matching" not in p.stderr.decode()
    assert len(np.loadtxt(tmp_path / "m.txt").reshape(-1, 4)) == int(log[1])
