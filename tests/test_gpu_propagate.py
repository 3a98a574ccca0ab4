"""-m gpu: match propagation (csrc/propagate.hip) against the numpy restatement of its contract (tests/propagate_ref.py) on the
cases of tests/propagate_cases.py, each of which tests/test_cpu_propagate.py has examined: forward and reversed restatement try
the same cells with the same winners, statuses and iteration counts, and nothing is decided within 1e-6 of a threshold.

Yardstick.  Cells, rounds, parents, statuses, iteration counts, the statistics, the list's length and the truncation flag are
integers: equal.  Keys and candidate rows of a proposal pass are fp64 expressions in a written order: equal to the bit.  Positions,
frames and zncc values pass through the window sums, whose order numpy does not restate: the restatement's forward and reversed
runs differ by at most propagate_cases.SPREAD = 2.14e-14 over the whole runs (measured on the CPU and held there), and the kernels
may differ from the forward run by ten times that."""
import ctypes as C

import numpy as np
import pytest

import lsm_cases as K
import lsm_ref as L
import propagate_cases as PC
import propagate_ref as P

pytestmark = pytest.mark.gpu
TOL = 10 * PC.SPREAD
EXACT = ("cell", "parent", "round", "iterations", "stats", "tried_status", "tried_iterations", "seed_status")
BYTES = EXACT + ("laf", "u6", "zncc")


@pytest.fixture(scope="module")
def ref():
    """the restatement's forward run of every case, computed once: name -> (img1, img2, seeds, parameter overrides, max_out, result)"""
    out = {}
    for name, img, seeds, kw, cap in PC.cases():
        a, b = PC.images_of(img)
        out[name] = (a, b, seeds, kw, cap, P.propagate(a, b, seeds, P.params(**kw), cap))
    return out


def check(got, want, tag):
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    assert got["truncated"] == want["truncated"] and len(got["laf"]) == len(want["laf"]), tag
    worst = 0.0
    if len(want["laf"]):
        worst = max(np.abs(got["laf"] - want["laf"]).max(), np.abs(got["u6"] - want["u6"]).max(), np.abs(got["zncc"] - want["zncc"]).max())
    print("%s: %d rows in %d rounds, largest difference %.3g (allowed %.3g)" % (tag, len(want["laf"]), want["round"].max() if len(want["laf"]) else 0,
                                                                               worst, TOL))
    assert worst <= TOL, (tag, worst)
    assert np.array_equal(got["u6"], L.u6_of(got["laf"]))


def bits(got):
    return tuple(np.ascontiguousarray(got[k]).tobytes() for k in BYTES) + (got["truncated"],)


def run(pkg, ctx, ref, name):
    a, b, seeds, kw, cap, want = ref[name]
    got = ctx.propagate_matches(a, b, seeds, pkg.propagate_defaults(**kw), cap)
    check(got, want, name)
    return got


@pytest.mark.parametrize("case", PC.propose_cases(), ids=lambda c: c[0])
def test_one_proposal_pass(pkg, gpu_ctx, case):
    """winners, keys, the list in raster order and the candidate rows: ties, collisions of 300 rows, clipping at the corners, and a
    grid of 48 x 40 cells, which the list's scan crosses in two workgroups"""
    name, w, h, cell, reach, rows, cells, state = case
    cl = cells if cells is not None else [P.own_cell(r, cell) for r in rows]
    key, win = P.propose(rows, cl, state, cell, reach)
    cand = P.candidates(key, rows, cell)
    for fc in ((cells,) if cells is not None else (None, cl)):            # the rows' own cells: computed by the library, or given
        gwin, gkey, gcell, glaf = pkg.test_propagate_round(gpu_ctx, w, h, cell, reach, rows, fc, state)
        assert np.array_equal(gkey, key) and np.array_equal(gwin, win), name
        assert gcell.tolist() == [c[0] for c in cand], name
        assert glaf.tobytes() == np.array([c[2] for c in cand]).tobytes(), name
    if not state.any():
        gwin, gkey, gcell, glaf = pkg.test_propagate_round(gpu_ctx, w, h, cell, reach, rows, cells, None)      # no state: all free
        assert np.array_equal(gkey, key)
    print("%s: %d of %d cells proposed by %d rows" % (name, len(cand), key.size, len(rows)))


@pytest.mark.parametrize("name", [c[0] for c in PC.cases()])
def test_whole_runs(pkg, gpu_ctx, ref, name):
    """strided images with NaN padding, the two images of different sizes; "big round": 1097 candidates in one round"""
    got = run(pkg, gpu_ctx, ref, name)
    if name == "big round":
        assert got["stats"][1].sum() > 1000


@pytest.mark.parametrize("name", ["up", "big round", "occluded", "cap"])
def test_two_calls_return_identical_bytes(pkg, gpu_ctx, ref, name):
    a, b, seeds, kw, cap, _ = ref[name]
    par = pkg.propagate_defaults(**kw)
    assert bits(gpu_ctx.propagate_matches(a, b, seeds, par, cap)) == bits(gpu_ctx.propagate_matches(a, b, seeds, par, cap))


@pytest.mark.parametrize("name", ["up", "down", "borders"])
def test_a_permutation_of_the_seeds_renames_the_parents(pkg, gpu_ctx, ref, name):
    a, b, seeds, kw, cap, _ = ref[name]
    par = pkg.propagate_defaults(**kw)
    one, two = gpu_ctx.propagate_matches(a, b, seeds, par, cap), gpu_ctx.propagate_matches(a, b, seeds[::-1], par, cap)
    n = len(seeds)
    assert np.array_equal(np.where(two["parent"] < n, n - 1 - two["parent"], two["parent"]), one["parent"])
    assert np.array_equal(two["seed_status"][::-1], one["seed_status"])
    for k in BYTES:
        if k not in ("parent", "seed_status"):
            assert np.ascontiguousarray(one[k]).tobytes() == np.ascontiguousarray(two[k]).tobytes(), k


def test_device_images_and_null_outputs(pkg, gpu_ctx, ref):
    """mods_propagate_matches_dev on strided device images gives the host entry point's bits; any output may be null; par == NULL:
    the defaults; n == 0"""
    import torch
    a, b, seeds, kw, cap, _ = ref["occluded"]
    par = pkg.propagate_defaults(**kw)
    want = gpu_ctx.propagate_matches(a, b, seeds, par, cap)
    ta = torch.full((K.H1, K.STRIDE1), float("nan")); ta[:, :K.W1] = torch.from_numpy(np.array(a))
    tb = torch.full((K.H2, K.STRIDE2), float("nan")); tb[:, :K.W2] = torch.from_numpy(np.array(b))
    ta, tb = ta.cuda(), tb.cuda()
    torch.cuda.synchronize()
    dev = (ta.data_ptr(), K.W1, K.H1, K.STRIDE1, tb.data_ptr(), K.W2, K.H2, K.STRIDE2)
    assert bits(gpu_ctx.propagate_matches_dev(*dev, seeds, par, cap)) == bits(want)
    n_out = C.c_int(-1)
    rc = pkg.lib().mods_propagate_matches_dev(gpu_ctx.h, C.c_void_p(dev[0]), *dev[1:4], C.c_void_p(dev[4]), *dev[5:], seeds.ctypes.data_as(C.c_void_p),
                                              len(seeds), None, 10000, *([None] * 7), C.byref(n_out), *([None] * 5))
    dflt = gpu_ctx.propagate_matches(a, b, seeds)
    assert rc == 0 and n_out.value == len(dflt["laf"]) > 0
    empty = gpu_ctx.propagate_matches(a, b, seeds[:0], par)
    assert len(empty["laf"]) == 0 and not empty["truncated"] and not empty["stats"].any()


def test_a_refused_call_launches_nothing_and_the_next_one_runs(pkg, gpu_ctx, ref):
    a, b, seeds, kw, cap, want = ref["one round"]
    for bad in (dict(cell=1), dict(reach=5), dict(rounds=0), dict(model_type=0, model=[float("inf")] * 9), dict(radius=16)):
        try:
            gpu_ctx.timing_enable(["propagate"]); gpu_ctx.timing_reset()
            with pytest.raises(pkg.ModsError, match="propagate_matches: "):
                gpu_ctx.propagate_matches(a, b, seeds, pkg.propagate_defaults(**dict(kw, **bad)))
            assert gpu_ctx.timing_read("propagate")[1] == 0
        finally:
            gpu_ctx.timing_enable([])
    check(gpu_ctx.propagate_matches(a, b, seeds, pkg.propagate_defaults(**kw), cap), want, "after the refusals")


def test_stage_timer(pkg, gpu_ctx, ref):
    a, b, seeds, kw, cap, want = ref["one round"]
    try:
        gpu_ctx.timing_enable(["propagate"]); gpu_ctx.timing_reset()
        gpu_ctx.propagate_matches(a, b, seeds, pkg.propagate_defaults(**kw), cap)
        ms, n, _ = gpu_ctx.timing_read("propagate")
        assert n == 3 and ms > 0               # the seeds; propose and list; register and gate
        gpu_ctx.propagate_matches(a, b, seeds[:0], pkg.propagate_defaults(**kw), cap)       # launches nothing
        assert gpu_ctx.timing_read("propagate")[1] == 3
    finally:
        gpu_ctx.timing_enable([])


def test_earlier_results_are_left_alone(pkg, gpu_ctx, ref):
    """behind a propagation the matcher's last search is fetched unchanged, and a k-NN search, a guided search and a refinement
    made before it, repeated on the buffers the context kept for them, return the bytes they returned before"""
    rng = np.random.default_rng(5)
    q = np.zeros(300, pkg.REGION_DTYPE)
    q["x"], q["y"] = rng.uniform(0, 600, 300), rng.uniform(0, 400, 300)
    q["s"], q["a11"], q["a22"] = rng.uniform(2, 6, 300), 1.0, 1.0
    q["desc"] = rng.integers(0, 256, (300, 128))
    t = q.copy()
    t["x"] += 3.0
    t["desc"] = np.clip(q["desc"].astype(np.int32) + rng.integers(-3, 4, (300, 128)), 0, 255)
    gpar = pkg.GuidedParams.default(model=[1, 0, 3, 0, 1, 0, 0, 0, 1], radius=4.0, ratio=0.9)
    a, b, seeds, kw, cap, _ = ref["up"]

    def earlier():
        d2, idx = gpu_ctx.match_knn(q, t, 5)
        gt, gu, gl = gpu_ctx.match_guided(q, t, gpar)
        rf = gpu_ctx.refine_matches(a, b, seeds)
        assert len(gt) > 100 and (idx[:, 0] == np.arange(300)).all()
        return (d2.tobytes(), idx.tobytes(), gt.tobytes(), gu.tobytes(), gl.tobytes()) + tuple(rf[k].tobytes() for k in sorted(rf))

    before = earlier()
    tent, u6 = gpu_ctx.match_fginn(q, t, 0.9)                 # last of all: the matcher's "last search"
    laf = gpu_ctx.last_laf.copy()
    run(pkg, gpu_ctx, ref, "up")
    run(pkg, gpu_ctx, ref, "big round")
    room = len(q)
    tent2 = np.zeros(room, pkg.TENT_DTYPE); u62 = np.zeros((room, 6)); laf2 = np.zeros((room, 14))
    n = C.c_int(-1)
    assert pkg.lib().mods_match_fetch_internal(gpu_ctx.h, tent2.ctypes.data_as(C.c_void_p), u62.ctypes.data_as(C.c_void_p),
                                               laf2.ctypes.data_as(C.c_void_p), room, C.byref(n)) == 0
    assert n.value == len(tent) > 100 and tent2[:n.value].tobytes() == tent.tobytes()
    assert np.array_equal(u62[:n.value], u6) and np.array_equal(laf2[:n.value], laf)
    assert earlier() == before


@pytest.mark.parametrize("name", ["down", "borders"])
def test_the_rows_of_a_round_are_the_refinement_of_its_candidates(pkg, gpu_ctx, ref, name):
    """the shared row body: every output row of the propagation, rebuilt on the host as a candidate from its parent's row and its
    cell and sent through mods_refine_matches, comes back with the propagation's bits"""
    a, b, seeds, kw, cap, _ = ref[name]
    par = pkg.propagate_defaults(**kw)
    got = gpu_ctx.propagate_matches(a, b, seeds, par, cap)
    seeds_out = gpu_ctx.refine_matches(a, b, seeds, par.lsm)
    assert np.array_equal(seeds_out["status"], got["seed_status"])
    combined = np.concatenate([seeds_out["laf"], got["laf"]])
    cand = np.array([P.candidate_row(combined[p], P.centre(c[0], par.cell), P.centre(c[1], par.cell)) for p, c in zip(got["parent"], got["cell"])])
    again = gpu_ctx.refine_matches(a, b, cand, par.lsm)
    assert (again["status"] == L.OK).all() and len(cand) == len(got["laf"]) > 90        # 201 ("down"), 95 ("borders")
    assert again["laf"].tobytes() == got["laf"].tobytes() and again["zncc_after"].tobytes() == got["zncc"].tobytes()
    assert np.array_equal(again["iterations"], got["iterations"])
