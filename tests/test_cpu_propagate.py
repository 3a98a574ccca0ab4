"""Match propagation (csrc/propagate.hip) without a device: the numpy restatement of its contract (tests/propagate_ref.py) held
against ground truth that does not come from it, the hand cases of the contract, the validity of every input the GPU test uses,
and the refusals.

Measured with the restatement on the analytic pairs of tests/lsm_cases.py (two seeds up to 1 px off, every frame entry changed by up
to +-5 %; cell 4, reach 1, six rounds, 11 x 11 window):
    pair "up":   16 / 27 / 32 / 34 / 31 / 30 rows accepted in rounds 1 .. 6, 170 in all; transfer error 0.0580 px max, 0.0182 median;
                 28 rejections, all OUTSIDE (windows over the border of image 2); smallest zncc 0.9998
    pair "down": 16 / 32 / 46 / 42 / 39 / 26, 201 in all; 0.0477 px max, 0.0119 median; 38 rejections, all OUTSIDE
The bound asserted is 0.1 px.  Forward and reversed window sums give the same rows, cells, parents, statuses and iteration counts in
every case of tests/propagate_cases.py and differ by at most propagate_cases.SPREAD = 2.14e-14 in a coordinate, a frame entry or a
zncc value (measured: 2.13e-14, the "down" pair)."""
import ctypes as C
import os

import numpy as np
import pytest

import lsm_cases as K
import lsm_ref as L
import propagate_cases as PC
import propagate_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read
E_ARG = -2
ERROR_BOUND = 0.1
NAMES = ("mods_propagate_defaults", "mods_propagate_matches_dev", "mods_propagate_matches", "mods_test_propagate_round")
EXACT = ("cell", "parent", "round", "iterations", "stats", "tried_status", "tried_iterations", "seed_status")


@pytest.fixture(scope="module", autouse=True)
def library_defaults(pkg):
    """the restatement restates this library's contract: every test of this file starts from the library's own defaults being the
    restatement's (mods_propagate_defaults)"""
    p, want = pkg.propagate_defaults(), P.params()
    assert (p.cell, p.reach, p.rounds, p.model_type, p.model_thr, p.lsm.radius) == \
        (want["cell"], want["reach"], want["rounds"], want["model_type"], want["model_thr"], want["lsm"]["radius"])
    return p


@pytest.fixture(scope="module")
def runs():
    """every case through the restatement, forward and reversed, once: name -> (images, seeds, parameters, max_out, forward, reversed)"""
    out = {}
    for name, img, seeds, kw, cap in PC.cases():
        a, b = PC.images_of(img)
        par = P.params(**kw)
        out[name] = (a, b, seeds, par, cap, P.propagate(a, b, seeds, par, cap), P.propagate(a, b, seeds, par, cap, order="reverse"))
    return out


def same(f, g, keys=EXACT + ("laf", "zncc", "u6")):
    return all(np.array_equal(f[k], g[k]) for k in keys) and f["truncated"] == g["truncated"]


# ---- ground truth

@pytest.mark.parametrize("kind", ["up", "down"])
def test_propagation_grows_on_the_analytic_pairs(runs, kind):
    f = runs[kind][5]
    per_round = np.bincount(f["round"], minlength=7)[1:]
    err = K.transfer_error(f["laf"], kind)
    print("%s: accepted per round %s, transfer error %.4f max %.4f median, rejections %s, smallest zncc %.4f"
          % (kind, per_round.tolist(), err.max(), np.median(err), f["stats"][1:, 1:].sum(0).tolist(), f["zncc"].min()))
    assert (f["seed_status"] == L.OK).all()
    assert (per_round > 0).all() and len(f["laf"]) > 150                  # it grows in every round
    rejected = f["stats"][1:].sum(0)
    assert rejected[L.OUTSIDE] > 0 and rejected[[1, 2, 4, 5, 6, 7]].sum() == 0           # every rejection is OUTSIDE
    assert err.max() < ERROR_BOUND                                        # measured: 0.0580 ("up"), 0.0477 ("down")
    assert f["zncc"].min() - 0.8 > 0.19
    # every accepted row sits in its own cell's centre on side 1 (image 1 holds the template of "up") or was moved by LSM ("down")
    p = np.array([[P.centre(c[0], 4), P.centre(c[1], 4)] for c in f["cell"]])
    if kind == "up":
        assert np.array_equal(f["laf"][:, :2], p)
    else:
        assert np.abs(f["laf"][:, :2] - p).max() <= 3.0 and (f["laf"][:, :2] != p).any()


# ---- validity of the inputs of the GPU test

@pytest.mark.parametrize("name", [c[0] for c in PC.cases()])
def test_case_is_a_valid_gpu_input(runs, name):
    a, b, seeds, par, cap, f, r = runs[name]
    assert same(f, r, EXACT), name                                        # the same cells, winners, statuses and iteration counts
    spread = max(np.abs(f["laf"] - r["laf"]).max(), np.abs(f["zncc"] - r["zncc"]).max()) if len(f["laf"]) else 0.0
    print("%s: %d rows, forward / reversed spread %.3g" % (name, len(f["laf"]), spread))
    assert spread <= PC.SPREAD
    assert P.margins(a, b, f, par) == []                                  # nothing decided within 1e-6 of a threshold
    assert f["stats"].sum() == len(seeds) + len(f["tried"])
    assert (f["tried_status"] >= 0).sum() == len(f["tried"])              # a cell is tried once


def test_proposal_pass_on_the_inputs_of_the_gpu_test():
    """the fronts of the GPU proposal test: the key is a function of integers and of one fp64 expression rounded to float32, so it
    has no yardstick but equality; here: what the pass must and must not touch"""
    for name, w, h, cell, reach, rows, cells, state in PC.propose_cases():
        cl = cells if cells is not None else [P.own_cell(r, cell) for r in rows]
        key, win = P.propose(rows, cl, state, cell, reach)
        assert key.shape == (h // cell, w // cell) == state.shape and (win >= 0).any(), name
        assert (win[state != P.FREE] == -1).all(), name                       # occupied and closed cells are never proposed
        gy, gx = np.nonzero(win >= 0)
        for y, x, k in zip(gy, gx, win[gy, gx]):                              # the winner is within reach of the cell
            assert max(abs(cl[k][0] - x), abs(cl[k][1] - y)) <= reach, name
        cand = P.candidates(key, rows, cell)
        assert [c[0] for c in cand] == sorted(c[0] for c in cand) and len(cand) == (win >= 0).sum()
    name, w, h, cell, reach, rows, cells, state = PC.propose_cases()[3]
    key, win = P.propose(rows, cells, state, cell, reach)
    assert win[0, 0] == 0 and win[0, 23] == 1 and win[19, 0] == 2 and win[19, 23] == 3       # all four corners, clipped
    assert win[10, 23] == 4 and win[19, 12] == 5 and win[5, 0] == 6                          # rows whose own cell lies outside the grid
    assert win[12, 12] == 7 and 8 not in win                                                  # identical rows: the lower index


# ---- hand cases

def test_two_seeds_equidistant_from_a_cell_the_lower_index_wins(runs):
    a, b, seeds, par, cap, f, r = runs["tie"]
    assert P.own_cell(seeds[0], 4) == (10, 9) and P.own_cell(seeds[1], 4) == (12, 9) and P.own_cell(seeds[2], 4) == (10, 9)
    first = {tuple(c): p for c, p, rd in zip(f["cell"].tolist(), f["parent"].tolist(), f["round"].tolist()) if rd == 1}
    for gy in (8, 9, 10):                       # the column between them: d2 = 16, 32 from both
        assert first[(11, gy)] == 0
    state = np.zeros((20, 24), np.uint8)
    key, win = P.propose(seeds[:2], [(10, 9), (12, 9)], state, 4, 1)
    assert key[9, 11] == (int(np.float32(16.0).view(np.uint32)) << 32) and win[9, 11] == 0
    key, win = P.propose(seeds[:2][::-1], [(12, 9), (10, 9)], state, 4, 1)
    assert win[9, 11] == 0                      # ... whichever row that is
    # seeds in one cell: both propose its neighbours, the nearer one wins each
    assert first[(9, 9)] == 2 and first[(10, 8)] in (0, 2) and (10, 9) not in first
    assert set(first.values()) == {0, 1, 2}


def test_seed_in_the_partial_last_column_or_row(runs):
    a, b, seeds, par, cap, f, r = runs["partial"]
    Gx, Gy = P.lattice(a.shape[1], a.shape[0], 11)
    assert (Gx, Gy) == (4, 6) and P.own_cell(seeds[0], 11)[0] == Gx and P.own_cell(seeds[1], 11)[1] == Gy     # outside the grid
    assert (f["seed_status"] == L.OK).all()
    first = f["round"] == 1
    assert set(f["parent"][first].tolist()) == {0, 1} and (f["cell"][first][f["parent"][first] == 0, 0] == Gx - 1).all()
    assert (f["cell"][first][f["parent"][first] == 1, 1] == Gy - 1).all()


def test_proposals_are_clipped_at_all_four_borders(runs):
    a, b, seeds, par, cap, f, r = runs["borders"]
    h, w = a.shape
    assert w % 5 and h % 5                                               # w1 is no multiple of the cell
    t = f["tried_status"]
    assert t.shape == (h // 5, w // 5)
    assert (t[0] >= 0).any() and (t[-1] >= 0).any() and (t[:, 0] >= 0).any() and (t[:, -1] >= 0).any()
    assert (f["stats"][-1] == 0).all() and f["stats"][1:].sum() == (t >= 0).sum()     # it ran out of cells before it ran out of rounds
    # reach 2: the first round tries the 5 x 5 blocks around the two seeds' one cell
    assert f["stats"][1].sum() == 24
    assert PC.window_error(f["laf"]).max() < ERROR_BOUND


def test_one_round_and_the_cap(runs):
    whole, one, cut, none = runs["up"][5], runs["one round"][5], runs["cap"][5], runs["cap 0"][5]
    n1 = (whole["round"] == 1).sum()
    assert len(one["laf"]) == n1 and np.array_equal(one["laf"], whole["laf"][:n1]) and one["stats"].shape == (2, 8)
    assert cut["truncated"] and len(cut["laf"]) == 30 and not whole["truncated"]
    assert n1 < 30 < (whole["round"] <= 2).sum()                           # the cap cuts round 2 ...
    for k in ("laf", "zncc", "cell", "parent", "round"):
        assert np.array_equal(cut[k], whole[k][:30]), k                    # ... to its prefix in raster order
    assert np.array_equal(cut["stats"][:3], whole["stats"][:3]) and not cut["stats"][3:].any()
    assert none["truncated"] and len(none["laf"]) == 0 and none["stats"][1].sum() == 16 and not none["stats"][2].any()


def test_rejected_seeds_do_not_propagate(runs):
    f = runs["bad seeds"][5]
    assert f["seed_status"].tolist() == [L.OK, L.OK, L.BAD_FRAME]
    a, b, seeds, par, cap = runs["bad seeds"][:5]
    two = P.propagate(a, b, seeds[:2], par, cap)
    ren = lambda p, n: np.where(p >= n, p - n, -1 - p)                     # a seed, or an output row, whatever n is
    assert np.array_equal(f["laf"], two["laf"]) and np.array_equal(ren(f["parent"], 3), ren(two["parent"], 2))
    g = runs["maxiter seed"][5]
    assert g["seed_status"].tolist() == [L.OK, L.MAXITER]
    assert len(g["laf"]) > 8 and (g["parent"][g["round"] == 1] == 0).all() and g["stats"][1].sum() == 8


def test_an_unrelated_rectangle_of_image_2_is_not_entered(runs):
    a, b, seeds, par, cap, f, r = runs["occluded"]
    x0, y0 = PC.OCC[:2]
    R = par["lsm"]["radius"]
    inside = np.minimum(f["laf"][:, 7] - x0, f["laf"][:, 8] - y0)          # how far inside the rectangle (it reaches the image's corner)
    print("occluded: %d rows, deepest %.2f px inside, statuses %s" % (len(f["laf"]), inside.max(), f["stats"][1:].sum(0).tolist()))
    assert len(f["laf"]) > 100 and inside.max() <= R
    assert f["stats"][1:, [L.DIVERGED, L.LOW_ZNCC, L.MAXITER]].sum() > 0   # the rectangle's edge is where the pixels say no


def test_model_gates(runs):
    free = runs["up"][5]
    assert same(runs["H gate"][5], free) and same(runs["F gate"][5], free) and same(runs["F gate down"][5], runs["down"][5])
    off = runs["H gate off"][5]
    assert len(off["laf"]) == 0 and off["stats"][1, P.OFF_MODEL] == 16 and off["stats"][1].sum() == 16 and not off["stats"][2:].any()
    assert (off["tried_status"] == P.OFF_MODEL).sum() == 16
    d2 = [t["d2"] for t in off["tried"]]
    assert min(d2) > 16.0                                                  # 5 px off against a threshold of 2
    H = PC.affine_h("up")
    x1 = np.array([30.0, 50.0]); x2 = K.A_OF["up"] @ x1 + K.T_OF["up"]
    assert P.model_d2(0, H, x1[0], x1[1], x2[0] + 3.0, x2[1] - 4.0) == pytest.approx(25.0, abs=1e-9)
    F = PC.epipolar_f(H)
    assert P.model_d2(1, F, x1[0], x1[1], x2[0], x2[1]) < 1e-20
    Fm = F.reshape(3, 3).T                                                 # F_ij
    l = Fm @ np.r_[x1, 1.0]
    off_line = x2 + 3.0 * l[:2] / np.hypot(l[0], l[1])                     # 3 px off its epipolar line
    m = Fm.T @ np.r_[off_line, 1.0]
    e = np.r_[off_line, 1.0] @ l
    assert P.model_d2(1, F, x1[0], x1[1], off_line[0], off_line[1]) == pytest.approx(e * e / (l[0] ** 2 + l[1] ** 2 + m[0] ** 2 + m[1] ** 2), rel=1e-12)
    assert P.model_d2(0, [1, 0, 0, 0, 1, 0, 0, 0, 0], 1.0, 1.0, 1.0, 1.0) is None and P.model_d2(1, np.zeros(9), 1.0, 1.0, 1.0, 1.0) is None


def test_candidate_row_carries_the_winners_affine_map():
    f = K.displaced(K.true_rows(1, 3, "up", scale=2.0), 4)[0]
    row = P.candidate_row(f, 41.5, 37.5)
    B = L.affine_of(f)
    assert np.array_equal(row[:7], [41.5, 37.5, 1, 0, 0, 1, 1])
    assert np.allclose(L.affine_of(row), B, rtol=0, atol=1e-14)
    assert np.allclose(row[7:9], f[7:9] + B @ (np.array([41.5, 37.5]) - f[:2]), rtol=0, atol=1e-12)


# ---- symbols, defaults and the refusals that need no device

def test_symbols_defaults_and_stage(pkg):
    header = open(os.path.join(ROOT, "include", "mods_hip.h")).read()
    for name in NAMES:
        assert hasattr(pkg.lib(), name) and name + "(" in header, name
    assert header.index("MODS_STAGE_REFINE,") < header.index("MODS_STAGE_PROPAGATE,") < header.index("MODS_STAGE_COUNT")
    assert pkg.stage_index("propagate") == pkg.stage_index("refine") + 1
    p = pkg.propagate_defaults()
    want = P.params()
    assert dict(cell=p.cell, reach=p.reach, rounds=p.rounds, model_type=p.model_type, model_thr=p.model_thr) == \
        {k: want[k] for k in ("cell", "reach", "rounds", "model_type", "model_thr")}
    q = p.lsm
    got = dict(radius=q.radius, max_iter=q.max_iter, eps_shift=q.eps_shift, max_shift=q.max_shift, max_scale_change=q.max_scale_change,
               max_magnification=q.max_magnification, min_zncc=q.min_zncc, lam=q.lam, affine=q.affine)
    assert got == want["lsm"] and got == dict(L.DEFAULTS, radius=5)
    assert pkg.PROP_STATUS == P.STATUS_NAMES and len(pkg.PROP_STATUS) == P.STATUS_COUNT
    assert C.sizeof(pkg.PropagateParams) == 16 + 64 + 72 + 8
    assert "MODS_PROP_OFF_MODEL = MODS_LSM_STATUS_COUNT, MODS_PROP_STATUS_COUNT" in header
    with pytest.raises(TypeError):
        pkg.propagate_defaults(no_such_field=1)


REFUSED = [
    (dict(cell=1), {}, "cell"), (dict(cell=65), {}, "cell"), (dict(reach=0), {}, "reach"), (dict(reach=5), {}, "reach"),
    (dict(rounds=0), {}, "rounds"), (dict(rounds=65), {}, "rounds"), (dict(model_type=2), {}, "model_type"), (dict(model_type=-2), {}, "model_type"),
    (dict(model_type=0, model=[1, 0, 0, 0, 1, 0, 0, float("nan"), 1]), {}, "model entry 7"), (dict(model_type=1, model_thr=0.0), {}, "model_thr"),
    (dict(model_type=0, model_thr=float("inf")), {}, "model_thr"), (dict(radius=0), {}, "radius"), (dict(radius=16), {}, "radius"),
    (dict(max_iter=0), {}, "max_iter"), (dict(eps_shift=0.0), {}, "eps_shift"), (dict(max_shift=float("inf")), {}, "max_shift"),
    (dict(lam=0.0), {}, "lambda"), (dict(max_scale_change=0.5), {}, "max_scale_change"), (dict(max_magnification=float("nan")), {}, "max_magnification"),
    (dict(min_zncc=1.5), {}, "min_zncc"), (dict(affine=2), {}, "affine"),
    ({}, dict(n=-1), "n = -1"), ({}, dict(max_out=-1), "max_out"), ({}, dict(stride1=95), "stride"), ({}, dict(stride2=63), "stride"),
    ({}, dict(w2=1), "image size"), (dict(cell=64), dict(h1=63), "holds no cell"),
    ({}, dict(img1=None), "null"), ({}, dict(img2=None), "null"), ({}, dict(laf=None), "null"), ({}, dict(ctx=None), "null"),
]


def _call(pkg, entry, a, par):
    return getattr(pkg.lib(), entry)(a["ctx"], a["img1"], a["w1"], a["h1"], a["stride1"], a["img2"], a["w2"], a["h2"], a["stride2"], a["laf"],
                                     a["n"], par, a["max_out"], *([None] * 13))


@pytest.mark.parametrize("entry", ["mods_propagate_matches", "mods_propagate_matches_dev"])
@pytest.mark.parametrize("par_kw,arg_kw,part", REFUSED, ids=[r[2] + str(i) for i, r in enumerate(REFUSED)])
def test_refusals_before_any_device_call(pkg, entry, par_kw, arg_kw, part):
    """no context exists in this process and no pointer is valid: a call that got past its checks would crash"""
    a = dict(ctx=BUF, img1=BUF, w1=96, h1=80, stride1=96, img2=BUF, w2=64, h2=112, stride2=64, laf=BUF, n=3, max_out=10)
    a.update(arg_kw)
    rc = _call(pkg, entry, a, C.byref(pkg.propagate_defaults(**par_kw)))
    err = pkg.lib().mods_last_error().decode()
    assert rc == E_ARG and err.startswith("propagate_matches: ") and part in err, (rc, err)


def test_an_empty_list_launches_nothing(pkg):
    """n == 0 with arguments that would crash if they were used: MODS_OK, an empty list"""
    a = dict(ctx=BUF, img1=BUF, w1=96, h1=80, stride1=96, img2=BUF, w2=64, h2=112, stride2=64, laf=None, n=0, max_out=10)
    for entry in ("mods_propagate_matches", "mods_propagate_matches_dev"):
        n, t = C.c_int(-1), C.c_int(-1)
        rc = getattr(pkg.lib(), entry)(a["ctx"], a["img1"], 96, 80, 96, a["img2"], 64, 112, 64, None, 0, None, 10, None, None, None, None, None, None,
                                       None, C.byref(n), C.byref(t), None, None, None, None)
        assert rc == 0 and n.value == 0 and t.value == 0
    for args, part in (((None, 96, 80, 4, 1, BUF, None, 1), "null"), ((BUF, 96, 80, 1, 1, BUF, None, 1), "cell"), ((BUF, 96, 80, 4, 0, BUF, None, 1), "reach"),
                       ((BUF, 96, 80, 4, 1, BUF, None, 0), "front"), ((BUF, 96, 80, 4, 1, None, None, 1), "null")):
        rc = pkg.lib().mods_test_propagate_round(*args, None, None, None, None, None, None)
        err = pkg.lib().mods_last_error().decode()
        assert rc == E_ARG and err.startswith("propagate_matches: ") and part in err, (rc, err)
