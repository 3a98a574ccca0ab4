"""The distractor database of the FGINN ratio test (csrc/distractor.hip) without a device: its symbols and refusals, the numpy
statement of its contract (tests/distractor_ref.py) against a transcription of the reference's loop, the grid of its sweep, the
resources of its kernels read from the built library, and the command line's refusals."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import distractor_ref as dr
import match_cases as mc
import match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read
E_ARG, E_CAPACITY = -2, -3
QPB, MIN_TPS, ROW, MAX_SPLITS = 512, 16, 256, 4096      # csrc/distractor.hip: DB_QPB, DB_MIN_TPS, DB_ROW, DB_MAX_SPLITS
NAMES = ("mods_descdb_create", "mods_descdb_create_from_reps", "mods_descdb_count", "mods_descdb_destroy", "mods_descdb_min_dist",
         "mods_filter_distractor", "mods_ctx_distractor_db", "mods_distractor_counts", "mods_distractor_fetch",
         "mods_pipeline_distractor_db", "mods_descdb_grid", "mods_ctx_descdb_splits")


def test_symbols_are_exported(pkg):
    for name in NAMES:
        assert hasattr(pkg.lib(), name), name
    assert pkg.stage_index("distractor") + 1 == pkg.stage_index("distractor_sweep") == pkg.stage_index("knn_sweep") + 2
    header = open(os.path.join(ROOT, "include", "mods_hip.h")).read()
    assert header.index("MODS_STAGE_KNN_SWEEP,") < header.index("MODS_STAGE_DISTRACTOR,") < header.index("MODS_STAGE_DISTRACTOR_SWEEP,") \
        < header.index("MODS_STAGE_COUNT")
    for name in NAMES:
        assert name + "(" in header, name
    for cls in ("DescDB", "descdb_grid", "filter_distractor"):
        assert hasattr(pkg, cls)


def _refused(pkg, rc, prefix, part, code=E_ARG):
    err = pkg.lib().mods_last_error()
    assert rc == code and err.startswith(prefix) and part in err, (rc, err)


class _Db(C.Structure):
    """the head of mods_descdb (csrc/distractor.hip): device, rows - a database without a device, of which the refusals read these"""
    _fields_ = [("device", C.c_int), ("n", C.c_long), ("n_tiles", C.c_int), ("rest", C.c_char * 256)]


def test_refusals(pkg):
    L = pkg.lib()
    out = C.c_void_p()
    i1, i2 = C.c_int(), C.c_int()
    _refused(pkg, L.mods_descdb_create(0, BUF, C.c_long(4), None), b"descdb_create: ", b"null")
    _refused(pkg, L.mods_descdb_create(0, None, C.c_long(4), C.byref(out)), b"descdb_create: ", b"null")
    _refused(pkg, L.mods_descdb_create(0, BUF, C.c_long(-1), C.byref(out)), b"descdb_create: ", b"negative")
    _refused(pkg, L.mods_descdb_create(-1, BUF, C.c_long(4), C.byref(out)), b"descdb_create: ", b"negative")
    _refused(pkg, L.mods_descdb_create(0, BUF, C.c_long((1 << 24) + 1), C.byref(out)), b"descdb_create: ", b"capacity", E_CAPACITY)
    _refused(pkg, L.mods_descdb_create_from_reps(None, BUF, 1, C.byref(out)), b"descdb_create_from_reps: ", b"null")
    _refused(pkg, L.mods_descdb_create_from_reps(BUF, None, 1, C.byref(out)), b"descdb_create_from_reps: ", b"null")
    _refused(pkg, L.mods_descdb_create_from_reps(BUF, BUF, -1, C.byref(out)), b"descdb_create_from_reps: ", b"negative")
    _refused(pkg, L.mods_descdb_create_from_reps(BUF, BUF, 1, None), b"descdb_create_from_reps: ", b"null")
    L.mods_descdb_count.restype = C.c_long
    assert L.mods_descdb_count(None) == 0
    L.mods_descdb_destroy(None)
    _refused(pkg, L.mods_descdb_min_dist(None, BUF, BUF, 1, BUF), b"descdb_min_dist: ", b"null")
    _refused(pkg, L.mods_descdb_min_dist(BUF, None, BUF, 1, BUF), b"descdb_min_dist: ", b"null")
    _refused(pkg, L.mods_filter_distractor(None, BUF, BUF, 1, C.c_double(0.8), BUF, BUF, BUF, 1, BUF, C.byref(i1)), b"filter_distractor: ", b"null")
    _refused(pkg, L.mods_filter_distractor(BUF, None, BUF, 1, C.c_double(0.8), BUF, BUF, BUF, 1, BUF, C.byref(i1)), b"filter_distractor: ", b"null")
    _refused(pkg, L.mods_ctx_distractor_db(None, None, None), b"distractor_db: ", b"null")
    _refused(pkg, L.mods_distractor_counts(None, C.byref(i1), C.byref(i2)), b"distractor_counts: ", b"null")
    _refused(pkg, L.mods_distractor_counts(BUF, None, C.byref(i2)), b"distractor_counts: ", b"null")
    _refused(pkg, L.mods_distractor_fetch(None, BUF, 1, C.byref(i1)), b"distractor_fetch: ", b"null")
    _refused(pkg, L.mods_distractor_fetch(BUF, BUF, -1, C.byref(i1)), b"distractor_fetch: ", b"negative")
    _refused(pkg, L.mods_distractor_fetch(BUF, None, 1, C.byref(i1)), b"distractor_fetch: ", b"null")
    _refused(pkg, L.mods_pipeline_distractor_db(None, None), b"pipeline: ", b"null")
    _refused(pkg, L.mods_ctx_descdb_splits(None, 0), b"descdb_splits: ", b"null")
    _refused(pkg, L.mods_ctx_descdb_splits(BUF, -1), b"descdb_splits: ", b"negative")
    g = (C.c_int * 3)()
    for args in ((10, 10, 0, None), (-1, 10, 0, g), (10, -1, 0, g), (10, 10, -1, g), ((1 << 24) + 1, 10, 0, g)):
        _refused(pkg, L.mods_descdb_grid(C.c_long(args[0]), *args[1:]), b"descdb_grid: ", b"")
    # zeroed memory in the place of a context (device 0, nothing allocated) and dummy databases: the arguments that are read
    ctx0 = C.create_string_buffer(4 << 20)
    db0, db1 = _Db(0, 40, 2, b""), _Db(1, 40, 2, b"")
    for fn, tail in ((L.mods_descdb_min_dist, (BUF, 1, BUF)),
                     (L.mods_filter_distractor, (BUF, 1, C.c_double(0.8), BUF, BUF, BUF, 1, BUF, C.byref(i1)))):
        rc = fn(ctx0, C.byref(db1), *tail)
        assert rc == E_ARG and b"lives on device 1, the context on device 0" in L.mods_last_error(), L.mods_last_error()
    assert L.mods_ctx_distractor_db(ctx0, C.byref(db1), None) == E_ARG and b"the full database lives on device 1" in L.mods_last_error()
    assert L.mods_ctx_distractor_db(ctx0, None, C.byref(db1)) == E_ARG and b"the half database lives on device 1" in L.mods_last_error()
    _refused(pkg, L.mods_descdb_min_dist(ctx0, C.byref(db0), BUF, -1, BUF), b"descdb_min_dist: ", b"negative")
    _refused(pkg, L.mods_descdb_min_dist(ctx0, C.byref(db0), None, 1, BUF), b"descdb_min_dist: ", b"null")
    _refused(pkg, L.mods_filter_distractor(ctx0, C.byref(db0), BUF, 1, C.c_double(0.8), BUF, BUF, BUF, -1, BUF, C.byref(i1)),
             b"filter_distractor: ", b"negative")
    _refused(pkg, L.mods_filter_distractor(ctx0, C.byref(db0), BUF, 1, C.c_double(0.8), None, BUF, BUF, 1, BUF, C.byref(i1)),
             b"filter_distractor: ", b"null")
    tent = np.zeros(2, ref.TENT_DTYPE)
    _refused(pkg, L.mods_filter_distractor(ctx0, C.byref(db0), BUF, 1, C.c_double(1.0), C.c_void_p(tent.ctypes.data), BUF, BUF, 2, BUF, C.byref(i1)),
             b"filter_distractor: ", b"ratio")
    tent["q"][1] = 7
    _refused(pkg, L.mods_filter_distractor(ctx0, C.byref(db0), BUF, 7, C.c_double(0.8), C.c_void_p(tent.ctypes.data), BUF, BUF, 2, BUF, C.byref(i1)),
             b"filter_distractor: ", b"tentative 1 names query 7 of 7")
    # with no work to do nothing is touched: an empty list, an empty database
    assert L.mods_descdb_min_dist(ctx0, C.byref(db0), None, 0, None) == 0
    empty = _Db(0, 0, 0, b"")
    d = (C.c_int * 3)()
    assert L.mods_descdb_min_dist(ctx0, C.byref(empty), BUF, 0, d) == 0
    q = np.zeros((3, 128), np.uint8)
    assert L.mods_descdb_min_dist(ctx0, C.byref(empty), C.c_void_p(q.ctypes.data), 3, d) == 0 and list(d) == [dr.INT_MAX] * 3


def _reference_loop(q, t, db, ratio, contrad, nn):
    """MatchFlannFGINNPlusDB's loop over the queries (matching/matching.cpp:538-569) with exact neighbours: the rows (q, t, j-th
    neighbour, d0, dj, dDB, ratio) it pushes, float distances as FLANN hands them over"""
    sq = np.float64(ratio) * np.float64(ratio)
    c2 = np.float64(contrad) * np.float64(contrad)
    K = min(nn, len(t))
    dist, index = ref.neighbours(q, t, K)
    dists_db = dr.min_dist(q["desc"], db).astype(np.float32)
    rows = []
    for i in range(len(q)):
        row, ind = dist[i].astype(np.float32), index[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio_db = np.float64(row[0] / dists_db[i])
        for j in range(1, K):
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.float64(row[0] / row[j])
            r = ratio_db if r < ratio_db else r                 # std::max(ratio, ratioDB)
            if r <= sq:
                rows.append((i, int(ind[0]), int(ind[j]), float(row[0]), float(row[j]), float(dists_db[i]), float(np.sqrt(r))))
                break
            dx, dy = t["x"][ind[0]] - t["x"][ind[j]], t["y"][ind[0]] - t["y"][ind[j]]
            if dx * dx + dy * dy > c2:
                break
    return rows


def _bank(seed, nq=60, nt=70, ndb=90):
    """small random banks: two thirds of the queries copy a train with noise, and every second of those has a database row that
    is a noisier copy, an exact copy, or a copy at the same distance as the train; a duplicate train makes a d0 = 0 pair"""
    rng = np.random.default_rng(seed)
    q, t = mc.random_regions(nq, rng, 300.0), mc.random_regions(nt, rng, 300.0)
    db = rng.integers(0, 256, (ndb, 128), dtype=np.uint8)
    for i in range(0, 2 * nq // 3):
        t["desc"][i] = np.clip(q["desc"][i].astype(np.int16) + rng.integers(-3, 4, 128), 0, 255).astype(np.uint8)
        if i % 2 == 0:
            kind = (i // 2) % 4
            noise = (4, 7, 0, 12)[kind]
            db[i] = np.clip(q["desc"][i].astype(np.int16) + rng.integers(-noise, noise + 1, 128), 0, 255).astype(np.uint8)
            if kind == 3:
                db[i] = t["desc"][i]                                  # dDB = d0
    t["desc"][1] = q["desc"][1]; db[1] = q["desc"][1]                 # d0 = 0 and dDB = 0: 0 / 0, kept with its ratio
    t["desc"][3] = q["desc"][3]                                       # d0 = 0, dDB > 0
    return q, t, db


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("ratio,contrad,nn", [(0.8, 10.0, 50), (0.95, 1e9, 50), (0.6, 10.0, 5)])
def test_restatement_against_the_reference_loop(seed, ratio, contrad, nn):
    q, t, db = _bank(seed)
    kept, fwd, keep, ddb = dr.match_fginn_db(q, t, db, ratio, contrad, nn)
    rows = _reference_loop(q, t, db, ratio, contrad, nn)
    assert len(fwd) >= 30 and 0 < len(kept) < len(fwd), (len(fwd), len(kept))
    assert len(rows) == len(kept)
    for k, row in zip(kept, rows):
        assert (int(k["q"]), int(k["t"]), int(k["t_bad"]), float(k["d1"]), float(k["d2"])) == row[:5]
        assert float(k["ratio"]) == row[6]
    assert np.array_equal(ddb[keep].astype(np.float32), np.array([r[5] for r in rows], np.float32))
    # the survivors keep every other field, and a ratio that grew only where the database is the nearer rival
    src = fwd[keep]
    for f in ("q", "t", "t_bad", "t_2nd", "d1", "d2", "d2nd"):
        assert np.array_equal(kept[f], src[f]), f
    assert (kept["ratio"] >= src["ratio"]).all() and (kept["ratio"] > src["ratio"]).any() and (kept["ratio"] == src["ratio"]).any()
    if ratio == 0.8:
        assert 1 in kept["q"] and kept["ratio"][list(kept["q"]).index(1)] == 0.0        # 0 / 0 vetoes nothing
    # an empty database changes nothing
    same, _, keep0, ddb0 = dr.match_fginn_db(q, t, db[:0], ratio, contrad, nn)
    assert same.tobytes() == fwd.tobytes() and keep0.all() and (ddb0 == dr.INT_MAX).all()


def test_the_fp32_boundary_of_the_restatement():
    assert ref.dstar(5000, 0.8) == 7813
    base = np.full(128, 20, np.uint8)
    for d in (1, 2, 7, 5000, 7812, 7813, 39999, 40000):
        assert int(ref.sqdist(base[None], dr.at_distance(base, d)[None])[0, 0]) == d
    sq = np.float64(0.8) * np.float64(0.8)
    assert ref.ratio_quotient(5000, 7813) <= sq < ref.ratio_quotient(5000, 7812)


def test_grid(pkg):
    """the sweep's grid: the tiles are covered, a forced split count is honoured while the database has that many tiles, the query
    blocks cover the queries, a handful of query blocks is spread over the chip, and a split never falls below its minimum"""
    for m in (0, 1, 31, 32, 33, 8191, 8192, 8193, 1 << 17, 1 << 20, 1 << 22, 1 << 24):
        n_tiles = (m + 31) // 32
        for forced in (0, 1, 2, 3, 7, 64, 1000, 5000):
            prev = None
            for n_q in (0, 1, 511, 512, 513, 3000, 20000, 60156):
                qb, splits, tps = pkg.descdb_grid(m, n_q, forced)
                assert splits >= 1 and tps * splits >= n_tiles, (m, n_q, forced)
                assert qb * QPB >= n_q > (qb - 1) * QPB or (n_q == 0 and qb == 0)
                if forced > 0:
                    assert splits == max(1, min(forced, n_tiles, MAX_SPLITS))
                else:
                    assert splits == max(1, min(max(ROW, qb) // max(qb, 1), n_tiles // MIN_TPS, MAX_SPLITS))
                    assert splits == 1 or tps >= MIN_TPS
                if prev is not None:
                    assert qb >= prev[0] and splits <= prev[1] and tps >= prev[2]
                prev = (qb, splits, tps)
    # the sizes the timing tool reports (profiles/distractor_timing.txt)
    assert pkg.descdb_grid(1 << 20, 3000) == (6, 42, 781)
    assert pkg.descdb_grid(1 << 22, 20000) == (40, 6, 21846)
    assert pkg.descdb_grid(1 << 17, 3000) == (6, 42, 98)


def _kernel_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr


def test_descdb_sweep_owns_its_simds(pkg):
    """the co-residency rule (DESIGN.md "The matcher and its neighbours") for the new matrix-core kernel, read from the built library:
    a workgroup of 256 threads whose waves fill the 512-entry register file of each SIMD, no scratch in any kernel of the file; and
    the matcher's and the k-NN search's kernels are no further instantiations"""
    kr = _kernel_resources()
    if not os.path.exists(os.path.join(kr.LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump")
    ks = kr.kernels(os.path.join(ROOT, "mods-light-zmq_amd", "libmodsgpu.so"))
    mine = [k for k in ks if "descdb_" in k["name"]]
    names = sorted(n for k in mine for n in ("descdb_pack_kernel", "descdb_sweep_kernel", "descdb_gather_kernel", "descdb_fold_kernel",
                                             "descdb_ratio_kernel") if n in k["name"])
    assert names == ["descdb_fold_kernel", "descdb_gather_kernel", "descdb_pack_kernel", "descdb_ratio_kernel", "descdb_sweep_kernel"], names
    sweep = [k for k in mine if k["mfma"]]
    assert len(sweep) == 1 and "descdb_sweep_kernel" in sweep[0]["name"] and sweep[0]["mfma"] >= 16
    k = sweep[0]
    assert k["wg_size"] == 256 and k["alloc"] == 512 and k["scratch"] == 0, k
    for k in mine:
        assert k["scratch"] == 0, k
    named = sorted(n for k in ks for n in ("match_nn1_kernel", "match_fginn_kernel", "knn_sweep_kernel") if n in k["name"])
    assert named == ["knn_sweep_kernel", "match_fginn_kernel", "match_nn1_kernel"], named


# ---- the command line's refusals (they come before the device is looked for) ----------------------------------------------------

def _cli(tmp_path, value, key="distractorDB", env=None):
    cfg = open(os.path.join(CFG, "classic.ini")).read().replace("[Matching]\n", "[Matching]\n%s = %s\n" % (key, value), 1)
    assert key in cfg
    (tmp_path / "c.ini").write_text(cfg)
    p = subprocess.run([MODS, G1, G6, "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, env=dict(os.environ, **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stderr.decode()


def test_cli_refusals(pkg, tmp_path):
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    rng = np.random.default_rng(3)
    good = {"xy": rng.random((5, 2)), "scales": rng.random((5, 1)), "responses": rng.random((5, 1)), "A": rng.random((5, 4)),
            "descs": rng.integers(0, 256, (5, 128), dtype=np.uint8)}
    np.savez(tmp_path / "good.npz", **good)
    np.savez(tmp_path / "nodescs.npz", xy=good["xy"])
    np.savez(tmp_path / "wide.npz", descs=rng.integers(0, 256, (5, 64), dtype=np.uint8))
    np.savez(tmp_path / "floats.npz", descs=rng.random((5, 128)))
    for key in ("distractorDB", "distractorDBHalf"):
        rc, err = _cli(tmp_path, "good.npz, missing.npz", key)
        assert rc == 1 and "[Matching] %s: missing.npz" % key in err and "no MI355X" not in err, err
        rc, err = _cli(tmp_path, "nodescs.npz", key)
        assert rc == 1 and "[Matching] %s: nodescs.npz: no array descs" % key in err, err
        rc, err = _cli(tmp_path, "good.npz,wide.npz", key)
        assert rc == 1 and "[Matching] %s: wide.npz: descriptors of dimension 64" % key in err, err
        rc, err = _cli(tmp_path, "floats.npz", key)
        assert rc == 1 and "[Matching] %s: floats.npz: descs must be uint8" % key in err, err
    # with several devices the keys are ignored with a note, the files are not even opened
    rc, err = _cli(tmp_path, "missing.npz", env={"MODS_DEVICES": "0,1"})
    assert "Note: [Matching] distractorDB / distractorDBHalf are ignored with MODS_DEVICES" in err and "missing.npz" not in err, err
    import torch
    if not torch.cuda.is_available():
        # good files pass the checks; what stops the run is the missing device
        rc, err = _cli(tmp_path, "good.npz , good.npz")
        assert rc == 1 and "[Matching] distractorDB: 10 descriptors" in err and "no MI355X / HIP device available" in err, err
