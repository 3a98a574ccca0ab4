"""The k-nearest-neighbour search (csrc/knn.hip) without a device: its symbols, its refusals, the grid of its sweep, the resources of
its matrix-core kernel read from the built library, and the numpy statement of its contract (tests/match_ref.py::neighbours) against a
double loop."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import match_cases as mc
import match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUF = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before anything is read
E_ARG = -2


def test_symbols_are_exported(pkg):
    for name in ("mods_match_knn", "mods_match_knn_dev", "mods_match_knn_reps", "mods_match_knn_grid", "mods_ctx_knn_splits"):
        assert hasattr(pkg.lib(), name), name
    assert pkg.stage_index("knn") + 1 == pkg.stage_index("knn_sweep") == pkg.stage_index("spatial_select") + 2
    header = open(os.path.join(ROOT, "include", "mods_hip.h")).read()
    assert header.index("MODS_STAGE_SPATIAL_SELECT,") < header.index("MODS_STAGE_KNN,") < header.index("MODS_STAGE_KNN_SWEEP,") < header.index("MODS_STAGE_COUNT")


def _refused(pkg, rc, prefix, part):
    err = pkg.lib().mods_last_error()
    assert rc == E_ARG and err.startswith(prefix) and part in err, (rc, err)


def test_refusals(pkg):
    L = pkg.lib()
    out = (C.c_int * 64)()
    # mods_match_knn: null context, null lists, both outputs null, k out of range, negative counts
    _refused(pkg, L.mods_match_knn(None, BUF, 1, BUF, 1, 1, out, out), b"match_knn: ", b"null")
    _refused(pkg, L.mods_match_knn(BUF, None, 1, BUF, 1, 1, out, out), b"match_knn: ", b"null")
    _refused(pkg, L.mods_match_knn(BUF, BUF, 1, None, 1, 1, out, out), b"match_knn: ", b"null")
    _refused(pkg, L.mods_match_knn(BUF, BUF, 1, BUF, 1, 1, None, None), b"match_knn: ", b"both outputs")
    for k in (0, -1, 65, 1 << 20):
        _refused(pkg, L.mods_match_knn(BUF, BUF, 1, BUF, 1, k, out, None), b"match_knn: ", b"k = %d" % k)
    _refused(pkg, L.mods_match_knn(BUF, BUF, -1, BUF, 1, 1, out, None), b"match_knn: ", b"negative")
    _refused(pkg, L.mods_match_knn(BUF, BUF, 1, BUF, -1, 1, out, None), b"match_knn: ", b"negative")
    # mods_match_knn_dev
    _refused(pkg, L.mods_match_knn_dev(None, 0, 1, 1, out, out), b"match_knn_dev: ", b"null")
    _refused(pkg, L.mods_match_knn_dev(BUF, 0, 1, 1, None, None), b"match_knn_dev: ", b"both outputs")
    for k in (0, 65):
        _refused(pkg, L.mods_match_knn_dev(BUF, 0, 1, k, None, out), b"match_knn_dev: ", b"k = %d" % k)
    # mods_match_knn_reps
    _refused(pkg, L.mods_match_knn_reps(None, BUF, 0, 1, BUF, 1, out, out), b"match_knn_reps: ", b"null")
    _refused(pkg, L.mods_match_knn_reps(BUF, None, 0, 1, BUF, 1, out, out), b"match_knn_reps: ", b"null")
    _refused(pkg, L.mods_match_knn_reps(BUF, BUF, 0, 1, None, 1, out, out), b"match_knn_reps: ", b"null")
    _refused(pkg, L.mods_match_knn_reps(BUF, BUF, 0, 1, BUF, 1, None, None), b"match_knn_reps: ", b"both outputs")
    for k in (0, 65):
        _refused(pkg, L.mods_match_knn_reps(BUF, BUF, 0, 1, BUF, k, out, None), b"match_knn_reps: ", b"k = %d" % k)
    # the knob and the grid
    _refused(pkg, L.mods_ctx_knn_splits(None, 0), b"knn_splits: ", b"null")
    _refused(pkg, L.mods_ctx_knn_splits(BUF, -1), b"knn_splits: ", b"negative")
    g = (C.c_int * 3)()
    for args in ((10, 10, 1, 0, None), (-1, 10, 1, 0, g), (10, -1, 1, 0, g), (10, 10, 0, 0, g), (10, 10, 65, 0, g), (10, 10, 1, -1, g)):
        _refused(pkg, L.mods_match_knn_grid(*args), b"match_knn_grid: ", b"")


class _Bank(C.Structure):
    """the layout of mods_imgrep (csrc/imgrep.hip): device, stream, the region buffer's pointer and capacity, cap, n - a bank without
    a device, of which the refusals read n alone"""
    _fields_ = [("device", C.c_int), ("stream", C.c_void_p), ("reg", C.c_void_p), ("reg_cap", C.c_size_t), ("cap", C.c_int), ("n", C.c_int)]


def test_range_and_capacity_refusals(pkg):
    """the refusals that read a bank's length or the context's capacity, without a device: a dummy bank of 10 regions, and zeroed
    memory in the place of a context (capacity 0, nothing described), of which the refusals read max_cand and the counts of the last
    described batch and nothing else"""
    L = pkg.lib()
    out = (C.c_int * 64)()
    bank = _Bank(0, None, None, 0, 16, 10)
    b = C.byref(bank)
    for q0, q1 in ((5, 4), (-1, 3), (0, 11), (11, 11), (3, 12)):
        _refused(pkg, L.mods_match_knn_reps(BUF, b, q0, q1, b, 5, out, None), b"match_knn_reps: ", b"bad query range [%d, %d) of 10" % (q0, q1))
    ctx0 = C.create_string_buffer(4 << 20)              # larger than any mods_ctx, all zero
    for rc in (L.mods_match_knn_reps(ctx0, b, 0, 5, b, 5, out, None), L.mods_match_knn(ctx0, BUF, 1, BUF, 1, 1, out, None),
               L.mods_match_knn(ctx0, BUF, 0, BUF, 1, 1, out, None)):
        assert rc == -3 and b"list larger than the context capacity" in L.mods_last_error(), (rc, L.mods_last_error())
    _refused(pkg, L.mods_match_knn_dev(ctx0, 0, 0, 5, out, None), b"match_knn_dev: ", b"image index outside")
    _refused(pkg, L.mods_match_knn_dev(ctx0, -1, 0, 5, out, None), b"match_knn_dev: ", b"image index outside")


def test_grid(pkg):
    """the sweep's grid: the tiles are covered, a forced split count is honoured while the list has that many tiles, the query blocks
    cover the queries, and more queries never mean fewer query blocks or more splits"""
    for n_t in (0, 1, 31, 32, 33, 587, 2500, 10000, 47177):
        n_tiles = (n_t + 31) // 32
        for k in (1, 2, 10, 50, 64):
            for forced in (0, 1, 2, 3, 7, 64, 1000):
                prev = None
                for n_q in (0, 1, 255, 256, 257, 3000, 10000, 60156):
                    qb, splits, tps = pkg.knn_grid(n_q, n_t, k, forced)
                    assert splits >= 1 and tps * splits >= n_tiles, (n_q, n_t, k, forced)
                    assert qb * 256 >= n_q > (qb - 1) * 256 or (n_q == 0 and qb == 0)
                    assert splits <= 64
                    if forced > 0:
                        assert splits == max(1, min(forced, n_tiles, 64))
                    if prev is not None:
                        assert qb >= prev[0] and splits <= prev[1] and tps >= prev[2]
                    prev = (qb, splits, tps)
    # the sizes the timing tool reports (profiles/knn_timing.txt)
    assert pkg.knn_grid(60156, 47177, 50) == (235, 2, 738)
    assert pkg.knn_grid(10000, 10000, 64) == (40, 4, 79)


def _kernel_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr


def test_knn_sweep_owns_its_simds(pkg):
    """the co-residency rule (DESIGN.md "The matcher and its neighbours") for the new matrix-core kernel, read from the built library:
    a workgroup of a multiple of 256 threads whose waves fill the 512-entry register file of each SIMD, no scratch; and the new kernel
    is no further instantiation of the matcher's two"""
    kr = _kernel_resources()
    if not os.path.exists(os.path.join(kr.LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump")
    ks = kr.kernels(os.path.join(ROOT, "mods-light-zmq_amd", "libmodsgpu.so"))
    knn = [k for k in ks if "knn" in k["name"]]
    assert any("knn_sweep_kernel" in k["name"] for k in knn) and any("knn_merge_kernel" in k["name"] for k in knn)
    sweep = [k for k in knn if k["mfma"]]
    assert len(sweep) == 1 and "knn_sweep_kernel" in sweep[0]["name"] and sweep[0]["mfma"] >= 8
    for k in sweep:
        per_simd = k["wg_size"] // 64 // 4
        assert k["wg_size"] % 256 == 0 and per_simd >= 1 and k["alloc"] * per_simd == 512 and k["scratch"] == 0, k
    for k in knn:
        assert k["scratch"] == 0, k
    named = sorted(n for k in ks for n in ("match_nn1_kernel", "match_fginn_kernel") if n in k["name"])
    assert named == ["match_fginn_kernel", "match_nn1_kernel"], named
    assert not any("match_nn1_kernel" in k["name"] or "match_fginn_kernel" in k["name"] for k in knn)


def test_neighbours_against_a_double_loop():
    """match_ref.neighbours - the statement the GPU tests lean on - on 40 x 70 descriptors with planted ties: equal trains, trains at
    equal distances from a query, and ties across position k"""
    rng = np.random.default_rng(77)
    q, t = mc.random_regions(40, rng), mc.random_regions(70, rng)
    t["desc"][5] = t["desc"][50]; t["desc"][51] = t["desc"][50]                 # equal trains
    for i in range(10):
        for c, row in enumerate((3 + i, 20 + i, 60 - i)):                       # three trains at one distance from query i
            t["desc"][row] = mc.plant(q["desc"][i], 40 + i, start=10 * c)
        t["desc"][35 + i] = q["desc"][10 + i]                                   # distance 0
    qd, td = q["desc"].astype(np.int64), t["desc"].astype(np.int64)
    d = np.empty((40, 70), np.int64)
    for i in range(40):
        for j in range(70):
            d[i, j] = int(((qd[i] - td[j]) ** 2).sum())
    assert (d[np.arange(10), 3 + np.arange(10)] == 40 + np.arange(10)).all() and (d[10 + np.arange(10), 35 + np.arange(10)] == 0).all()
    for k in (1, 2, 3, 50, 64, 70):
        dist, index = ref.neighbours(q, t, k)
        assert dist.shape == index.shape == (40, k)
        for i in range(40):
            order = sorted(range(70), key=lambda j: (d[i, j], j))[:k]
            assert index[i].tolist() == order and dist[i].tolist() == [int(d[i, j]) for j in order], (k, i)
