"""The spatial selection of the count modes' cut (mods_ctx_spatial_selection, csrc/spatial_select.hip) without a GPU: the numpy
restatement (tests/spatial_select_ref.py) on cases worked out on paper, the constructed lists of the GPU tests held to what they are
built to show, the argument checks of the library, and the command line's [SpatialSelection] keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spatial_select_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
INF = float("inf")
BUF = C.create_string_buffer(64)      # stands in for a context where the arguments are refused before it is looked at


def test_four_collinear_points():
    """x = 0, 1, 3, 7 on a line, responses 4, 3, 2, 1.  c = 1: every key is suppressed by its left neighbour, r2 = inf, 1, 4, 16.
    c = 0.5: only the last key has suppressors (0.5 * 4 and 0.5 * 3 exceed 1, 0.5 * 2 does not): r2[3] = min(49, 36)."""
    x, y, r = [0, 1, 3, 7], [0, 0, 0, 0], [4, -3, 2, -1]
    assert ref.radii(x, y, r, 1.0).tolist() == [INF, 1.0, 4.0, 16.0]
    assert ref.select(x, y, r, 1, 1.0).tolist() == [0]
    assert ref.select(x, y, r, 2, 1.0).tolist() == [0, 3]
    assert ref.select(x, y, r, 3, 1.0).tolist() == [0, 2, 3]
    assert ref.radii(x, y, r, 0.5).tolist() == [INF, INF, INF, 36.0]
    assert ref.select(x, y, r, 2, 0.5).tolist() == [0, 1]          # three radii of inf: the smaller indices
    assert ref.select(x, y, r, 3, 0.5).tolist() == [0, 1, 2]


def test_equal_responses_do_not_suppress_each_other():
    """responses 5, -5, 1 at x = 0, 3, 10 with c = 1: neither of the first two is strictly stronger than the other"""
    x, y, r = [0, 3, 10], [0, 0, 0], [5, -5, 1]
    assert ref.radii(x, y, r, 1.0).tolist() == [INF, INF, 49.0]
    assert ref.select(x, y, r, 2, 1.0).tolist() == [0, 1]
    assert ref.select(x, y, r, 1, 1.0).tolist() == [0]


def test_coincident_points():
    """two keys on one spot: the weaker has r2 = 0 and goes last, behind a weaker key that stands alone"""
    x, y, r = [5, 5, 9], [2, 2, 2], [2, 1, 0.5]
    assert ref.radii(x, y, r, 1.0).tolist() == [INF, 0.0, 16.0]
    assert ref.select(x, y, r, 2, 1.0).tolist() == [0, 2]


def test_fp32_rounding_of_each_operation():
    """dx * dx and dy * dy are rounded before they are added: 4097^2 = 16785409 is not a float, nor is its sum with 1"""
    x, y, r = [0, 4097], [0, 1], [2, 1]
    dx2 = np.float32(4097) * np.float32(4097)
    assert float(dx2) == 16785408.0
    assert ref.radii(x, y, r, 1.0)[1] == dx2 + np.float32(1) == np.float32(16785408.0)
    # c * a is rounded to float before it is compared: 0.75 * (1 + 3 ulp) = 0.75 + 4.5 ulp' exactly, 0.75 + 4 ulp' as a float (the
    # tie goes to the even mantissa), which is the weaker key's response: no suppressor, where the exact product would be one
    ulp = np.float32(2.0 ** -23)
    strong, weak = np.float32(1) + np.float32(3) * ulp, np.float32(0.75) + np.float32(2) * ulp
    assert np.float32(0.75) * strong == weak and 0.75 * np.float64(strong) > np.float64(weak)
    assert ref.radii([0, 1], [0, 0], [strong, weak], 0.75).tolist() == [INF, INF]
    assert ref.radii([0, 1], [0, 0], [strong, weak], 1.0).tolist() == [INF, 1.0]


@pytest.mark.parametrize("n", [1, 2, 65, 700])
def test_no_robustness_is_the_prefix_cut_and_the_output_is_ordered(n):
    x, y, r = ref.random_list(n, seed=n)
    for keep in (0, 1, n // 3, n - 1, n, n + 7):
        assert ref.select(x, y, r, keep, 0.0).tolist() == list(range(max(0, min(keep, n))))
        for c in (1.0, 0.9):
            idx = ref.select(x, y, r, keep, c)
            assert len(idx) == max(0, min(keep, n)) and np.all(np.diff(idx) > 0)
            assert len(idx) == 0 or (idx[0] == 0 and idx[-1] < n)                # the strongest key has no suppressor
    assert ref.keep_count(2, n, 50) == min(n, 50) and ref.keep_count(3, n, relative_regions_number=0.5) == n // 2
    assert ref.keep_count(3, 10, relative_regions_number=0.3) == 3               # floor((double)0.3f * 10) = floor(3.0000001)


def test_constructed_lists_are_what_they_are_built_to_be():
    x, y, r = ref.clustered_scene()
    a = np.abs(r)
    assert len(r) == 400 and np.all(np.diff(a) < 0)
    assert np.all((x[:300] >= 100) & (x[:300] <= 110) & (y[:300] >= 100) & (y[:300] <= 110))
    got = ref.select(x, y, r, 100, 1.0)
    assert got[0] == 0 and np.count_nonzero(got >= 300) == 99 and len(got) == 100
    assert np.count_nonzero(np.arange(100) >= 300) == 0                           # the plain cut holds none of them
    x, y, r = ref.equal_radius_list()
    r2 = ref.radii(x, y, r, 0.9)
    assert len(r) == 101 and r2[0] == INF and np.all(r2[1:] == 625.0)
    assert ref.select(x, y, r, 40, 0.9).tolist() == list(range(40))
    x, y, r = ref.lattice_list()
    r2 = ref.radii(x, y, r, 1.0)
    assert len(np.unique(r2)) < 40 and np.count_nonzero(r2 == 1.0) > 300          # many equal radii: the index decides
    x, y, r = ref.tied_response_list()
    assert len(np.unique(np.abs(r))) == 50 and (r > 0).any() and (r < 0).any()
    assert np.all(ref.radii(x, y, r, 1.0)[:10] == INF)                            # the first block: ten equal maxima
    x, y, r = ref.duplicate_position_list()
    assert np.count_nonzero(ref.radii(x, y, r, 1.0) == 0.0) > 300


def test_arguments_are_refused_without_a_device(pkg):
    lib = pkg.lib()
    d = C.c_double
    for mode, c, word in ((3, 0.9, b"mode 3"), (-1, 0.9, b"mode -1"), (1, 1.5, b"robustness 1.5"), (1, -0.1, b"robustness -0.1"),
                          (0, 2.0, b"robustness 2"), (1, float("nan"), b"robustness")):
        assert lib.mods_ctx_spatial_selection(BUF, mode, d(c)) == -2
        err = lib.mods_last_error()
        assert err.startswith(b"spatial_selection: ") and word in err, err
        assert lib.mods_pipeline_spatial_selection(BUF, mode, d(c)) == -2 and b"spatial_selection" in lib.mods_last_error()
    for mode in (0, 1, 2):
        assert lib.mods_ctx_spatial_selection(None, mode, d(0.9)) == -2 and b"null context" in lib.mods_last_error()
        assert lib.mods_pipeline_spatial_selection(None, mode, d(0.9)) == -2 and b"null pipeline" in lib.mods_last_error()
    assert lib.mods_ctx_spatial_selection_get(None, None, None) == -2
    n = C.c_int()
    assert lib.mods_test_spatial_select(None, None, 1, C.byref(n), 1, C.byref(n), d(0.9), C.byref(n), C.byref(n)) == -2
    assert lib.mods_test_spatial_select(BUF, None, 1, C.byref(n), 1, C.byref(n), d(7.0), C.byref(n), C.byref(n)) == -2
    assert b"robustness 7" in lib.mods_last_error()
    # the stage id follows the existing ones, which keep their values
    assert pkg.stage_index("spatial_select") == 23 and pkg.stage_index("reproject_h") == 22 and pkg.stage_index("local_affine") == 21
    header = open(os.path.join(ROOT, "include", "mods_hip.h")).read()
    for decl in ("int mods_ctx_spatial_selection(mods_ctx *ctx, int mode, double robustness);",
                 "int mods_ctx_spatial_selection_get(const mods_ctx *ctx, int *mode, double *robustness);",
                 "int mods_pipeline_spatial_selection(mods_pipeline *p, int mode, double robustness);"):
        assert decl in header, decl
    assert header.index("MODS_STAGE_REPROJECT_H,") < header.index("MODS_STAGE_SPATIAL_SELECT,") < header.index("MODS_STAGE_COUNT")


def _run_cli(tmp_path, section):
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    ini = open(os.path.join(CFG, "classic.ini")).read()
    (tmp_path / "c.ini").write_text(ini + "\n" + section + "\n")
    p = subprocess.run([MODS, G1, G6, "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stderr.decode()


@pytest.mark.parametrize("value", ["1.5", "abc", "-0.2", "0.5x", "nan"])
def test_cli_refuses_a_bad_robustness_before_anything_runs(pkg, tmp_path, value):
    rc, err = _run_cli(tmp_path, "[SpatialSelection]\ndoSpatialSelection = 1\nrobustness = %s" % value)
    assert rc == 1 and "[SpatialSelection] robustness must be a number in [0, 1], not " + value in err, err
    assert "Image1:" not in err and "HIP device" not in err and not os.path.exists(tmp_path / "m")    # no image read, no device asked for


def test_cli_refuses_a_bad_switch(pkg, tmp_path):
    rc, err = _run_cli(tmp_path, "[SpatialSelection]\ndoSpatialSelection = 2")
    assert rc == 1 and "doSpatialSelection must be 0 or 1" in err and "Image1:" not in err
