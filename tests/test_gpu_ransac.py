"""-m gpu parity tests: GPU-scored LO-RANSAC (degensac C ABI of libmodsgpu) vs the reference's
own degensac compiled from /root/reference (oracle/_ref), same pinned seed."""
import numpy as np
import pytest

import refdeg

pytestmark = pytest.mark.gpu


def make_corr(n, inlier_ratio, noise, seed, w=1000.0):
    rng = np.random.default_rng(seed)
    H = np.array([[1.05, 0.08, 12.0], [-0.06, 0.97, -7.0], [8e-5, -4e-5, 1.0]])
    x1 = rng.uniform(0, w, (n, 2))
    p = np.c_[x1, np.ones(n)] @ H.T
    x2 = p[:, :2] / p[:, 2:] + rng.normal(0, noise, (n, 2))
    n_out = n - int(round(n * inlier_ratio))
    idx = rng.permutation(n)[:n_out]
    x2[idx] = rng.uniform(0, w, (n_out, 2))
    return np.c_[x1, np.ones(n), x2, np.ones(n)]


def _compare(got, want):
    assert got["samples"] == want["samples"], (got["samples"], want["samples"])
    assert got["lo"] == want["lo"] and got["rej"] == want["rej"]
    assert got["I"] == want["I"]
    if want["I"] == 0:
        # no model was ever accepted: the reference fills inl[] from a malloc'ed, never written
        # error buffer (exp_ranH.c:841,1199-1212) - undefined, not comparable
        assert not np.any(got["H"])
        return
    assert np.array_equal(got["inl"], want["inl"])
    assert abs(got["J"] - want["J"]) <= 1e-9 * max(1.0, abs(want["J"]))
    hg, hw = got["H"] / np.linalg.norm(got["H"]), want["H"] / np.linalg.norm(want["H"])
    if np.dot(hg, hw) < 0:
        hg = -hg
    assert np.max(np.abs(hg - hw)) < 1e-7


@pytest.mark.skipif(not refdeg.available(), reason="oracle/_ref not built")
# Not compared: inlier sets of 8-9 points.  exp_inHranicustom then draws 4-point subsets and u2h's
# len == 4 branch transposes a 9x9 stack buffer of which only 72 entries were written
# (Htools.c:107-114): the reference's result depends on uninitialised memory there.
@pytest.mark.parametrize("n,ratio,noise", [(12, 1.0, 0.1), (20, 0.8, 0.5), (21, 0.6, 0.5), (100, 0.5, 0.5), (500, 0.5, 0.5),
                                           (500, 0.25, 1.0), (2000, 0.3, 0.8), (1000, 0.1, 0.5), (300, 0.0, 0.5),
                                           # list lengths on the chunk edges of the two gain kernels (128 and 384 rows)
                                           (128, 0.5, 0.5), (129, 0.5, 0.5), (384, 0.5, 0.5), (385, 0.5, 0.5)])
@pytest.mark.parametrize("seed", [12345, 7])
def test_ransac_h_matches_reference(pkg, n, ratio, noise, seed):
    u = make_corr(n, ratio, noise, seed + n)
    max_sam = 1000 if n <= 20 else 20000
    for err, sym in (("sampson", 1), ("sampson", 0), ("symm_sum", 1), ("symm_max", 0)):
        want = refdeg.ransac_h(u, 16.0, max_sam=max_sam, err=err, sym_check=sym, seed_time=seed)
        got = pkg.ransac_h(u, 16.0, max_sam=max_sam, err=err, sym_check=sym, seed_time=seed)
        _compare(got, want)


@pytest.mark.skipif(not refdeg.available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("seed", [12345, 7])
def test_ransac_h_stops_one_sample_into_a_batch(pkg, seed):
    """max_sam = 73 ends the run one sample into the third scoring batch (8, then 64, then 128 samples); the reference accepts a
    model within its 73 samples for every error type here, so each comparison compares one"""
    u = make_corr(500, 0.25, 1.0, seed + 500)
    for err, sym in (("sampson", 1), ("sampson", 0), ("symm_sum", 1), ("symm_max", 0)):
        want = refdeg.ransac_h(u, 16.0, max_sam=73, err=err, sym_check=sym, seed_time=seed)
        assert want["samples"] == 73 and want["I"] > 0
        _compare(pkg.ransac_h(u, 16.0, max_sam=73, err=err, sym_check=sym, seed_time=seed), want)


@pytest.mark.skipif(not refdeg.available(), reason="oracle/_ref not built")
def test_ransac_h_large(pkg):
    u = make_corr(12000, 0.2, 0.7, 99)
    want = refdeg.ransac_h(u, 16.0, seed_time=4242)
    got = pkg.ransac_h(u, 16.0, seed_time=4242)
    _compare(got, want)


def test_ransac_properties(pkg):
    """Size-independent properties: determinism under a pinned seed, inliers consistent with H."""
    u = make_corr(3000, 0.4, 0.5, 5)
    a = pkg.ransac_h(u, 16.0, seed_time=1)
    b = pkg.ransac_h(u, 16.0, seed_time=1)
    assert np.array_equal(a["inl"], b["inl"]) and a["samples"] == b["samples"] and np.array_equal(a["H"], b["H"])
    assert abs(int(a["I"]) - 1200) < 60
    mask, H, ninl, stats = pkg.loransac_h(u, None, seed_time=1)
    assert ninl == mask.sum() and ninl > 1000
    p = np.c_[u[:, 0], u[:, 1], np.ones(len(u))] @ H.T
    err = np.hypot(p[:, 0] / p[:, 2] - u[:, 3], p[:, 1] / p[:, 2] - u[:, 4])
    assert np.all(err[mask] < 10.0)
    few = pkg.loransac_h(u[:7], None)
    assert few[2] == 0 and np.all(few[1] == -1)
