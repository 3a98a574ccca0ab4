"""-m gpu tests that pin what a context and the thread-local verification workspaces compute ACROSS a growth of their device and
pinned buffers: a call behind a reallocation gives what a fresh owner gives for that call alone."""
import threading

import numpy as np
import pytest

import fsynth
import synth

pytestmark = pytest.mark.gpu


def _dd_call(pkg, ctx, t, n_img, w, h, det=None, desc=None):
    """one detect + describe call on the device batch t; the regions of every image as whole records"""
    _, nr = ctx.detect_describe_dev(t.data_ptr(), n_img, w, h, det, desc)
    regs = [ctx.regions_fetch(i) for i in range(n_img)]
    assert [len(r) for r in regs] == nr
    return regs


def test_context_regrows_its_pools(pkg):
    """A small batch, then a large one (plane, dedup-map and description pools grow: recordings are dropped), three orientations
    per keypoint (first allocation of the multi-orientation table), the DoG detector (response scratch planes), the small batch
    again - every call equals the same call on a fresh context."""
    import torch
    small = torch.from_numpy(synth.texture(160, 120, seed=5)[None]).cuda(0)
    big = torch.from_numpy(np.stack([synth.texture(640, 480, seed=6), synth.texture(640, 480, seed=7)])).cuda(0)
    torch.cuda.synchronize()
    ori3 = pkg.DescribeParams.default()
    ori3.ori_maxAngles = 3
    calls = {"small": (small, 1, 160, 120, None, None), "big": (big, 2, 640, 480, None, None),
             "ori3": (big, 2, 640, 480, None, ori3), "dog": (big, 2, 640, 480, pkg.HessAffParams.dog(), None)}
    want = {}
    for name, args in calls.items():           # each reference from a context that made only that call
        fresh = pkg.Context(0, 640, 480, batch=2)
        want[name] = _dd_call(pkg, fresh, *args)
        fresh.close()
    ctx = pkg.Context(0, 640, 480, batch=2)
    ctx.graphs(True)
    for step, name in enumerate(["small", "small", "big", "big", "big", "ori3", "dog", "small"]):
        got = _dd_call(pkg, ctx, *calls[name])
        for i, (g, e) in enumerate(zip(got, want[name])):
            assert np.array_equal(g, e), (step, name, i, len(g), len(e))
    ctx.close()
    assert min(len(r) for r in want["big"]) > 200
    assert all(len(a) > len(b) for a, b in zip(want["ori3"], want["big"]))


def _h_corr(n, seed):
    """n correspondences (x1 y1 1 x2 y2 1), 60 % of them on one homography"""
    rng = np.random.default_rng(seed)
    H = np.array([[1.05, 0.08, 12.0], [-0.06, 0.97, -7.0], [8e-5, -4e-5, 1.0]])
    x1 = rng.uniform(0, 1000.0, (n, 2))
    p = np.c_[x1, np.ones(n)] @ H.T
    x2 = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (n, 2))
    out = rng.permutation(n)[:n - int(round(n * 0.6))]
    x2[out] = rng.uniform(0, 1000.0, (len(out), 2))
    return np.c_[x1, np.ones(n), x2, np.ones(n)]


def _in_thread(fn):
    """fn() in a fresh thread: the verification entry points keep their device workspace per thread"""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:   # noqa: BLE001 - reported in the caller's thread
            box["error"] = e
    th = threading.Thread(target=run)
    th.start()
    th.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def _assert_same_verdict(got, want, what):
    (mask, M, n, stats), (mask_w, M_w, n_w, stats_w) = got, want
    assert n == n_w and stats == stats_w, (what, n, n_w, stats, stats_w)
    assert np.array_equal(mask, mask_w) and np.array_equal(M, M_w), what


@pytest.mark.parametrize("model", ["h", "f"])
def test_ransac_workspace_regrows(pkg, model):
    """100 correspondences, 20 000 (above the 16 384-element floor of the workspace's per-correspondence buffers), 100 again in
    ONE thread: each verdict equals that of the same call in a thread of its own."""
    if model == "h":
        sets = [_h_corr(100, 1), _h_corr(20000, 2)]
        call = lambda u: pkg.loransac_h(u, None, seed_time=4242)
    else:
        sets = [fsynth.two_view(100, inlier_ratio=0.6, seed=1)[0], fsynth.two_view(20000, inlier_ratio=0.6, seed=2)[0]]
        call = lambda u: pkg.loransac_f(u, None, seed_time=4242)
    seq = [sets[0], sets[1], sets[0]]
    want = [_in_thread(lambda u=u: call(u)) for u in sets]
    got = _in_thread(lambda: [call(u) for u in seq])
    assert want[0][2] > 30 and want[1][2] > 6000, (want[0][2], want[1][2])
    for k, (g, e) in enumerate(zip(got, [want[0], want[1], want[0]])):
        _assert_same_verdict(g, e, (model, k))


def test_baumberg_stats_toggle(pkg):
    """Enabling the counters again frees, allocates and clears them: the same detection counts the same work both times."""
    img = synth.texture(640, 480, seed=78)
    ctx = pkg.Context(0, 640, 480, 1)
    reads = []
    for _ in range(2):
        ctx.baumberg_stats_enable(True)
        keys = ctx.detect_hessian_affine(img)
        reads.append(ctx.baumberg_stats(0))
    ctx.close()
    kp, it = reads[0]
    assert reads[1] == reads[0]
    assert kp >= len(keys) > 200 and kp <= it <= 16 * kp     # test_baumberg_work_counters' expectation for this image
