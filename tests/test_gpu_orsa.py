"""ORSA on the device: the scoring kernel against the host scalar path, and mods_orsa_f against the recorded reference runs
(tests/golden/orsa_ref.npz, see test_cpu_orsa.py for how it was recorded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_cpu_orsa as cpu  # noqa: E402

pkg = cpu.pkg
W, H = cpu.W, cpu.H


def _points(n, seed, ratio=0.5):
    m = cpu._gen(n, ratio, seed)
    norm = np.float32(1.0 / np.float32(np.sqrt(np.float64(np.float32(W) * np.float32(H)))))
    p1 = ((m[:, 0:2].astype(np.float64) - [0.5 * W, 0.5 * H]) * norm).astype(np.float32).reshape(-1)
    p2 = ((m[:, 2:4].astype(np.float64) - [0.5 * W, 0.5 * H]) * norm).astype(np.float32).reshape(-1)
    return p1, p2


def _models(p1, p2, count, seed):
    rng = np.random.default_rng(seed)
    n = len(p1) // 2
    out = []
    while len(out) < count:
        k = np.sort(rng.choice(n, 7, replace=False))
        F1, F2, z, m = pkg.orsa_test_epipolar(p1, p2, k)
        for r in range(m):
            out.append(F1 + z[r] * F2)
    return np.array(out[:count], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("n,wg_keys", [(8, 4096), (9, 64), (200, 4096), (200, 256), (1000, 4096), (1000, 32768), (4096, 4096),
                                       (32768, 4096), (32769, 4096)])
def test_kernel_equals_host(n, wg_keys):
    p1, p2 = _points(n, 100 + n)
    F = _models(p1, p2, 40 if n > 5000 else 300, n)
    if n == 200:   # NaN, inf and tied keys: a zero model (0/0), points duplicated
        F[5] = 0
        p1[2:40] = p1[0:38]
        p2[2:40] = p2[0:38]
        # +inf keys: a second-image point at the origin under models with F31 = F32 = 0 has rxc = ryc = 0 (a = 0) but
        # r = F33 != 0, so r^2 (a + b) / (a b) = b / 0
        p2[80:84] = 0
        F[10:60, 6:8] = 0
        for q in (40, 41):
            x1, y1 = p1[2 * q], p1[2 * q + 1]
            f = F[20].astype(np.float64)
            rx, ry = f[0] * x1 + f[1] * y1 + f[2], f[3] * x1 + f[4] * y1 + f[5]
            assert f[8] != 0 and rx * rx + ry * ry > 0   # so the error of points 40, 41 under model 20 is +inf
    a = pkg.orsa_test_score(p1, p2, W, H, F, on_device=True, wg_keys=wg_keys)
    b = pkg.orsa_test_score(p1, p2, W, H, F, on_device=False)
    if n == 200:
        assert a[5, 3] == 1 and b[5, 3] == 1
    ok = a[:, 3] == 0   # NaN models go to the host in production; their flag must agree
    assert np.array_equal(a[:, 3], b[:, 3])
    assert np.array_equal(a[ok], b[ok])


@pytest.mark.gpu
@pytest.mark.parametrize("name", cpu.CASES)
def test_device_reproduces_reference(name):
    u6, meta = cpu.case_inputs(name)
    r = pkg.orsa_f(u6, None, int(meta[1]), int(meta[2]), seed_time=int(meta[3]))
    cpu.check_run(name, r)


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed", [("n1000", 3), ("n3000_r03", 4444), ("n1000_r01", 3)])
def test_device_equals_host_path(name, seed):
    u6, _ = cpu.case_inputs(name)
    laf = cpu._laf_from_u6(u6)
    a = pkg.orsa_f(u6, laf, W, H, seed_time=seed)
    b = pkg.orsa_f(u6, laf, W, H, seed_time=seed, on_device=False)
    for k in ("mask", "F", "index"):
        assert np.array_equal(a[k], b[k]), k
    if name != "n1000_r01":   # significant: F, the first-k list and the LAF check are exercised
        assert a["log_nfa"] < -2 and a["n"] >= 8 and np.all(a["F"] != -1)
    assert a["n"] == b["n"] and a["stats"] == b["stats"] and a["log_nfa"].view(np.uint32) == b["log_nfa"].view(np.uint32)


@pytest.mark.gpu
def test_independent_of_threads_batch_and_packing():
    name = "n300_r02"
    u6, meta = cpu.case_inputs(name)
    for batch, wg in ((1, 256), (64, 32768), (5000, 1024)):
        r = pkg.orsa_f(u6, None, W, H, seed_time=int(meta[3]), batch=batch, wg_keys=wg)
        cpu.check_run(name, r)
    code = ("import sys; sys.path.insert(0, %r); import test_cpu_orsa as c; u6, m = c.case_inputs(%r); "
            "r = c.pkg.orsa_f(u6, None, 800, 640, seed_time=int(m[3])); c.check_run(%r, r); print('ok')"
            % (os.path.join(ROOT, "tests"), name, name))
    env = dict(os.environ, MODS_RANSAC_THREADS="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.gpu
def test_verify_tentatives_wh_equals_orsa_f():
    u6, meta = cpu.case_inputs("n1000")
    laf = cpu._laf_from_u6(u6)
    par = pkg.PairParams.default()
    par.ransac = pkg.RansacParams.default(useF=2)
    par.dup_dist = 0
    tent = np.zeros(len(u6), pkg.TENT_DTYPE)
    tent["q"] = np.arange(len(u6))
    tv, uv, lv, nu, Hm, stats = pkg.verify_tentatives(tent, u6, laf, par, seed_time=int(meta[3]), wh=(W, H))
    r = pkg.orsa_f(u6, laf, W, H, seed_time=int(meta[3]), on_device=False)
    assert nu == len(u6) and np.array_equal(tv["q"], np.nonzero(r["mask"])[0]) and np.array_equal(Hm, r["F"])
    assert stats == r["stats"]


def _oracle_unique(img1, img2):
    """the unique tentatives of one identity-view step, through the CPU oracle chain (the device's lists equal them)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc
    import pipeline_oracle as po
    (ra, _), (rb, _) = po.pmap(orc.detect_describe, (img1, img2))
    tc = po.match_fginn_par(ra, rb, 0.8)
    un = orc.duplicate_filter(tc, ra, rb, 2.0, 1)
    return len(tc), po.u6_of(ra, rb, un), po.laf_of(ra, rb, un)


def _grey(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.float32)


@pytest.mark.gpu
def test_match_pair_dev_graf_orsa():
    """mods_match_pair_dev with useF = 2 on graf 1 / 6: the same verified list, F and counts as the host-path ORSA on the
    oracle's unique tentatives, with the frame size passed through"""
    import torch
    a = _grey(os.path.join(ROOT, "tests", "golden", "graf1.png"))
    b = _grey(os.path.join(ROOT, "tests", "golden", "graf6.png"))
    assert a.shape == b.shape
    h, w = a.shape
    n_tc, u6, laf = _oracle_unique(a, b)
    want = pkg.orsa_f(u6, laf, w, h, seed_time=77, on_device=False)
    ctx = pkg.Context(0, w, h, 2)
    t = torch.from_numpy(np.stack([a, b])).cuda(0)
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    par.ransac = pkg.RansacParams.default(useF=2)
    pkg.ransac_pin_seed(77)
    res, m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, params=par, max_matches=100000)
    ctx.close()
    assert res.n_tentatives == n_tc and res.n_unique == len(u6) > 50
    assert res.n_inliers == want["n"] == len(m)
    assert np.array_equal(m, u6[want["mask"]][:, [0, 1, 3, 4]])
    assert np.array_equal(np.array(res.H), want["F"])
    assert [res.ransac_samples, res.ransac_lo, res.ransac_rejects] == want["stats"]


@pytest.mark.gpu
def test_ladder_orsa_equals_host_path():
    """mods_match_ladder_dev with useF = 2 on a pair of different sizes: ORSA runs on the gathered unique tentatives with
    ((w1 + w2) / 2, (h1 + h2) / 2), as mods.cpp:347-350 passes it"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    w, h = 640, 480
    a, b, _ = synth.pair(w, h, seed=41)
    b = np.ascontiguousarray(b[:h - 37, :w - 51])
    h2, w2 = b.shape
    n_tc, u6, laf = _oracle_unique(a, b)
    wa, ha = (w + w2) // 2, (h + h2) // 2
    want = pkg.orsa_f(u6, laf, wa, ha, seed_time=31, on_device=False)
    other = pkg.orsa_f(u6, laf, w, h, seed_time=31, on_device=False)
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    rep1, rep2 = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
    t1 = torch.from_numpy(a).cuda()
    t2 = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    par.ransac = pkg.RansacParams.default(useF=2)
    pkg.ransac_pin_seed(31)
    res, m = pkg.match_ladder_dev(ctx, t1.data_ptr(), w, h, [pkg.LadderStep.make((1,), 360.0)], rep1, rep2, params=par,
                                  max_matches=100000, img2_ptr=t2.data_ptr(), w2=w2, h2=h2)
    rep1.close(); rep2.close(); ctx.close()
    assert res.n_tentatives == n_tc and res.n_unique == len(u6) > 50
    assert res.n_inliers == want["n"] == len(m) >= 8
    assert np.array_equal(m, u6[want["mask"]][:, [0, 1, 3, 4]])
    assert np.array_equal(np.array(res.H), want["F"])
    assert not np.array_equal(want["F"], other["F"])   # the averaged size matters: the frame of image 1 alone gives another F
