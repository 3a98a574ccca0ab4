"""ORSA-H (useF = 3) on the device: the scoring kernel's homography instantiation - solve phase, keys, sort, NFA scan - and
whole mods_orsa_h calls, bit exact against the host path (test_cpu_orsa_h.py pins that path to the numpy restatement); the pair,
ladder and command-line routes to it."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orsa_h_ref as ref  # noqa: E402
import test_cpu_orsa_h as cpu  # noqa: E402

pkg = cpu.pkg
W, H = ref.W, ref.H
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
G1, G6 = (os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png"))
HGT = np.array([[0.42, -0.66, 453.6], [0.44, 1.01, -46.5], [5.2e-4, -8e-5, 1.0]])   # graf H1to6, as test_cpu_oracle.py holds it
_cache = {}


def _points(n, seed):
    u6, _, _ = ref.scene(n, 0.5, 1.0, seed)
    norm = np.float32(1.0 / np.float32(np.sqrt(np.float64(np.float32(W) * np.float32(H)))))
    p1 = ((u6[:, 0:2] - [0.5 * W, 0.5 * H]) * norm).astype(np.float32)
    p2 = ((u6[:, 3:5] - [0.5 * W, 0.5 * H]) * norm).astype(np.float32)
    return p1, p2


# P = the power-of-two segment of n, G = models per workgroup: (5, 64) G = 8; (5, 4096) G = 256, the cap; (6, 256) G = 32;
# (200, 256) and (1000, 64) G = 1 in LDS; (200, 4096) G = 16; (1000, 4096) G = 4; 33000: P = 65536, the HBM tier.  m is no
# multiple of G wherever G > 1.
@pytest.mark.gpu
@pytest.mark.parametrize("n,wg_keys,m", [(5, 64, 301), (5, 4096, 301), (6, 256, 301), (9, 64, 301), (200, 256, 150), (200, 4096, 301),
                                         (1000, 64, 60), (1000, 4096, 301), (4096, 4096, 40), (33000, 4096, 3)])
def test_kernel_equals_host(n, wg_keys, m):
    p1, p2 = _points(n, 300 + n)
    samples = cpu.random_samples(n, m, n)
    bad = []
    if n >= 9:   # invalid models among valid ones of one workgroup: a duplicated correspondence (zero pivot), tied keys
        p1[7], p2[7] = p1[3], p2[3]
        bad = [1, 2, 5, m - 1] if m > 8 else [1]
        for j in bad:
            samples[j] = [0, 3, 5, 7]
        p1[6], p2[6] = p1[8], p2[8]   # (a tie that no sample above holds twice)
        samples[samples == 6] = 4
        for j in range(m):   # keep the other samples distinct after the substitution, and free of the pair (3, 7)
            if j not in bad and (len(set(samples[j])) < 4 or {3, 7} <= set(samples[j])):
                samples[j] = [0, 1, 2, 5]
    a, Ha = pkg.orsa_h_test_score(p1, p2, W, H, samples, on_device=True, wg_keys=wg_keys)
    b, Hb = pkg.orsa_h_test_score(p1, p2, W, H, samples, on_device=False)
    assert np.array_equal(Ha.view(np.uint32), Hb.view(np.uint32))
    assert np.array_equal(a, b)
    assert sorted(np.nonzero(b[:, 3])[0]) == sorted(bad)
    assert np.all(b[b[:, 3] == 0, 1] >= 4) and np.all(b[:, 1] < n)


@pytest.mark.gpu
def test_kernel_clamps_exact_zero_errors():
    """the exactly solvable sample of the CPU test: ten zero errors, -inf without the clamp"""
    p1, _ = cpu._dyadic_points()
    p1[3:7] = [[0, 0], [1, 0], [0, 1], [1, 1]]
    p2 = p1.copy()
    p2[10:] = p2[10:] - np.float32(0.5)
    s = np.array([[3, 4, 5, 6], [0, 4, 5, 6]], np.int32)
    a, Ha = pkg.orsa_h_test_score(p1, p2, W, H, s, on_device=True, wg_keys=64)
    b, Hb = pkg.orsa_h_test_score(p1, p2, W, H, s, on_device=False)
    assert np.array_equal(a, b) and np.array_equal(Ha.view(np.uint32), Hb.view(np.uint32))
    assert a[0, 1] == 9 and np.isfinite(a[0, 0:1].view(np.float32)[0])


def _same(a, b):
    for k in ("mask", "H", "index", "refit"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n"] == b["n"] and a["stats"][:2] == b["stats"][:2] and a["thr_px"] == b["thr_px"]
    assert np.array_equal(cpu.bits(a["log_nfa"]), cpu.bits(b["log_nfa"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ref.SCENES))
def test_device_equals_host_path(name):
    u6, _, _ = cpu.scene_points(name)
    laf = ref.laf_from_u6(u6)
    seed = ref.SCENES[name][4]
    b = pkg.orsa_h(u6, laf, W, H, seed_time=seed, on_device=False)
    a = pkg.orsa_h(u6, laf, W, H, seed_time=seed)
    _same(a, b)
    assert a["stats"] == b["stats"]   # the same blocking: the same rewinds
    assert (a["log_nfa"] < -2) == (name in ref.SIGNIFICANT)
    if name in ref.SIGNIFICANT:
        assert a["n"] >= 8 and np.all(a["H"] != -1)
    p = pkg.orsa_last_profile()
    print(name, "profile of the device call (ms)", p)


@pytest.mark.gpu
def test_independent_of_batch_and_packing():
    name = "n200_r02"
    u6, _, _ = cpu.scene_points(name)
    want = cpu.host_run(name)
    for batch, wg in ((1, 256), (64, 32768), (5000, 1024)):
        r = pkg.orsa_h(u6, None, W, H, seed_time=ref.SCENES[name][4], batch=batch, wg_keys=wg)
        _same(r, want)


@pytest.mark.gpu
def test_verify_tentatives_wh_equals_orsa_h():
    name = "n200_r05"
    u6, _, _ = cpu.scene_points(name)
    u6 = np.concatenate([u6, u6[:30] + [0.25, 0.25, 0, 0.25, 0.25, 0]])   # 30 near-duplicates for DuplicateFiltering to drop
    laf = ref.laf_from_u6(u6)
    par = pkg.PairParams.default()
    par.ransac = pkg.RansacParams.default(useF=3)
    tent = np.zeros(len(u6), pkg.TENT_DTYPE)
    tent["q"] = np.arange(len(u6))
    td, ud, ld = pkg.duplicate_filter(tent, u6, par.dup_dist, par.dup_mode, laf)
    assert 8 < len(ud) < len(u6)
    tv, uv, lv, nu, Hm, stats = pkg.verify_tentatives(tent, u6, laf, par, seed_time=5, wh=(W, H))
    r = pkg.orsa_h(ud, ld, W, H, params=par.ransac, seed_time=5, on_device=False)
    assert nu == len(ud) and r["log_nfa"] < -2 and r["n"] >= 8
    assert np.array_equal(tv["q"], td["q"][r["mask"]]) and np.array_equal(uv, ud[r["mask"]]) and np.array_equal(Hm, r["H"])
    assert stats == r["stats"]
    with pytest.raises(pkg.ModsError, match="image size"):
        pkg.verify_tentatives(tent, u6, laf, par, seed_time=5)


def _grey(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.float32)


def _graf():
    """graf 1 / 6, the oracle's unique tentatives of one identity-view step, and the host-path ORSA-H on them"""
    if "graf" not in _cache:
        import orc
        import pipeline_oracle as po
        a, b = _grey(G1), _grey(G6)
        assert a.shape == b.shape
        (ra, _), (rb, _) = po.pmap(orc.detect_describe, (a, b))
        tc = po.match_fginn_par(ra, rb, 0.8)
        un = orc.duplicate_filter(tc, ra, rb, 2.0, 1)
        u6, laf = po.u6_of(ra, rb, un), po.laf_of(ra, rb, un)
        h, w = a.shape
        want = pkg.orsa_h(u6, laf, w, h, seed_time=77, on_device=False)
        _cache["graf"] = (a, b, len(tc), u6, laf, want)
    return _cache["graf"]


def _check_graf(res, m, n_tc, u6, want):
    """As test_gpu_orsa.py::test_match_pair_dev_graf_orsa treats F: the entry point's verified list, model and counts equal the
    host-path verifier's on the oracle's unique tentatives.  The model is significant, and it is graf's homography: within the
    bounds test_cpu_oracle.py sets on the Oxford H1to6 (which that file holds to two or three digits, so no pixel bound is taken
    from it: measured under that rounded matrix, the 21 verified matches lie at a median of 2.3 px, 15 of them within 3 px, the
    farthest at 6.2 px, while the model differs from it by 0.08 in that file's relative measure, bound 0.3); every verified match
    lies within thr_px (3.34) of the model."""
    assert res.n_tentatives == n_tc and res.n_unique == len(u6) > 50
    assert want["log_nfa"] < -2 and res.n_inliers == want["n"] == len(m) >= 8
    assert np.array_equal(m, u6[want["mask"]][:, [0, 1, 3, 4]])
    assert np.array_equal(np.array(res.H), want["H"])
    assert [res.ransac_samples, res.ransac_lo, res.ransac_rejects] == want["stats"]
    Hm = np.array(res.H).reshape(3, 3)
    Hn = Hm / Hm[2, 2]
    rel = np.max(np.abs(Hn - HGT) / np.array([[1, 1, 100], [1, 1, 100], [1e-3, 1e-3, 1]]))
    d = np.linalg.norm(ref.apply_h(Hm, m[:, 0:2]) - m[:, 2:4], axis=1)
    dg = np.linalg.norm(ref.apply_h(HGT, m[:, 0:2]) - m[:, 2:4], axis=1)
    print("graf: log_nfa", want["log_nfa"], "verified", len(m), "of", len(u6), "thr_px", want["thr_px"], "largest distance under the model",
          d.max(), "under the rounded H1to6: median", np.median(dg), "max", dg.max(), "relative model difference", rel)
    assert rel < 0.3
    assert d.max() <= want["thr_px"] * (1 + 1e-6)


@pytest.mark.gpu
def test_match_pair_dev_graf_orsa_h():
    import torch
    a, b, n_tc, u6, laf, want = _graf()
    h, w = a.shape
    ctx = pkg.Context(0, w, h, 2)
    t = torch.from_numpy(np.stack([a, b])).cuda(0)
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    par.ransac = pkg.RansacParams.default(useF=3)
    pkg.ransac_pin_seed(77)
    res, m = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, params=par, max_matches=100000)
    ctx.close()
    _check_graf(res, m, n_tc, u6, want)


@pytest.mark.gpu
def test_ladder_graf_orsa_h():
    import torch
    a, b, n_tc, u6, laf, want = _graf()
    h, w = a.shape
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    rep1, rep2 = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    par.ransac = pkg.RansacParams.default(useF=3)
    pkg.ransac_pin_seed(77)
    res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, [pkg.LadderStep.make((1,), 360.0)], rep1, rep2, params=par, max_matches=100000)
    rep1.close(); rep2.close(); ctx.close()
    _check_graf(res, m, n_tc, u6, want)


def _cli(tmp_path, ver_type, a_contrario):
    text = open(os.path.join(CFG, "classic.ini")).read()
    assert "[RANSAC]" in text and "aContrario" not in text
    cfg = tmp_path / ("ac%d.ini" % a_contrario)
    cfg.write_text(text.replace("[RANSAC]", "[RANSAC]\naContrario = %d" % a_contrario, 1))
    args = [MODS, G1, G6, "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", ver_type, "H.txt", str(cfg),
            os.path.join(CFG, "iters_one_view.ini")]
    return subprocess.run(args, cwd=tmp_path, env=dict(os.environ, MODS_RANSAC_SEED="4242"), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=600)


def _library(use_f):
    import torch
    import orc
    from PIL import Image
    a, b = (orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB"))) for fn in (G1, G6))
    h, w = a.shape
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    rep1, rep2 = pkg.ImgRep(ctx, 1 << 20), pkg.ImgRep(ctx, 1 << 20)
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    par = pkg.PairParams.default()
    par.ransac.useF = use_f
    pkg.ransac_pin_seed(4242)
    res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, [pkg.LadderStep.make((1,), 360.0)], rep1, rep2, par, max_matches=1 << 20)
    pkg.ransac_pin_seed(-1)
    rep1.close(); rep2.close(); ctx.close()
    return res, m


@pytest.mark.gpu
@pytest.mark.parametrize("ver_type,use_f,label", [("0", 3, "ORSA(homography)"), ("2", 2, "ORSA(epipolar)")])
def test_cli_a_contrario(tmp_path, ver_type, use_f, label):
    """[RANSAC] aContrario = 1: ver_type 0 runs ORSA-H, ver_type 2 ORSA F; the files equal the library's run with that useF"""
    p = _cli(tmp_path, ver_type, 1)
    err = p.stderr.decode()
    assert p.returncode == 0, err
    res, m = _library(use_f)
    got = np.loadtxt(tmp_path / "m.txt").reshape(-1, 4)
    assert len(got) == res.n_inliers >= 8
    assert np.allclose(got, m, rtol=1e-5, atol=1e-3)                 # text output carries 6 significant digits
    Hm = np.loadtxt(tmp_path / "H.txt")
    assert Hm.shape == (3, 3) and np.allclose(Hm, np.array(res.H).reshape(3, 3), rtol=1e-4, atol=1e-6)
    assert label + " verification is used" in err
    log = (tmp_path / "log.txt").read_text().split()
    assert len(log) == 7 and int(log[1]) == res.n_inliers
    if use_f == 3:   # a homography row of the log (region counts), and the data-driven threshold under verbose
        assert [int(log[4]), int(log[5])] == [res.n_unoriented[0], res.n_unoriented[1]]
        assert "inlier threshold = " in err
    else:
        assert [int(log[4]), int(log[5])] == [res.n_described[0], res.n_described[1]]


@pytest.mark.gpu
def test_cli_rejects_bad_a_contrario_and_ver_type_3(tmp_path):
    p = _cli(tmp_path, "0", 2)
    assert p.returncode != 0 and "aContrario" in p.stderr.decode()
    p = _cli(tmp_path, "3", 1)
    assert p.returncode != 0 and "wrong correspondence verification type" in p.stderr.decode()
