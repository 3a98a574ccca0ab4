"""-m gpu: AffNet, OriNet and HardNet in-process (csrc/nets.hip, pkg.Net) - against the reference's own outputs for its
weights (tests/golden/nets.npz), against the daemon's PyTorch model on the CPU, and as built-in networks of the describe
stage, where everything around the networks has to be exactly what the callback path computes."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import orc
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nets.npz")
FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_int))
MR = 3.0 * np.sqrt(3.0)
KINDS = ("affnet", "orinet", "hardnet")


def _zd():
    sys.path.insert(0, os.path.join(ROOT, "mods-light-zmq_amd"))
    import zmq_daemon
    return zmq_daemon


def _golden_state(kind):
    g = np.load(GOLDEN)
    return {k[len(kind) + 1:]: g[k] for k in g.files if k.startswith(kind + ".")}


def _module_of(fn, seen=None):
    """the torch module a model function of zmq_daemon.build_model closes over"""
    import torch
    seen = seen if seen is not None else set()
    for c in fn.__closure__ or ():
        v = c.cell_contents
        if isinstance(v, torch.nn.Module):
            return v
        if callable(v) and getattr(v, "__closure__", None) and id(v) not in seen:
            seen.add(id(v))
            m = _module_of(v, seen)
            if m is not None:
                return m
    return None


def hardnet_state(seed, random_stats=True):
    """HardNet weights of the daemon's seeded model; the BatchNorm running statistics replaced by random ones (variances in
    [0.5, 2]) so that they take part in the result."""
    net = _module_of(_zd().build_model("hardnet", None, seed, "cpu"))
    st = {k: v.detach().numpy().copy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    if random_stats:
        rng = np.random.default_rng(seed + 1000)
        for k in st:
            if k.endswith("running_mean"):
                st[k] = rng.normal(0, 0.2, st[k].shape).astype(np.float32)
            elif k.endswith("running_var"):
                st[k] = rng.uniform(0.5, 2.0, st[k].shape).astype(np.float32)
    return st


def _state(kind):
    return hardnet_state(5) if kind == "hardnet" else _golden_state(kind)


def _patches(n, seed):
    """n patches in 0..255: the golden ones, smooth random ones, noise, one constant patch"""
    rng = np.random.default_rng(seed)
    out = [np.load(GOLDEN)["patches"].astype(np.float32)]
    m = len(out[0])
    n_smooth = (n - m - 1) // 2
    yy, xx = np.mgrid[0:32, 0:32].astype(np.float32)
    smooth = []
    for _ in range(n_smooth):
        a = rng.uniform(-4, 4, 6)
        f = a[0] * xx + a[1] * yy + 20 * np.sin(a[2] * xx / 6 + a[3]) * np.cos(a[4] * yy / 6 + a[5])
        smooth.append(np.clip(128 + f * rng.uniform(0.2, 2.0), 0, 255))
    out.append(np.array(smooth, np.float32).reshape(-1, 32, 32))
    out.append(rng.uniform(0, 255, (n - m - 1 - n_smooth, 32, 32)).astype(np.float32))
    out.append(np.full((1, 32, 32), 77.0, np.float32))
    p = np.concatenate(out, 0)
    assert p.shape == (n, 32, 32)
    return p


@pytest.fixture(scope="module")
def nets(pkg):
    d = {k: pkg.Net(k, _state(k)) for k in KINDS}
    yield d
    for n in d.values():
        n.close()


# ---- 2. reference weights ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["affnet", "orinet"])
def test_reference_weights_reference_outputs(pkg, nets, kind):
    g = np.load(GOLDEN)
    got = nets[kind].forward(g["patches"], quantise=False)
    want = g[kind + "_out"]
    assert got.shape == want.shape and nets[kind].dim == want.shape[1]
    # the yardstick: how far a plain float32 evaluation on the CPU (tests/nets_ref.py) is from the same outputs
    import nets_ref
    e_ref = np.max(np.abs(nets_ref.forward32(kind, _golden_state(kind), g["patches"]) - want))
    err = np.max(np.abs(got - want))
    print("%s: largest error against the reference's outputs %.3g, e_ref %.3g, ratio %.2f" % (kind, err, e_ref, err / e_ref))
    assert 0 < e_ref < 1e-5
    assert err <= 4 * e_ref


# ---- 3. HardNet against the daemon's model on the CPU ---------------------------------------------------------
def test_hardnet_equals_daemon_model(pkg, nets):
    p = _patches(512, 1)
    want = _zd().build_model("hardnet", hardnet_state(5), 0, "cpu")(p.reshape(-1, 1, 32, 32))
    got = nets["hardnet"].forward(p, quantise=False)
    assert got.shape == want.shape == (512, 128) and np.array_equal(got, np.floor(got)) and got.min() >= 0 and got.max() <= 255
    assert got.std() > 5
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("hardnet: %d of %d bytes differ (%.3g), largest difference %d" % ((diff > 0).sum(), diff.size, (diff > 0).mean(), diff.max()))
    assert diff.max() <= 1
    assert (diff > 0).mean() <= 1e-3


# ---- 4. a patch's output depends on nothing else ----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_output_is_a_function_of_the_patch_alone(pkg, nets, kind):
    import torch
    net = nets[kind]
    chunk = pkg.net_chunk()
    p = np.tile(_patches(512, 2), (10, 1, 1))[:5000].copy()
    rng = np.random.default_rng(3)
    p[512:] += rng.uniform(-3, 3, p[512:].shape).astype(np.float32)      # (no two of the 5000 alike)
    full = net.forward(p, quantise=True)
    assert full.shape == (5000, net.dim) and np.all(np.isfinite(full))
    for n in (1, 63, 64, 65, chunk + 1):
        assert np.array_equal(net.forward(p[:n], quantise=True), full[:n]), n
    # a tail that starts in the middle of a chunk
    assert np.array_equal(net.forward(p[chunk + 7:chunk + 300], quantise=True), full[chunk + 7:chunk + 300])
    perm = rng.permutation(len(p))
    assert np.array_equal(net.forward(p[perm], quantise=True), full[perm])
    # host entry point against the device entry point
    t = torch.from_numpy(p).cuda()
    out = torch.zeros((len(p), net.dim), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    net.forward_dev(torch.cuda.current_stream().cuda_stream, t.data_ptr(), len(p), out.data_ptr(), quantise=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), full)


def _set_builtin(ctx, nets, quantise, descriptor=True):
    ctx.set_builtin_shape(nets["affnet"], MR, quantise)
    ctx.set_builtin_orientation(nets["orinet"], MR, quantise)
    if descriptor:
        ctx.set_builtin_descriptor(nets["hardnet"], MR, quantise)


def _clear(ctx):
    ctx.set_builtin_shape(None); ctx.set_builtin_orientation(None); ctx.set_builtin_descriptor(None)
    ctx.set_external_shape(None, None); ctx.set_external_orientation(None, None); ctx.set_external_descriptor(None, None)


def test_two_threads_share_the_networks(pkg, nets):
    """one mods_net under two contexts and two threads at once: the results of a single thread"""
    w, h = 480, 360
    img = synth.texture(w, h, seed=3)
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    ctxs = [pkg.Context(0, w, h, 1, nonblocking=True) for _ in range(2)]
    keys = ctxs[0].detect_hessian_affine(img, det)
    for c in ctxs:
        _set_builtin(c, nets, True)
    want = ctxs[0].orient_describe(img, keys)
    p = _patches(512, 4)
    want_f = {k: nets[k].forward(p) for k in KINDS}
    got, errs = [[], []], []

    def work(i):
        try:
            for _ in range(3):
                got[i].append(ctxs[i].orient_describe(img, keys))
                got[i].append({k: nets[k].forward(p) for k in KINDS})
        except Exception as e:           # noqa: BLE001 - reported below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        for r in got[i]:
            if isinstance(r, dict):
                assert all(np.array_equal(r[k], want_f[k]) for k in KINDS)
            else:
                assert len(r) == len(want) > 100 and r.tobytes() == want.tobytes()
    for c in ctxs:
        c.close()


# ---- 5. quantisation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_quantisation_is_the_wire_rounding(pkg, nets, kind):
    p = _patches(200, 5)
    p[:50] = np.floor(p[:50]) + 0.5                        # ties: half to even
    p[50:60] -= 200.0                                      # negatives
    p[60:70] += 200.0                                      # beyond 255
    p[70, 0, :8] = [0.5, 1.5, 2.5, 254.5, 255.5, -0.5, 255.49, 300.0]
    q = np.clip(np.rint(p), 0, 255).astype(np.float32)
    assert np.array_equal(nets[kind].forward(p, quantise=True), nets[kind].forward(q, quantise=False))
    assert not np.array_equal(nets[kind].forward(p, quantise=False), nets[kind].forward(q, quantise=False))


# ---- 6. plumbing ----------------------------------------------------------------------------------------------
def _hook(net, quantise):
    def fn(user, patches, n, ps, out, cap, dim_out):
        a = np.ctypeslib.as_array(patches, shape=(n, ps, ps)).copy()
        r = net.forward(a, quantise=quantise)
        np.ctypeslib.as_array(out, shape=(n * net.dim,))[:] = r.reshape(-1)
        dim_out[0] = net.dim
        return 0
    return FN(fn)


def _set_hooks(ctx, hooks, descriptor=True):
    ctx.set_external_shape(C.cast(hooks["affnet"], C.c_void_p).value, None, MR, 32)
    ctx.set_external_orientation(C.cast(hooks["orinet"], C.c_void_p).value, None, MR, 32)
    if descriptor:
        ctx.set_external_descriptor(C.cast(hooks["hardnet"], C.c_void_p).value, None, MR, 32)


def _same_regions(a, b):
    assert len(a) == len(b)
    for f in ("x", "y", "s", "a11", "a12", "a21", "a22", "response", "sub_type", "id", "parent"):
        assert np.array_equal(a[f], b[f]), f
    assert np.array_equal(a["desc"], b["desc"])


@pytest.mark.parametrize("quantise", [True, False])
@pytest.mark.parametrize("w,h,seed", [(480, 360, 3), (640, 400, 9)])
def test_builtin_networks_equal_callbacks_and_oracle(pkg, nets, w, h, seed, quantise):
    img = synth.texture(w, h, seed=seed)
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    ctx = pkg.Context(0, w, h, 1)
    keys = ctx.detect_hessian_affine(img, det)
    assert len(keys) > 200
    hooks = {k: _hook(nets[k], quantise) for k in KINDS}
    # shape + orientation, RootSIFT descriptors: built-in = callbacks = the oracle chain driven by the same networks
    _set_builtin(ctx, nets, quantise, descriptor=False)
    got = ctx.orient_describe(img, keys)
    _clear(ctx)
    _set_hooks(ctx, hooks, descriptor=False)
    via_hooks = ctx.orient_describe(img, keys)
    _clear(ctx)
    _same_regions(got, via_hooks)
    regs = orc.regions_from_keys(keys)
    p1 = orc.extract_patches_column(img, regs, MR, 32)
    regs = orc.affnet_apply(regs, nets["affnet"].forward(p1, quantise=quantise), w, h, MR)
    assert 0 < len(regs) <= len(keys)
    regs = orc.filter_centres_inside(regs, w, h)
    p2 = orc.extract_patches_column(img, regs, MR, 32)
    regs = orc.orinet_apply(regs, nets["orinet"].forward(p2, quantise=quantise))
    regs = orc.filter_touch_boundary(regs, w, h)
    want = orc.describe_rootsift(img, regs)
    assert len(got) == len(want) > 100
    for f in ("x", "y", "s", "a11", "a12", "a21", "a22", "response"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["desc"], want["desc"])
    # all three slots: built-in against callbacks
    _set_builtin(ctx, nets, quantise)
    got3 = ctx.orient_describe(img, keys)
    _clear(ctx)
    _set_hooks(ctx, hooks)
    hooks3 = ctx.orient_describe(img, keys)
    _clear(ctx)
    _same_regions(got3, hooks3)
    for f in ("x", "y", "a11", "a12", "a21", "a22"):
        assert np.array_equal(got3[f], got[f]), f
    assert got3["desc"].std() > 5 and not np.array_equal(got3["desc"], got["desc"])
    # switching the slots off restores the classic path
    plain = ctx.orient_describe(img, keys)
    assert not np.array_equal(plain["a11"][:50], got["a11"][:50])
    ctx.close()


def test_slots_hold_a_callback_or_a_network(pkg, nets):
    w, h = 320, 240
    img = synth.texture(w, h, seed=4)
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    ctx = pkg.Context(0, w, h, 1)
    keys = ctx.detect_hessian_affine(img, det)
    calls = []

    def fn(user, patches, n, ps, out, cap, dim_out):
        calls.append(n)
        r = nets["orinet"].forward(np.ctypeslib.as_array(patches, shape=(n, ps, ps)).copy(), quantise=True)
        np.ctypeslib.as_array(out, shape=(n * 2,))[:] = r.reshape(-1)
        dim_out[0] = 2
        return 0
    cb = FN(fn)
    ctx.set_external_orientation(C.cast(cb, C.c_void_p).value, None, MR, 32)
    ctx.set_builtin_orientation(nets["orinet"], MR, True)          # clears the callback
    a = ctx.orient_describe(img, keys)
    assert not calls
    ctx.set_external_orientation(C.cast(cb, C.c_void_p).value, None, MR, 32)   # clears the network
    b = ctx.orient_describe(img, keys)
    assert calls and a.tobytes() == b.tobytes()
    with pytest.raises(pkg.ModsError, match="affnet"):
        ctx.set_builtin_shape(nets["orinet"])
    lib = pkg.lib()
    assert lib.mods_ctx_set_builtin_descriptor(ctx.h, nets["affnet"].h, C.c_double(MR), 1) == -2
    assert b"HardNet" in lib.mods_last_error()
    ctx.close()


def test_tilted_view_builtin_equals_callbacks(pkg, nets):
    import torch
    w, h = 480, 360
    img = synth.texture(w, h, seed=3)
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    t = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    hooks = {k: _hook(nets[k], True) for k in KINDS}
    _set_builtin(ctx, nets, True)
    _, nd, nr = ctx.detect_describe_view_dev(t.data_ptr(), w, h, 2.0, 60.0, det=det)
    got = ctx.regions_fetch(0)
    _clear(ctx)
    _set_hooks(ctx, hooks)
    _, nd2, nr2 = ctx.detect_describe_view_dev(t.data_ptr(), w, h, 2.0, 60.0, det=det)
    want = ctx.regions_fetch(0)
    _clear(ctx)
    assert (nd, nr) == (nd2, nr2) and nr == len(got) > 50
    _same_regions(got, want)
    ctx.close()


def test_ladder_builtin_equals_callbacks(pkg, nets):
    """A two-step HessianAffine ladder: the callbacks force one view worker, the built-in networks keep the default number (and
    pair the two images of a view), so equal banks also mean that the workers fill the banks in job order."""
    import torch
    w, h = 480, 360
    a, b, _ = synth.pair(w, h, seed=7)
    d = pkg.view_ctx_dims(w, h)
    steps = [pkg.LadderStep.make((1,), 360.0), pkg.LadderStep.make((1, 2, 4), 120.0)]
    par = pkg.PairParams.default()
    par.det.doBaumberg = 0
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    hooks = {k: _hook(nets[k], True) for k in KINDS}
    out = []
    for mode in ("builtin", "hooks"):
        ctx = pkg.Context(0, d[0], d[1], 2)
        rep1, rep2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
        if mode == "builtin":
            _set_builtin(ctx, nets, True)
        else:
            _set_hooks(ctx, hooks)
        pkg.ransac_pin_seed(4242)
        res, m = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, rep1, rep2, par, min_matches=10 ** 6, max_matches=1 << 16)
        pkg.ransac_pin_seed(-1)
        out.append((res, m, rep1.fetch(), rep2.fetch()))
        _clear(ctx)
        rep1.close(); rep2.close(); ctx.close()
    (r1, m1, a1, b1), (r2, m2, a2, b2) = out
    assert r1.steps_done == r2.steps_done == 2 and r1.n_views == r2.n_views > 4
    assert len(a1) > 300 and len(b1) > 300
    _same_regions(a1, a2)
    _same_regions(b1, b2)
    assert (r1.n_tentatives, r1.n_unique, r1.n_inliers) == (r2.n_tentatives, r2.n_unique, r2.n_inliers)
    assert list(r1.H) == list(r2.H) and np.array_equal(m1, m2)


# ---- 7. command line --------------------------------------------------------------------------------------------
def _weights_file(path, kinds=KINDS):
    """AffNet / OriNet of the reference and the daemon's HardNet of seed 5 as it is built (what the three-daemon test serves with
    --seed 5).  With the random running statistics of the tests above this untrained network saturates: 37 of the 3358 regions of
    graf1 share their 128 bytes with a neighbour, and a tie is not a match of a point with itself."""
    arrays = {}
    for k in kinds:
        st = hardnet_state(5, random_stats=False) if k == "hardnet" else _golden_state(k)
        arrays.update({k + "." + n: v for n, v in st.items()})
    np.savez(path, **arrays)            # stored members: what cli/npz_io.hpp reads
    return str(path)


def _deep_config(tmp_path, weights):
    import re
    cfg = open(os.path.join(ROOT, "tests", "configs", "classic.ini")).read()
    assert "doBaumberg=1" in cfg.replace(" ", "")
    cfg = re.sub(r"doBaumberg\s*=\s*1", "doBaumberg=0", cfg)
    # (a key given twice reads as both values joined: the section's own useZMQ is switched, not repeated)
    assert len(re.findall(r"useZMQ\s*=\s*0", cfg)) == 1
    cfg = re.sub(r"useZMQ\s*=\s*0", "useZMQ=1", cfg)
    cfg += ("\n[AffineAdaptation]\nuseZMQ=1\n[AffNet]\nweights=%s\npatchSize=32\nmrSize=5.1962\n" % weights
            + "[OriNet]\nweights=%s\npatchSize=32\nmrSize=5.1962\n" % weights
            + "[zmqDescriptor]\nweights=%s\npatchSize=32\nmrSize=5.1962\n" % weights)
    (tmp_path / "deep.ini").write_text(cfg)
    return str(tmp_path / "deep.ini")


def _mods(tmp_path, config, k1="k1.txt", k2="k2.txt"):
    from test_gpu_cli import MODS, G1, CFG
    args = [MODS, G1, G1, "o1.png", "o2.png", k1, k2, "m.txt", "log.txt", "0", "0", "H.txt", config, os.path.join(CFG, "iters_zmq.ini")]
    return subprocess.run(args, cwd=tmp_path, env=dict(os.environ, MODS_RANSAC_SEED="4242"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=600)


def test_cli_deep_configuration_in_process(pkg, nets, tmp_path):
    """The deep configuration of test_cli_deep_configuration_three_daemons with weights= in the three sections: no daemon, no
    port; and the keypoints the command line writes are those of the Python path."""
    from test_gpu_cli import G1, _grey
    cfg = _deep_config(tmp_path, _weights_file(tmp_path / "nets_w.npz"))
    p = _mods(tmp_path, cfg, "k1.npz", "k2.npz")
    assert p.returncode == 0, p.stderr.decode()
    err = p.stderr.decode()
    assert "AffNet in-process" in err and "OriNet in-process" in err and "HardNet in-process" in err and "daemon" not in err
    got = np.loadtxt(tmp_path / "m.txt").reshape(-1, 4)
    print("command line: %d matches, %d of them not of a point with itself" % (len(got), int(np.sum(np.abs(got[:, :2] - got[:, 2:]).max(1) > 1e-3))))
    assert len(got) > 300 and np.allclose(got[:, :2], got[:, 2:], atol=1e-3)
    H = np.loadtxt(tmp_path / "H.txt")
    assert np.allclose(H / H[2, 2], np.eye(3), atol=1e-3)
    # the same image through the library: detect (doBaumberg = 0), then the three built-in networks, quantisation on
    img = _grey(G1)
    h, w = img.shape
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    ctx = pkg.Context(0, w, h, 1)
    keys = ctx.detect_hessian_affine(img, det)
    desc = pkg.DescribeParams.default()
    desc.ori_mrSize = desc.desc_mrSize = 5.1962
    hard = pkg.Net("hardnet", hardnet_state(5, random_stats=False))
    ctx.set_builtin_shape(nets["affnet"], 5.1962, True)
    ctx.set_builtin_orientation(nets["orinet"], 5.1962, True)
    ctx.set_builtin_descriptor(hard, 5.1962, True)
    want = ctx.orient_describe(img, keys, desc)
    _clear(ctx)
    ctx.close()
    hard.close()
    k = np.load(tmp_path / "k1.npz")
    assert len(k["xy"]) == len(want) > 300
    assert np.array_equal(k["xy"], np.stack([want["x"], want["y"]], 1))
    assert np.array_equal(k["A"].reshape(-1, 4), np.stack([want["a11"], want["a12"], want["a21"], want["a22"]], 1))
    assert np.array_equal(k["scales"].reshape(-1), want["s"])
    assert np.array_equal(k["descs"], want["desc"])


def test_cli_reports_missing_arrays(pkg, tmp_path):
    cfg = _deep_config(tmp_path, _weights_file(tmp_path / "no_ori.npz", kinds=("affnet", "hardnet")))
    p = _mods(tmp_path, cfg)
    assert p.returncode != 0
    assert "orinet." in p.stderr.decode() and "no_ori.npz" in p.stderr.decode()
