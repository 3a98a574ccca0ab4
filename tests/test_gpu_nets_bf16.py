"""-m gpu: the bf16 matrix-core mode of the built-in networks (csrc/nets_mfma.hip, pkg.Net(..., precision="bf16")) against its
contract (include/mods_hip.h) as tests/nets_bf16_ref.py evaluates it on the CPU.

  1  stage 0 = the fp32 net's, stage 1 = bf16(the fp32 net's), the small heads on bf16 values = the fp32 net's: to the bit
  2  integer weights, integer activations (one-hot impulses and dense): every product and sum is exact, so is the comparison
  3  dense stages 2..6 against float64 inside min(8 e_cpu, (K + 3) 2^-23 S), as an interval of bf16 values; HardNet's head by bytes
  4  whole networks against forward_bf16 in float64, e_cpu from forward_bf16 in float32
  5  a row does not depend on the rest of the call   6  the guard of the stage hook   7  through the library and the command line
  8  mods_net_create_ex(MODS_NET_FP32) = mods_net_create

e_cpu of 3 is the largest deviation of the reference's float32 evaluation from its float64 one on the same (rounded) operands,
before the output is rounded to bf16.  e_gpu there is the kernel's distance from the float64 value that the last rounding to bf16
(half a place of the reference's own rounded value) does not explain.

Observed on an MI355X (-s prints them): 3, e_gpu / e_cpu per stage 2..6, the largest over n: AffNet 0.39 0.09 0.15 0.05 0.09
(trained) and 0.61 0.51 0.12 0.00 0.28 (synthetic), OriNet 0.00 0.59 0.15 0.48 0.28 and 0.04 0.00 0.00 0.24 0.00, HardNet
0.05 0.07 0.25 1.30 0.58 (seed 5) and 0.55 0.18 0.06 0.29 1.15; at most 6 of 163 840 elements leave the reference's own bf16
value, by one place.  HardNet's dense head: no wrong byte, exempt share at most 4.6e-4.  4, e_gpu / e_cpu: AffNet 1.00 1.00 1.00
0.90, OriNet 1.02 1.00 1.31 0.36 (trained / synthetic, quantise off / on); HardNet delta 0.22 / 0.10 bytes (seed 5) and 1.61 / 1.07
(synthetic), 1 to 20 of 1152 bytes off floor(q64), none by more than 1.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import nets_bf16_ref as br
import nets_ref
import synth
from test_gpu_nets import GOLDEN, KINDS, MR, _clear, _deep_config, _hook, _mods, _same_regions, _set_hooks, _weights_file
from test_gpu_nets_stages import IDS, STATES, _impulse_input, _patch_set, _state

pytestmark = pytest.mark.gpu
PPW8 = 2                                  # patches of a workgroup at the 8 x 8 maps (stages 5 and 6), nets_mfma.hpp


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def nets(pkg):
    d = {}

    def get(kind, which, precision="bf16", state=None):
        key = (kind, which, precision)
        if key not in d:
            d[key] = pkg.Net(kind, state if state is not None else _state(kind, which), precision=precision)
        return d[key]
    yield get
    for n in d.values():
        n.close()


# ---- 1. what the mode leaves alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,which", STATES, ids=IDS)
def test_untouched_stages_equal_the_fp32_net(pkg, nets, kind, which):
    b, f = nets(kind, which), nets(kind, which, "fp32")
    assert (b.precision, f.precision) == ("bf16", "fp32")
    assert pkg.lib().mods_net_precision(b.h) == 1 and pkg.lib().mods_net_precision(f.h) == 0
    p = _patch_set()[3:20].reshape(17, 1024)
    for q in (False, True):
        x0, ok = b.stage(0, p, quantise=q)
        assert ok and np.array_equal(_bits(x0), _bits(f.stage(0, p, quantise=q)[0]))
    x1, ok = b.stage(1, x0)
    want = br.bf16(f.stage(1, x0)[0])
    assert ok and x1.shape == want.shape and np.array_equal(_bits(x1), _bits(want)) and 0.05 < np.mean(x1 > 0) < 0.95
    if kind != "hardnet":
        x = br.dense_input(kind, 7, 9)
        got, ok = b.stage(7, x)
        assert ok and np.array_equal(_bits(got), _bits(f.stage(7, x)[0])) and np.ptp(got, axis=0).min() > 0


# ---- 2. exact integer data -------------------------------------------------------------------------------------
def _integer_state(kind, seed):
    """Integer weights in -8..8, running_var = float32(1 - 1e-5) (1 / sqrt(var + 1e-5) = 1 to 2e-8: the fold rounds back to the
    integer), running_mean = -16 in the blocks (a folded bias of 16 that no single weight pulls below 0) and small integers in
    HardNet's head.  The small heads are not used."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, shape in nets_ref.tensor_shapes(kind):
        if name.endswith("weight"):
            st[name] = rng.integers(-8, 9, shape).astype(np.float32)
        elif name.endswith("running_var"):
            st[name] = np.full(shape, 1.0 - 1e-5, np.float32)
        elif name.endswith("running_mean"):
            st[name] = np.full(shape, -16.0, np.float32) if name != "features.20.running_mean" else rng.integers(-3, 4, shape).astype(np.float32)
        else:
            st[name] = np.zeros(shape, np.float32)
    return st


@pytest.mark.parametrize("block", range(1, 6))
@pytest.mark.parametrize("kind", ["affnet", "hardnet"])          # C = 16 (OriNet runs the same instantiations) and C = 32
def test_integer_convolutions_are_exact(pkg, nets, kind, block):
    st = _integer_state(kind, 21)
    net = nets(kind, "integer", state=st)
    s = block + 1
    w, b = br.folded(kind, st)[s]
    assert np.array_equal(w, st["features.%d.weight" % (3 * block)]) and np.array_equal(b, np.full(len(b), 16.0, np.float32))
    cin, cout, stride, h = nets_ref.blocks(kind)[block]
    ho = h // stride
    # impulses: one product per output element, so every (tap, input channel, output channel) shows as 16 + its weight
    x = _impulse_input(cin, h)
    n = len(x)
    pos = x.any(axis=(0, 1))
    ys, xs = np.nonzero(pos)
    assert n % PPW8 == 1 and x.any(axis=(0, 2, 3)).all()
    assert pos[0, 0] and pos[0, h - 1] and pos[h - 1, 0] and pos[h - 1, h - 1] and x[n - 1, cin - 1, h - 1, h - 1] == 1
    assert {(y % 2, c % 2) for y, c in zip(ys, xs)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for ci in range(cin):          # every input channel at every tap (a row and a column inside the map on either side) and at both parities
        yy, cc = np.nonzero(x[:, ci].any(axis=0))
        assert ((yy > 0) & (yy < h - 1) & (cc > 0) & (cc < h - 1)).any()
        if stride == 2:
            assert {(y % 2, c % 2) for y, c in zip(yy, cc)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if h == 32:
        # a workgroup holds the whole map; rows 7 | 8 and 15 | 16 are where the pixel quarters of two waves meet (stride 1: a wave
        # has 8 output rows) and, at stride 2, where their input rows do
        assert 7 in ys and 8 in ys and 15 in ys and 16 in ys
    got, ok = net.stage(s, x)
    want = br.stage_bf16(kind, st, s, x)
    assert ok and got.shape == want.shape == (n, cout, ho, ho)
    assert want.min() >= 8 and len(np.unique(want)) >= 15 and np.array_equal(want, np.rint(want))
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "impulses: %d of %d elements differ, the first at %s: %r for %r" % (len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    # dense small integers: sums of up to 9 cin products of at most 16, exact in fp32; only the last rounding to bf16 is not
    rng = np.random.default_rng(100 + block)
    for m in (1, PPW8 + 1):
        x = rng.integers(0, 3, (m, cin, h, h)).astype(np.float32)
        got, ok = net.stage(s, x)
        unrounded = br.stage_bf16(kind, st, s, x, rounded=False)
        want = br.bf16(unrounded)
        assert ok and np.array_equal(unrounded, np.rint(unrounded)) and 0.1 < np.mean(want > 0) < 0.9 and want.max() > 64
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "dense, n = %d: %d of %d elements differ, the first at %s: %r for %r" % (m, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_integer_head_one_hot_reaches_every_weight(pkg, nets):
    """HardNet's head on one-hot inputs: y = W[:, k] + bias, integers, exact; the bytes behind the L2 normalisation follow the
    rule of nets_ref.check_hardnet_bytes with the e_cpu of the tail alone"""
    st = _integer_state("hardnet", 22)
    net = nets("hardnet", "integer22", state=st)
    w, b = br.folded("hardnet", st)[7]
    assert np.array_equal(w, st["features.19.weight"]) and np.array_equal(b, -st["features.20.running_mean"])
    K, chunk = 8192, 512
    assert chunk <= pkg.net_chunk()
    x = np.zeros((chunk, K), np.float32)
    got = []
    for k0 in range(0, K, chunk):
        x[:] = 0
        x[np.arange(chunk), k0 + np.arange(chunk)] = 1.0
        out, ok = net.stage(7, x)
        assert ok
        got.append(out)
    got = np.concatenate(got)

    def tail(dt):
        y = w.reshape(128, K).T.astype(dt) + b.astype(dt)
        return y / np.sqrt((y * y).sum(1, keepdims=True) + dt(1e-10))
    d64 = tail(np.float64)
    e_cpu = float(np.max(np.abs(tail(np.float32) - d64)))
    wrong, exempt = nets_ref.check_hardnet_bytes(got, d64, e_cpu)
    print("hardnet bf16 head, one-hot: e_cpu %.3g, %d wrong bytes of %d, exempt share %.3g, bytes %g..%g" % (e_cpu, wrong, got.size, exempt, got.min(), got.max()))
    assert got.std() > 10 and wrong == 0 and exempt <= 0.01


# ---- 3. dense stages against float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,which", STATES, ids=IDS)
def test_dense_stages_against_float64(pkg, nets, kind, which):
    st, net = _state(kind, which), nets(kind, which)
    f = br.folded(kind, st)
    rst = br.rounded_state(kind, st)
    ratios = []
    for s in range(2, 7):
        K = 9 * nets_ref.in_shape(kind, s)[0]
        worst_ratio = 0.0
        for n in (1, 5) + ((PPW8 + 1,) if s >= 5 else ()):
            x = br.dense_input(kind, s, n)
            got, ok = net.stage(s, x)
            r64 = br.stage_bf16(kind, st, s, x, rounded=False, _folded=f)
            r32 = br.stage_bf16(kind, st, s, x, torch.float32, rounded=False, _folded=f)
            assert ok and got.shape == r64.shape == (n,) + nets_ref.out_shape(kind, s) and 0.05 < np.mean(got > 0) < 0.95
            e_cpu = float(np.max(np.abs(r32 - r64)))
            tol = np.minimum(8 * e_cpu, (K + 3) * 2.0 ** -23 * nets_ref.abs_terms(kind, rst, s, x))
            lo, hi = br.bf16(np.maximum(r64 - tol, 0)), br.bf16(r64 + tol)
            e_gpu = float(np.max(np.abs(got - br.bf16(r64))))          # (0 where the kernel lands on the reference's own rounding)
            raw = float(np.max(np.abs(got - r64)))                     # includes the final rounding: at most half a bf16 place more
            line = "%s-%s stage %d n=%d: e_cpu %.3g, |got - R64| %.3g, %d of %d elements off bf16(R64), the largest by %.3g" % (
                kind, which, s, n, e_cpu, raw, int(np.sum(got != br.bf16(r64))), got.size, e_gpu)
            print(line)
            assert 0 < e_cpu and np.array_equal(_bits(got), _bits(br.bf16(got)))
            out = (got < lo) | (got > hi)
            assert not out.any(), "%s: %d elements outside the interval" % (line, int(out.sum()))
            # e_gpu / e_cpu in the sense of the fp32 tests: distance to R64 that the final rounding does not explain
            half = np.abs(br.bf16(r64) - r64)
            worst_ratio = max(worst_ratio, float(np.max(np.maximum(np.abs(got - r64) - half, 0))) / e_cpu)
        ratios.append(worst_ratio)
    print("RATIOS bf16 %s-%s stages 2..6 e_gpu / e_cpu: %s" % (kind, which, " ".join("%.2f" % r for r in ratios)))


@pytest.mark.parametrize("n", br.HEAD_N)
def test_dense_hardnet_head(pkg, nets, n):
    st, x, d64, _, e_cpu = br.head_case(n)
    got, ok = nets("hardnet", "synthetic").stage(7, x)
    wrong, exempt = nets_ref.check_hardnet_bytes(got, d64, e_cpu)
    print("hardnet bf16 head n=%d: e_cpu %.3g, %d wrong bytes of %d, exempt share %.3g" % (n, e_cpu, wrong, got.size, exempt))
    assert ok and got.std() > 5 and wrong == 0 and exempt <= 0.01


# ---- 4. whole networks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("kind,which", STATES, ids=IDS)
def test_whole_network_against_float64(pkg, nets, kind, which, quantise):
    st = _state(kind, which)
    p = _patch_set()[7:16]
    assert len(p) == 9
    ref = br.forward_bf16(kind, st, p, quantise=quantise)
    e_cpu = float(np.max(np.abs(br.forward_bf16(kind, st, p, torch.float32, quantise=quantise) - ref)))
    got = nets(kind, which).forward(p, quantise=quantise)
    assert got.shape == ref.shape and e_cpu > 0
    if kind == "hardnet":
        delta = 210.0 * 8.0 * e_cpu
        q = nets_ref.hardnet_q(ref)
        lo, hi = np.floor(np.clip(q - delta, 0, 255)), np.floor(np.clip(q + delta, 0, 255))
        print("RATIOS bf16 whole %s-%s quantise %d: e_cpu %.3g, delta %.3g, %d of %d bytes off floor(q64), the largest by %g" % (
            kind, which, quantise, e_cpu, delta, int(np.sum(got != np.floor(np.clip(q, 0, 255)))), got.size, np.max(np.abs(got - np.floor(np.clip(q, 0, 255))))))
        assert got.std() > 5
        assert np.all((got >= lo) & (got <= hi))
        return
    e_gpu = float(np.max(np.abs(got - ref)))
    print("RATIOS bf16 whole %s-%s quantise %d: e_gpu %.3g e_cpu %.3g ratio %.2f" % (kind, which, quantise, e_gpu, e_cpu, e_gpu / e_cpu))
    assert e_gpu <= 8 * e_cpu


# ---- 5. independence -----------------------------------------------------------------------------------------------
def test_a_row_depends_on_its_patch_alone(pkg, nets):
    net = nets("hardnet", "synthetic")
    n = pkg.net_chunk() + 1
    rng = np.random.default_rng(5)
    p = np.tile(_patch_set(), (n // len(_patch_set()) + 1, 1, 1))[:n].copy()
    p[len(_patch_set()):] += rng.uniform(-3, 3, p[len(_patch_set()):].shape).astype(np.float32)
    full = net.forward(p)
    assert full.shape == (n, 128) and full.std() > 5
    alone = np.concatenate([net.forward(p[i:i + 1]) for i in range(n)])
    assert np.array_equal(alone, full)
    assert np.array_equal(net.forward(p[::-1])[::-1], full)


# ---- 6. the guard ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_is_written_behind_the_last_patch(pkg, nets, kind):
    net = nets(kind, "synthetic")
    rng = np.random.default_rng(6)
    for n in (1, pkg.net_chunk()):
        for s in range(8):
            x = rng.uniform(0, 2, (n,) + net.stage_shapes(s)[0]).astype(np.float32)
            out, ok = net.stage(s, x)
            assert ok, (n, s)
            assert np.all(np.isfinite(out[-1])) and out[-1].any()


# ---- 7. through the library and the command line ----------------------------------------------------------------
def test_builtin_bf16_networks_equal_callbacks(pkg, nets):
    """orient_describe with the three bf16 nets in the built-in slots = the callback path (the host-side arithmetic) fed with
    Net.forward of the same nets on the patches the describe stage extracts"""
    w, h = 320, 240
    img = synth.texture(w, h, seed=4)
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    ctx = pkg.Context(0, w, h, 1)
    keys = ctx.detect_hessian_affine(img, det)
    b = {k: nets(k, "seed5" if k == "hardnet" else "golden") for k in KINDS}
    f = {k: nets(k, "seed5" if k == "hardnet" else "golden", "fp32") for k in KINDS}
    out = {}
    for name, d in (("bf16", b), ("fp32", f)):
        ctx.set_builtin_shape(d["affnet"], MR, True)
        ctx.set_builtin_orientation(d["orinet"], MR, True)
        ctx.set_builtin_descriptor(d["hardnet"], MR, True)
        out[name] = ctx.orient_describe(img, keys)
        _clear(ctx)
    hooks = {k: _hook(b[k], True) for k in KINDS}
    _set_hooks(ctx, hooks)
    via_hooks = ctx.orient_describe(img, keys)
    patches = ctx.patches_fetch(0, 32)          # what the descriptor callback was handed
    _clear(ctx)
    ctx.close()
    assert len(out["bf16"]) > 50
    _same_regions(out["bf16"], via_hooks)
    # the descriptor bytes are HardNet's answer to the stored patches
    assert len(patches) == len(out["bf16"]) and np.array_equal(b["hardnet"].forward(patches, quantise=True), out["bf16"]["desc"].astype(np.float32))
    assert len(out["bf16"]) != len(out["fp32"]) or not np.array_equal(out["bf16"]["desc"], out["fp32"]["desc"])       # a mode of its own


def test_cli_deep_configuration_in_bf16(pkg, tmp_path):
    cfg = _deep_config(tmp_path, _weights_file(tmp_path / "nets_w.npz"))
    text = open(cfg).read()
    for sec in ("AffNet", "OriNet", "zmqDescriptor"):
        assert text.count("[%s]\nweights=" % sec) == 1
        text = text.replace("[%s]\nweights=" % sec, "[%s]\nprecision = bf16\nweights=" % sec)
    open(cfg, "w").write(text)
    p = _mods(tmp_path, cfg, "k1.npz", "k2.npz")
    err = p.stderr.decode()
    assert p.returncode == 0, err
    for name in ("AffNet", "OriNet", "HardNet"):
        assert name + " in-process (precision bf16)" in err, err
    got = np.loadtxt(tmp_path / "m.txt").reshape(-1, 4)
    assert len(got) > 300 and np.allclose(got[:, :2], got[:, 2:], atol=1e-3)
    assert len(np.load(tmp_path / "k1.npz")["xy"]) > 300


# ---- 8. the old entry point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_create_is_create_ex_fp32(pkg, nets, kind):
    st = _state(kind, "synthetic")
    lib = pkg.lib()
    tensors = pkg.net_tensors(kind, st)
    ptrs = (C.POINTER(C.c_float) * len(tensors))(*[t.ctypes.data_as(C.POINTER(C.c_float)) for t in tensors])
    sizes = (C.c_size_t * len(tensors))(*[t.size for t in tensors])
    h = C.c_void_p()
    assert lib.mods_net_create(0, pkg.NET_KINDS[kind], ptrs, sizes, len(tensors), C.byref(h)) == 0
    assert lib.mods_net_precision(h) == 0
    p = np.ascontiguousarray(_patch_set()[:21])
    old = np.zeros((len(p), pkg.NET_DIMS[kind]), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))         # noqa: E731
    assert lib.mods_net_forward(h, fp(p), len(p), 1, fp(old)) == 0
    lib.mods_net_destroy.restype = None
    lib.mods_net_destroy(h)
    new = nets(kind, "synthetic", "fp32").forward(p, quantise=True)
    assert np.array_equal(_bits(old), _bits(new)) and np.ptp(new, axis=0).min() > 0
    assert not np.array_equal(new, nets(kind, "synthetic").forward(p, quantise=True))
