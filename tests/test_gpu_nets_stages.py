"""-m gpu: the network kernels of csrc/nets.hip one stage at a time (pkg.Net.stage, mods_test_net_stage: the launch functions of
the production path on buffers of the hook's own) against tests/nets_ref.py, a float64 evaluation of the unfolded architecture.

  a  chaining the eight stages through the hook is Net.forward, to the bit
  b  impulse responses: with a bias above every weight the ReLU never clips and an input of isolated ones leaves exactly one
     product per output element, so every element is float32(folded weight + folded bias) or the bias, to the bit - every
     (cout, cin, ky, kx) of all 12 convolution instantiations, the corners, both parities of the stride-2 blocks, the seam
     between two 8-row bands and the last pixel of a partial block; one-hot inputs of the heads reach every head weight
  c  dense random inputs, every stage, n in {1, 4, 5, 9} (5 and 9 leave a block with one live patch), against float64 within
     min((9 cin + 3) 2^-24 S, 8 e_cpu); S = the sum of the magnitudes added into the element (nets_ref.abs_terms), e_cpu = the
     largest deviation of the float32 CPU evaluation from float64 over the same tensor; stages 0 and 7: 8 e_cpu
  d  the whole networks on the golden patches, degenerate patches (constant, 0, 255, one pixel, corners, checkerboard) and noise:
     8 e_cpu; HardNet's bytes equal floor(clip(210 (d64 + 0.45))) unless that lies within 210 * 8 * e_cpu of an integer

Weights: the trained AffNet / OriNet (tests/golden/nets.npz), the daemon's HardNet of seed 5 with random statistics, and for all
three a synthetic state whose running means are as large as the activations (the trained block 0 has means of 1e-3: its bias
is invisible there).

Observed on an MI355X: e_gpu / e_cpu, the largest deviation of the kernel from float64 over that of the float32 CPU evaluation
(c: the largest over the states and the four n; 9 cin = products summed into one element):

    stage            0     1     2     3     4     5     6     7
    C = 16  9 cin    -     9   144   144   288   288   576   4096
            ratio  1.00  1.18  1.20  1.36  1.83  2.04  3.82  1.52
    C = 32  9 cin    -     9   288   288   576   576  1152   8192
            ratio  1.00  1.24  1.85  2.07  3.36  4.01  4.46  bytes: none wrong, at most 1 of 128 exempt

The ratio grows with 9 cin and passes 4 in HardNet's last two blocks.  The cause is the order of the sum, not a term: the kernel
adds the 9 cin products of an element in one float32 chain (input channel, then tap), the CPU's convolution in blocks.  A CPU
emulation of that chain on the folded tensors (fma = a float64 product and sum rounded once) has the kernel's e_gpu to all three
printed digits in every case tried (1.57e-06 for HardNet seed 5, stage 6, n = 4: ratio 4.46), and both stay below 3 % of the
worst-case rounding bound from stage 2 on (34 % at 9 cin = 9, where the float32 CPU evaluation reaches 41 %).
d, quantise off / on: AffNet 1.52 / 1.52 (trained) and 0.91 / 0.91 (synthetic), OriNet 0.71 / 0.98 and 0.87 / 0.87; HardNet no
wrong byte of 11136, exempt shares 4.5e-4 / 3.6e-4 (seed 5) and 1.6e-3 / 6.3e-4 (synthetic).  One-hot heads: 1.17 (AffNet) and
2.93 (OriNet) units in the last place; HardNet no wrong byte of 1048576, 2.4e-4 exempt.
"""
import functools

import numpy as np
import pytest

import nets_ref
from test_gpu_nets import GOLDEN, _golden_state, hardnet_state

pytestmark = pytest.mark.gpu
STATES = [("affnet", "golden"), ("affnet", "synthetic"), ("orinet", "golden"), ("orinet", "synthetic"), ("hardnet", "seed5"),
          ("hardnet", "synthetic")]
IDS = ["%s-%s" % s for s in STATES]


@functools.lru_cache(maxsize=None)
def _state(kind, which):
    if which == "golden":
        return _golden_state(kind)
    if which == "seed5":
        return hardnet_state(5)
    if which == "impulse":
        st = nets_ref.impulse_state(kind, 7)
        if kind == "hardnet":      # no ReLU behind the head: a small mean lets the weight of a one-hot input decide the bytes
            st["features.20.running_mean"] = np.random.default_rng(8).uniform(-0.2, 0.2, 128).astype(np.float32)
        return st
    return nets_ref.synthetic_state(kind, 3)


@pytest.fixture(scope="module")
def nets(pkg):
    d = {}

    def get(kind, which):
        if (kind, which) not in d:
            d[kind, which] = pkg.Net(kind, _state(kind, which))
        return d[kind, which]
    yield get
    for n in d.values():
        n.close()


@functools.lru_cache(maxsize=None)
def _patch_set():
    """e: degenerate and noise patches (nets_ref.special_patches), then the 64 golden ones; 87 = 21 blocks of 4 and one of 3"""
    p = np.concatenate([nets_ref.special_patches(), np.load(GOLDEN)["patches"].astype(np.float32)])
    p.setflags(write=False)
    return p


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ---- a. the hook is the production path ------------------------------------------------------------------------
@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("kind,which", STATES, ids=IDS)
def test_chained_stages_are_forward(pkg, nets, kind, which, quantise):
    net = nets(kind, which)
    p = _patch_set()[7:16]                  # a corner pixel, the checkerboard, integer and non-integer noise
    assert len(p) == 9 and not np.array_equal(p, np.rint(p))
    x = p.reshape(9, 1024)
    for s in range(8):
        assert net.stage_shapes(s) == (nets_ref.in_shape(kind, s) if s else (1, 32, 32), nets_ref.out_shape(kind, s))
        x, ok = net.stage(s, x, quantise=quantise)
        assert ok, s
        if s == 0:                          # the flag reaches the normalisation
            assert not np.array_equal(x, net.stage(0, p.reshape(9, 1024), quantise=not quantise)[0])
    want = net.forward(p, quantise=quantise)
    assert x.shape == want.shape == (9, net.dim) and np.array_equal(x, want)


def test_stage_refuses_bad_arguments(pkg, nets):
    net = nets("affnet", "golden")
    with pytest.raises(pkg.ModsError):
        net.stage(8, np.zeros((1, 1024), np.float32))
    with pytest.raises(pkg.ModsError):
        net.stage(1, np.zeros((1, 1025), np.float32))
    with pytest.raises(pkg.ModsError):
        net.stage(0, np.zeros((pkg.net_chunk() + 1, 1024), np.float32))
    assert pkg.lib().mods_test_net_stage(net.h, 0, None, 1, 0, None, None) == -2


# ---- b. impulse responses ------------------------------------------------------------------------------------
def _impulse_input(cin, h):
    """Patches of isolated ones, each patch within one channel and on a lattice of pitch 5 (two ones never reach the same output,
    and along a lattice line rows and columns alternate in parity).  Patch p: channel p % cin, lattice offset from a list that
    begins with the offsets holding the corners and rows 7 and 8; one more patch than a multiple of 4 (the 8 x 8 maps pack 4
    patches into a block), the last one with the last pixel of the last channel."""
    m = (h - 1) % 5
    valid = range(min(5, h - 5))                                   # at least two lattice points a side
    offs = [o for o in [(0, 0), (m, m), (0, m), (m, 0), (2, 3), (3, 2)] if o[0] in valid and o[1] in valid]
    offs += [(a, b) for a in valid for b in valid if (a, b) not in offs]
    offs = list(dict.fromkeys(offs))
    n = max(cin, 8) + 1
    x = np.zeros((n, cin, h, h), np.float32)
    for p in range(n):
        ci, off = (cin - 1, (m, m)) if p == n - 1 else (p % cin, offs[p % len(offs)])
        x[p, ci, off[0]::5, off[1]::5] = 1.0
    return x


@pytest.mark.parametrize("block", range(6))
@pytest.mark.parametrize("kind", ["affnet", "hardnet"])          # C = 16 (OriNet runs the same six instantiations) and C = 32
def test_convolution_impulse_responses_are_exact(pkg, nets, kind, block):
    st = _state(kind, "impulse")
    cin, cout, stride, h = nets_ref.blocks(kind)[block]
    ho = h // stride
    x = _impulse_input(cin, h)
    n = len(x)
    got, ok = nets(kind, "impulse").stage(block + 1, x)
    assert ok and got.shape == (n, cout, ho, ho)
    # the folded tensors as one rounding each of the float64 values
    inv = 1.0 / np.sqrt(st["features.%d.running_var" % (3 * block + 1)].astype(np.float64) + 1e-5)
    wf = (st["features.%d.weight" % (3 * block)].astype(np.float64) * inv[:, None, None, None]).astype(np.float32)
    bf = (-st["features.%d.running_mean" % (3 * block + 1)].astype(np.float64) * inv).astype(np.float32)
    assert bf.min() > np.abs(wf).max()                            # ReLU never clips
    seen = np.zeros((cin, 3, 3), bool)
    want = np.zeros_like(got)
    for p in range(n):
        ci = int(np.flatnonzero(x[p].any(axis=(1, 2)))[0])
        assert not np.delete(x[p], ci, axis=0).any()
        xp = np.pad(x[p, ci], 1)
        tap = np.zeros((cout, ho, ho), np.float64)
        count = np.zeros((ho, ho))
        for ky in range(3):
            for kx in range(3):
                sel = xp[ky:ky + stride * ho:stride, kx:kx + stride * ho:stride]      # input (oy s + ky - 1, ox s + kx - 1)
                tap += sel[None] * wf[:, ci, ky, kx].astype(np.float64)[:, None, None]
                count += sel
                seen[ci, ky, kx] |= bool(sel.any())
        assert count.max() == 1                                   # one product per element: tap holds a weight or 0, exactly
        want[p] = tap.astype(np.float32) + bf[:, None, None]      # one float32 addition
    pos = x.any(axis=(0, 1))
    ys, xs = np.nonzero(pos)
    assert seen.all()
    assert pos[0, 0] and pos[0, h - 1] and pos[h - 1, 0] and pos[h - 1, h - 1]
    assert {(y % 2, c % 2) for y, c in zip(ys, xs)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if stride == 2:                                               # every input channel at both parities of rows and columns
        for ci in range(cin):
            yy, cc = np.nonzero(x[:, ci].any(axis=0))
            assert {(y % 2, c % 2) for y, c in zip(yy, cc)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if h == 32:
        assert 7 in ys and 8 in ys
    assert x[n - 1, cin - 1, h - 1, h - 1] == 1 and n % 4 == 1
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d of %d elements differ, the first at %s: %r for %r" % (
        len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("kind", nets_ref.KINDS)
def test_head_one_hot_reaches_every_weight(pkg, nets, kind):
    st = _state(kind, "impulse")
    net = nets(kind, "impulse")
    K = 4 * nets_ref.width(kind) * 64
    chunk = 512
    assert chunk <= pkg.net_chunk() and K % chunk == 0
    x = np.zeros((chunk, K), np.float32)
    got = []
    for k0 in range(0, K, chunk):
        x[:] = 0
        x[np.arange(chunk), k0 + np.arange(chunk)] = 1.0
        out, ok = net.stage(7, x)
        assert ok
        got.append(out)
    got = np.concatenate(got)
    W = st["features.19.weight"].reshape(net.dim, K)
    if kind == "hardnet":
        def tail(dt):                       # patch k: y = BatchNorm(W[:, k]), then the unit vector
            y = (W.T.astype(dt) - st["features.20.running_mean"].astype(dt)) / np.sqrt(st["features.20.running_var"].astype(dt) + dt(1e-5))
            return y / np.sqrt((y * y).sum(1, keepdims=True) + dt(1e-10))
        d64 = tail(np.float64)
        e_cpu = np.max(np.abs(tail(np.float32) - d64))
        wrong, exempt = nets_ref.check_hardnet_bytes(got, d64, e_cpu)
        print("hardnet head, one-hot: e_cpu %.3g, %d wrong bytes of %d, exempt share %.3g, bytes %g..%g" % (
            e_cpu, wrong, got.size, exempt, got.min(), got.max()))
        assert got.std() > 10
        assert wrong == 0 and exempt <= 0.01
        return
    ref = []
    for k0 in range(0, K, chunk):
        x[:] = 0
        x[np.arange(chunk), k0 + np.arange(chunk)] = 1.0
        ref.append(nets_ref.stage(kind, st, 7, x))
    ref = np.concatenate(ref)
    if kind == "affnet":                    # the head's tail written out: tanh(W[:, k] + bias) + (1, 0, 1)
        direct = np.tanh(W.T.astype(np.float64) + st["features.19.bias"].astype(np.float64)) + np.array([1.0, 0.0, 1.0])
        assert np.max(np.abs(direct - ref)) < 1e-15
    err = np.abs(got - ref) / _ulp32(ref)
    print("%s head, one-hot: largest error %.2f units in the last place" % (kind, err.max()))
    assert np.ptp(ref, axis=0).min() > 0.3
    assert err.max() <= 4


# ---- c. dense stages against float64 ---------------------------------------------------------------------------
STAGE0_PATCHES = {1: [9], 4: [0, 1, 2, 3], 5: [4, 5, 6, 7, 8], 9: list(range(9, 18))}


def _dense_input(kind, s, n):
    rng = np.random.default_rng(1000 * n + 10 * s + nets_ref.KINDS.index(kind))
    if s == 0:
        return _patch_set()[STAGE0_PATCHES[n]].reshape(n, 1024)
    x = rng.normal(0, 1, (n,) + nets_ref.in_shape(kind, s)).astype(np.float32)
    return x if s == 1 else np.maximum(x, 0)


def _check_against_ref(kind, st, s, x, got, quantise=False):
    """the bound of c for stage s; returns a line of figures, e_gpu / e_cpu among them"""
    ref = nets_ref.stage(kind, st, s, x, quantise=quantise)
    ref32 = nets_ref.stage32(kind, st, s, x, quantise=quantise)
    e_cpu = float(np.max(np.abs(ref32 - ref)))
    if s == 7 and kind == "hardnet":
        wrong, exempt = nets_ref.check_hardnet_bytes(got, ref, e_cpu)
        line = "stage 7 e_cpu %.3g, %d wrong bytes of %d, exempt share %.3g" % (e_cpu, wrong, got.size, exempt)
        print(line)
        assert wrong == 0 and exempt <= 0.01, line
        return None
    err = np.abs(got.astype(np.float64) - ref)
    e_gpu = float(err.max())
    tol = np.full(ref.shape, 8 * e_cpu)
    line = "stage %d e_gpu %.3g e_cpu %.3g ratio %.2f" % (s, e_gpu, e_cpu, e_gpu / e_cpu if e_cpu else float(e_gpu > 0))
    if 1 <= s <= 6:
        worst = (9 * nets_ref.in_shape(kind, s)[0] + 3) * 2.0 ** -24 * nets_ref.abs_terms(kind, st, s, x)
        tol = np.minimum(tol, worst)
        line += ", largest share of the rounding bound %.3g (float32 on the CPU %.3g)" % (np.max(err / worst), np.max(np.abs(ref32 - ref) / worst))
    print(line)
    assert np.all(err <= tol), "%s: %d of %d elements beyond the tolerance" % (line, int(np.sum(err > tol)), err.size)
    return e_gpu / e_cpu if e_cpu else 0.0


@pytest.mark.parametrize("n", [1, 4, 5, 9])
@pytest.mark.parametrize("kind,which", STATES, ids=IDS)
def test_dense_stages_against_float64(pkg, nets, kind, which, n):
    st, net = _state(kind, which), nets(kind, which)
    ratios = []
    for s in range(8):
        x = _dense_input(kind, s, n)
        got, ok = net.stage(s, x)
        assert ok and got.shape == (n,) + nets_ref.out_shape(kind, s), s
        if 1 <= s <= 6:
            assert 0.05 < np.mean(got > 0) < 0.95, s             # the ReLU decides
        ratios.append(_check_against_ref(kind, st, s, x, got))
    print("RATIOS c %s-%s n=%d: %s" % (kind, which, n, " ".join("-" if r is None else "%.2f" % r for r in ratios)))


@pytest.mark.parametrize("quantise", [False, True])
def test_normalisation_on_the_patch_set(pkg, nets, quantise):
    x = _patch_set().reshape(-1, 1024)
    got, ok = nets("orinet", "golden").stage(0, x, quantise=quantise)
    assert ok and len(x) % 4 == 3
    assert not got[:3].any()                                      # constant patches: 0 / 1e-7
    r = _check_against_ref("orinet", None, 0, x, got, quantise)
    print("RATIOS e stage 0 on the patch set, quantise %d: %.2f" % (quantise, r))


# ---- d. whole networks against float64 ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_forward(kind, which, quantise):
    ref = nets_ref.forward(kind, _state(kind, which), _patch_set(), quantise=quantise)
    ref32 = nets_ref.forward32(kind, _state(kind, which), _patch_set(), quantise=quantise)
    return ref, float(np.max(np.abs(ref32 - ref)))


@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("kind,which", STATES, ids=IDS)
def test_whole_network_against_float64(pkg, nets, kind, which, quantise):
    ref, e_cpu = _ref_forward(kind, which, quantise)
    got = nets(kind, which).forward(_patch_set(), quantise=quantise)
    assert got.shape == ref.shape
    if kind == "hardnet":
        wrong, exempt = nets_ref.check_hardnet_bytes(got, ref, e_cpu)
        print("RATIOS d %s-%s quantise %d: e_cpu %.3g, delta %.3g, %d wrong bytes of %d, exempt share %.3g" % (
            kind, which, quantise, e_cpu, 210 * 8 * e_cpu, wrong, got.size, exempt))
        assert got.std() > 5
        assert wrong == 0 and exempt <= 0.01
        return
    e_gpu = float(np.max(np.abs(got - ref)))
    print("RATIOS d %s-%s quantise %d: e_gpu %.3g e_cpu %.3g ratio %.2f" % (kind, which, quantise, e_gpu, e_cpu, e_gpu / e_cpu))
    assert np.ptp(ref, axis=0).min() > 0.05
    assert e_gpu <= 8 * e_cpu
