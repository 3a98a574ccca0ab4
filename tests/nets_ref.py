"""A plain reference of AffNet, OriNet and HardNet on the CPU, written from the architecture and the tensors of a state dict as
they are (BatchNorm is not folded into anything), one stage at a time:

    stage 0      (x - mean) / (std + 1e-7) per 32 x 32 patch, std with the N - 1 divisor; optionally clip(rint(x), 0, 255) first
    stage 1..6   conv3x3(pad 1, no bias) -> (y - running_mean) / sqrt(running_var + 1e-5) -> ReLU;
                 channels C, C, 2C (stride 2), 2C, 4C (stride 2), 4C with C = 16 (AffNet, OriNet) or 32 (HardNet)
    stage 7      AffNet   conv8x8(64 -> 3) + bias -> tanh -> + (1, 0, 1)
                 OriNet   conv8x8(64 -> 2, pad 1) + bias -> tanh -> mean of the 3 x 3 map
                 HardNet  conv8x8(128 -> 128) -> (y - running_mean) / sqrt(running_var + 1e-5) -> y / sqrt(sum y^2 + 1e-10)

Everything runs in torch on the CPU in `dtype`: float64 is the reference, float32 the independent single-precision evaluation
whose distance from float64 gives the tests their tolerances.  HardNet's stage 7 returns the unit descriptor d; the daemon's
bytes are hardnet_bytes(d) = floor(clip(210 (d + 0.45), 0, 255))."""
import functools

import numpy as np
import torch

KINDS = ("affnet", "orinet", "hardnet")
DIMS = {"affnet": 3, "orinet": 2, "hardnet": 128}
BN_EPS = 1e-5


def width(kind):
    return 32 if kind == "hardnet" else 16


def blocks(kind):
    """(cin, cout, stride, input size) of the six convolution blocks"""
    c = width(kind)
    return [(1, c, 1, 32), (c, c, 1, 32), (c, 2 * c, 2, 32), (2 * c, 2 * c, 1, 16), (2 * c, 4 * c, 2, 16), (4 * c, 4 * c, 1, 8)]


def in_shape(kind, s):
    """shape of one patch's input of stage s"""
    if s == 0:
        return (1024,)
    if s == 7:
        return (4 * width(kind), 8, 8)
    cin, _, _, h = blocks(kind)[s - 1]
    return (cin, h, h)


def out_shape(kind, s):
    if s == 0:
        return (1, 32, 32)
    if s == 7:
        return (DIMS[kind],)
    _, cout, stride, h = blocks(kind)[s - 1]
    return (cout, h // stride, h // stride)


def _t(a, dtype):
    return torch.tensor(np.asarray(a)).to(dtype)             # (a copy: the caller's array may be read-only)


def _bn(y, state, i, dtype):
    mean, var = _t(state["features.%d.running_mean" % i], dtype), _t(state["features.%d.running_var" % i], dtype)
    shape = (1, -1) + (1,) * (y.dim() - 2)
    return (y - mean.view(shape)) / torch.sqrt(var.view(shape) + BN_EPS)


def stage(kind, state, s, x, dtype=torch.float64, quantise=False):
    """stage s of the network `kind` on x = [n] + in_shape(kind, s) (any shape with that many elements per patch); a numpy array
    of `dtype` of shape [n] + out_shape(kind, s)"""
    x = _t(x, dtype)
    n = x.shape[0]
    x = x.reshape((n,) + in_shape(kind, s))
    with torch.no_grad():
        if s == 0:
            if quantise:
                x = torch.clamp(torch.round(x), 0, 255)            # round half to even, as rint
            v = x - x.sum(1, keepdim=True) / 1024
            sd = torch.sqrt((v * v).sum(1, keepdim=True) / 1023) + 1e-7
            y = (v / sd).view(n, 1, 32, 32)
        elif s <= 6:
            _, _, stride, _ = blocks(kind)[s - 1]
            y = torch.nn.functional.conv2d(x, _t(state["features.%d.weight" % (3 * (s - 1))], dtype), stride=stride, padding=1)
            y = torch.relu(_bn(y, state, 3 * (s - 1) + 1, dtype))
        elif kind == "hardnet":
            y = torch.nn.functional.conv2d(x, _t(state["features.19.weight"], dtype)).view(n, 128)
            y = _bn(y, state, 20, dtype)
            y = y / torch.sqrt((y * y).sum(1, keepdim=True) + 1e-10)
        else:
            y = torch.nn.functional.conv2d(x, _t(state["features.19.weight"], dtype), _t(state["features.19.bias"], dtype),
                                           padding=1 if kind == "orinet" else 0)
            y = torch.tanh(y).mean(dim=(2, 3))
            if kind == "affnet":
                y = y + torch.tensor([1.0, 0.0, 1.0], dtype=dtype)
    return y.numpy()


def forward(kind, state, patches, dtype=torch.float64, quantise=False):
    """the whole network on patches [n][32][32] in 0..255 (HardNet: the unit descriptor, see hardnet_bytes)"""
    x = np.asarray(patches).reshape(len(patches), 1024)
    for s in range(8):
        x = stage(kind, state, s, x, dtype, quantise and s == 0)
    return x


def stage32(kind, state, s, x, quantise=False):
    return stage(kind, state, s, x, torch.float32, quantise)


def forward32(kind, state, patches, quantise=False):
    return forward(kind, state, patches, torch.float32, quantise)


def abs_terms(kind, state, s, x):
    """S of a convolution stage (1..6) in float64: conv(|x|, |W|) / sqrt(var + eps) + |mean| / sqrt(var + eps), the sum of the
    magnitudes of everything that is added into an output element - what a rounding bound of that element scales with"""
    assert 1 <= s <= 6
    x = _t(x, torch.float64)
    x = x.reshape((x.shape[0],) + in_shape(kind, s)).abs()
    i = 3 * (s - 1)
    inv = 1.0 / torch.sqrt(_t(state["features.%d.running_var" % (i + 1)], torch.float64) + BN_EPS).view(1, -1, 1, 1)
    with torch.no_grad():
        y = torch.nn.functional.conv2d(x, _t(state["features.%d.weight" % i], torch.float64).abs(), stride=blocks(kind)[s - 1][2], padding=1)
    return (y * inv + _t(state["features.%d.running_mean" % (i + 1)], torch.float64).abs().view(1, -1, 1, 1) * inv).numpy()


def hardnet_q(d):
    """210 (d + 0.45) in float64: what the daemon clips to 0..255 and truncates to a byte"""
    return 210.0 * (np.asarray(d, np.float64) + 0.45)


def hardnet_bytes(d):
    return np.floor(np.clip(hardnet_q(d), 0, 255))


def check_hardnet_bytes(got, d64, e_cpu):
    """The rule for HardNet's bytes: a byte equals floor(clip(q64)) unless q64 lies within delta = 210 * 8 * e_cpu of an integer,
    where the byte on either side is taken.  Returns (number of wrong bytes, share of bytes that the exception covered)."""
    delta = 210.0 * 8.0 * e_cpu
    q = hardnet_q(d64)
    lo, hi = np.floor(np.clip(q - delta, 0, 255)), np.floor(np.clip(q + delta, 0, 255))
    got = np.asarray(got, np.float64)
    assert got.shape == q.shape
    return int(np.sum((got != lo) & (got != hi))), float(np.mean(lo != hi))


# ---- state dicts ---------------------------------------------------------------------------------------------
def tensor_shapes(kind):
    out = []
    for i, (cin, cout, _, _) in enumerate(blocks(kind)):
        out += [("features.%d.weight" % (3 * i), (cout, cin, 3, 3)), ("features.%d.running_mean" % (3 * i + 1), (cout,)),
                ("features.%d.running_var" % (3 * i + 1), (cout,))]
    if kind == "hardnet":
        out += [("features.19.weight", (128, 128, 8, 8)), ("features.20.running_mean", (128,)), ("features.20.running_var", (128,))]
    else:
        out += [("features.19.weight", (DIMS[kind], 64, 8, 8)), ("features.19.bias", (DIMS[kind],))]
    return out


@functools.lru_cache(maxsize=None)
def synthetic_state(kind, seed):
    """Random weights, running_var in [0.5, 2], and a running_mean of the size of what it is subtracted from: per channel the mean
    of the convolution's output over a few noise patches plus up to one standard deviation either way, so that every (folded)
    bias decides which elements the ReLU keeps.  The heads of AffNet and OriNet are scaled to keep tanh out of saturation."""
    rng = np.random.default_rng(seed)
    st = {}
    x = stage(kind, st, 0, rng.uniform(0, 255, (6, 1024)))
    for i, (cin, cout, stride, _) in enumerate(blocks(kind)):
        w = rng.normal(0, np.sqrt(2.0 / (9 * cin)), (cout, cin, 3, 3)).astype(np.float32)
        var = rng.uniform(0.5, 2.0, cout).astype(np.float32)
        with torch.no_grad():
            y = torch.nn.functional.conv2d(_t(x, torch.float64), _t(w, torch.float64), stride=stride, padding=1).numpy()
        mean = (y.mean((0, 2, 3)) + rng.uniform(-1, 1, cout) * y.std((0, 2, 3))).astype(np.float32)
        st.update({"features.%d.weight" % (3 * i): w, "features.%d.running_mean" % (3 * i + 1): mean, "features.%d.running_var" % (3 * i + 1): var})
        x = stage(kind, st, i + 1, x)
    k = x[0].size
    if kind == "hardnet":
        w = rng.normal(0, np.sqrt(2.0 / k), (128, 128, 8, 8)).astype(np.float32)
        y = x.reshape(len(x), -1) @ w.reshape(128, -1).T.astype(np.float64)
        st["features.19.weight"] = w
        st["features.20.running_mean"] = (y.mean(0) + rng.uniform(-1, 1, 128) * y.std(0)).astype(np.float32)
        st["features.20.running_var"] = rng.uniform(0.5, 2.0, 128).astype(np.float32)
    else:
        st["features.19.weight"] = rng.normal(0, 0.5 / np.sqrt(k * float(np.mean(x * x))), (DIMS[kind], 64, 8, 8)).astype(np.float32)
        st["features.19.bias"] = rng.uniform(-0.3, 0.3, DIMS[kind]).astype(np.float32)
    assert [(n, st[n].shape) for n, _ in tensor_shapes(kind)] == tensor_shapes(kind)
    return st


def impulse_state(kind, seed):
    """Weights in [-0.5, 0.5], running_var in [0.5, 2] and running_mean = -(2 + r) sqrt(var + 1e-5), r in [0, 1]: the folded bias
    (2 + r) exceeds every folded weight (at most 0.5 / sqrt(0.5)), so bias + one weight is never clipped by the ReLU.  The heads of
    AffNet and OriNet: weights in [-0.5, 0.5]; the bias 0.6 wherever outputs are added (to 1, or over the 3 x 3 map), so that
    no sum cancels and an error of tanh in units of the last place stays one of the result."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, shape in tensor_shapes(kind):
        if name.endswith("weight"):
            st[name] = rng.uniform(-0.5, 0.5, shape).astype(np.float32)
        elif name.endswith("running_var"):
            st[name] = rng.uniform(0.5, 2.0, shape).astype(np.float32)
    for name, shape in tensor_shapes(kind):
        if name.endswith("running_mean"):
            var = st[name.replace("running_mean", "running_var")].astype(np.float64)
            st[name] = (-(2.0 + rng.uniform(0, 1, shape)) * np.sqrt(var + BN_EPS)).astype(np.float32)
    if kind == "affnet":
        st["features.19.bias"] = np.array([0.6, rng.uniform(-0.3, 0.3), 0.6], np.float32)
    elif kind == "orinet":
        st["features.19.bias"] = np.array([0.6, 0.6], np.float32)
    return st


# ---- patches ---------------------------------------------------------------------------------------------------
def special_patches(seed=11):
    """Integer-valued patches in 0..255 that stress the normalisation and the zero padding (their sums are exact in float32, so
    the comparison stays well conditioned where std is tiny): constant 77, all 0, all 255, 100 with one pixel 101, a single 255
    in each corner, a checkerboard of 0 and 255, noise; then a dozen non-integer noise patches.  Their std is 20 and more: float32 rounds the mean of non-integer values near 128
    to 2^-17, an offset of 2^-17 / std on every normalised pixel, which at a std of 1 is a hundred times the rounding noise of
    the rest of the network - in any float32 evaluation, the reference's own included."""
    rng = np.random.default_rng(seed)
    p = [np.full((32, 32), 77.0), np.zeros((32, 32)), np.full((32, 32), 255.0), np.full((32, 32), 100.0)]
    p[3][13, 21] = 101.0
    for y, x in ((0, 0), (0, 31), (31, 0), (31, 31)):
        c = np.zeros((32, 32))
        c[y, x] = 255.0
        p.append(c)
    yy, xx = np.mgrid[0:32, 0:32]
    p.append(255.0 * ((yy + xx) % 2))
    p += [rng.integers(0, 256, (32, 32)).astype(np.float64), rng.integers(90, 110, (32, 32)).astype(np.float64)]
    n_int = len(p)
    for i in range(12):
        p.append(np.clip(rng.uniform(20, 235) + rng.normal(0, (20.0, 40.0, 70.0)[i % 3], (32, 32)), 0, 255))
    p = np.array(p, np.float32)
    assert np.array_equal(p[:n_int], np.rint(p[:n_int])) and p[n_int:].reshape(12, -1).std(1).min() >= 1
    return p
