"""The bf16 mode of the built-in networks (include/mods_hip.h, "bf16 mode") evaluated on the CPU, on top of tests/nets_ref.py:

    bf16(x)        the float32 value x rounded to the nearest bfloat16, ties to even, by bit arithmetic in numpy
    folded()       BatchNorm folded as mods_net_create folds it: wf = float32(float64(W) * inv), bf = float32(-float64(mean) * inv),
                   inv = 1 / sqrt(float64(var) + 1e-5); blocks 2..6 and HardNet's head then use wq = bf16(wf)
    stage_bf16()   one stage of the contract in torch on the CPU in `dtype`: float64 is the reference, float32 the independent
                   evaluation.  Stage 0 is nets_ref's; stage 1 is the convolution with wf; stages 2..6 with wq; all of 1..6 add bf,
                   apply the ReLU and round the result to bf16 (rounded=False returns it before that rounding: what a tolerance
                   interval is built around).  Stage 7: AffNet / OriNet as nets_ref (fp32 weights), HardNet with wq, + bf, then the
                   unit vector.
    forward_bf16() the eight stages chained, activations rounded between them.
"""
import functools

import numpy as np
import torch

import nets_ref


def bf16(x):
    """float32 (or anything that converts to it) -> the nearest bfloat16 as float32, ties to even; finite input"""
    a = np.ascontiguousarray(x, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (u & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(a.shape)


def fold(W, mean, var):
    """the C fold of one layer, spelled out: (wf, bf) in float32"""
    inv = 1.0 / np.sqrt(np.asarray(var, np.float32).astype(np.float64) + 1e-5)
    W = np.asarray(W, np.float32)
    wf = (W.astype(np.float64) * inv.reshape((-1,) + (1,) * (W.ndim - 1))).astype(np.float32)
    bf = (-np.asarray(mean, np.float32).astype(np.float64) * inv).astype(np.float32)
    return wf, bf


def folded(kind, state):
    """{stage s: (weight, bias)} for s = 1..6 and, for HardNet, 7: float32 arrays holding what the bf16 mode multiplies with
    (wf for stage 1, wq = bf16(wf) from stage 2 on) and the fp32 bias"""
    out = {}
    for s in range(1, 7):
        i = 3 * (s - 1)
        wf, bf = fold(state["features.%d.weight" % i], state["features.%d.running_mean" % (i + 1)], state["features.%d.running_var" % (i + 1)])
        out[s] = (wf if s == 1 else bf16(wf), bf)
    if kind == "hardnet":
        wf, bf = fold(state["features.19.weight"], state["features.20.running_mean"], state["features.20.running_var"])
        out[7] = (bf16(wf), bf)
    return out


def rounded_state(kind, state):
    """A state dict whose float64 evaluation by nets_ref multiplies with the rounded operands: weight = the folded weight of
    folded(), running_mean = -bias, running_var = float32(1 - 1e-5), so that 1 / sqrt(var + 1e-5) is 1 to 2e-8.  For
    nets_ref.abs_terms, whose result scales a rounding bound."""
    f = folded(kind, state)
    st = {}
    for s in range(1, 7):
        i = 3 * (s - 1)
        st["features.%d.weight" % i] = f[s][0]
        st["features.%d.running_mean" % (i + 1)] = -f[s][1]
        st["features.%d.running_var" % (i + 1)] = np.full(f[s][1].shape, 1.0 - 1e-5, np.float32)
    return st


def _t(a, dtype):
    return torch.tensor(np.asarray(a)).to(dtype)


def stage_bf16(kind, state, s, x, dtype=torch.float64, quantise=False, rounded=True, _folded=None):
    """stage s of the bf16 mode on x = [n] + nets_ref.in_shape(kind, s); a numpy array of `dtype` (float32 where it was rounded to
    bf16).  The input of stages 2..7 is taken as it is: the caller passes bf16-representable values."""
    if s == 0 or (s == 7 and kind != "hardnet"):
        return nets_ref.stage(kind, state, s, x, dtype, quantise)
    w, b = (_folded or folded(kind, state))[s]
    x = _t(x, dtype)
    n = x.shape[0]
    x = x.reshape((n,) + nets_ref.in_shape(kind, s))
    with torch.no_grad():
        if s == 7:
            y = torch.nn.functional.conv2d(x, _t(w, dtype)).view(n, 128) + _t(b, dtype).view(1, -1)
            return (y / torch.sqrt((y * y).sum(1, keepdim=True) + 1e-10)).numpy()
        stride = nets_ref.blocks(kind)[s - 1][2]
        y = torch.relu(torch.nn.functional.conv2d(x, _t(w, dtype), stride=stride, padding=1) + _t(b, dtype).view(1, -1, 1, 1)).numpy()
    return bf16(y) if rounded else y


def forward_bf16(kind, state, patches, dtype=torch.float64, quantise=False):
    """the whole network in bf16 mode on patches [n][32][32] in 0..255 (HardNet: the unit descriptor, nets_ref.hardnet_bytes)"""
    f = folded(kind, state)
    x = np.asarray(patches).reshape(len(patches), 1024)
    for s in range(8):
        x = stage_bf16(kind, state, s, x, dtype, quantise and s == 0, _folded=f)
    return x


# ---- inputs the CPU and the GPU tests share -----------------------------------------------------------------------
def dense_input(kind, s, n):
    """bf16-representable input of stage s = 2..7: the ReLU of noise"""
    rng = np.random.default_rng(2000 * n + 10 * s + nets_ref.KINDS.index(kind))
    return bf16(np.maximum(rng.normal(0, 1, (n,) + nets_ref.in_shape(kind, s)), 0).astype(np.float32))


HEAD_N = (1, 5, 17)      # patches of the HardNet head cases: one, a few, one more than a workgroup's 16


@functools.lru_cache(maxsize=None)
def head_case(n):
    """(state, input, d64, d32, e_cpu) of HardNet's dense head test with n patches: the unit descriptors of the reference in
    float64 and float32 and their largest difference"""
    st = nets_ref.synthetic_state("hardnet", 3)
    x = dense_input("hardnet", 7, n)
    d64 = stage_bf16("hardnet", st, 7, x)
    d32 = stage_bf16("hardnet", st, 7, x, torch.float32)
    return st, x, d64, d32, float(np.max(np.abs(d32 - d64)))
