"""The contract of the doubled first octave (mods_ctx_upscale_input; include/mods_hip.h) restated for the tests: double_image in
numpy, and the whole upscaled scale space composed from the CPU oracle's own primitives.  The oracle itself has no such switch
(its initial blur assumes an input blur of 0.5), so where the contract's initial blur runs (initialSigma > 1.0) these planes are
the reference; where it does not (initialSigma <= 0.5 skips it on both sides) they equal orc.Pyramid(double_image(img)), which
tests/test_cpu_upscale.py checks.  Test infrastructure only."""
import ctypes as C

import numpy as np

import orc

MAX_OCTAVES = 16     # kMaxOctaves of the library


def double_image(img):
    """D of 2h x 2w from I of h x w, fp32, one rounding per operation, in the order the contract writes:
        D[2r, 2c] = a                     D[2r, 2c + 1]     = 0.5f * (a + b)
        D[2r + 1, 2c] = 0.5f * (a + c_)   D[2r + 1, 2c + 1] = 0.25f * (((a + b) + c_) + d)
    with a = I[r, c], b = I[r, c'], c_ = I[r', c], d = I[r', c'], r' = min(r + 1, h - 1), c' = min(c + 1, w - 1)."""
    f = np.float32
    a = np.ascontiguousarray(img, np.float32)
    h, w = a.shape
    rn = np.minimum(np.arange(h) + 1, h - 1)
    cn = np.minimum(np.arange(w) + 1, w - 1)
    b, c_, d = a[:, cn], a[rn, :], a[rn][:, cn]
    out = np.empty((2 * h, 2 * w), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        out[0::2, 0::2] = a
        out[0::2, 1::2] = f(0.5) * (a + b)
        out[1::2, 0::2] = f(0.5) * (a + c_)
        out[1::2, 1::2] = f(0.25) * (((a + b) + c_) + d)
    return out


def _kind(params):
    return 3 if (params.detectorType == 1 and params.iiDoGMode) else int(params.detectorType)


def planes(img, params=None):
    """The upscaled scale space of `img`: (dims, planes) with dims[o] = (w, h) of octave o and planes[(o, level, kind)] the blur
    (kind 0) and response (kind 1) planes.  Octave 0 is double_image(img); the input is assumed to carry a blur of 1.0, so the
    initial blur runs only for initialSigma > 1.0, with sigma = sqrtf(initialSigma^2 - 1.0f); the rest is the oracle's schedule
    (oracle/detect.cpp: build_pyramid) in fp32."""
    f = np.float32
    p = params or orc.HessAffParams.default()
    S, s0 = int(p.numberOfScales), f(p.initialSigma)
    step = f(orc.lib().orc_det_pow2f(C.c_float(f(1.0) / f(S))))
    first = double_image(img)
    if s0 > f(1.0):
        first = orc.gauss_blur(first, float(np.sqrt(s0 * s0 - f(1.0) * f(1.0))))
    kind = _kind(p)
    min_size = 2 * p.border + 2
    dims, out = [], {}
    while first.shape[0] > min_size and first.shape[1] > min_size and len(dims) < MAX_OCTAVES:
        o = len(dims)
        dims.append((first.shape[1], first.shape[0]))
        cur = s0
        blur = first
        out[(o, 0, 0)] = blur
        out[(o, 0, 1)] = orc.response(blur, float(cur * cur), kind)
        nxt = None
        for lv in range(1, S + 2):
            blur = orc.gauss_blur(blur, float(cur * np.sqrt(step * step - f(1.0))))
            sigma = cur * step
            out[(o, lv, 0)] = blur
            out[(o, lv, 1)] = orc.response(blur, float(sigma * sigma), kind)
            if lv == S:
                nxt = orc.resize_half(blur)
            cur = cur * step
        first = nxt
    return dims, out


def halved(keys):
    """The oracle's keys of a doubled image carried to the original image's coordinates: x, y, s halved (exact)."""
    k = keys.copy()
    for fld in ("x", "y", "s"):
        k[fld] = k[fld] * 0.5
    return k
