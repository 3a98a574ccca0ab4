"""Domain-size pooling of SIFT descriptors (mods_ctx_domain_pooling; contract in include/mods_hip.h), restated with numpy.

The raw histogram is sift_from_patch's (csrc/sift.hip) up to `s_vec`: fp32 gradients, the table-driven atan2 (the table of
tools/gen_atan_lut.py), samplePatch's bins and weights, per-bin sums in raster order in double (np.cumsum on float64 is the
ordered sum).  The tail is the one every SIFT kernel shares: HalfSIFT fold, normalise / clip / renormalise with the length summed
in 4-term groups, RootSIFT or plain SIFT, quantisation.  tests/test_cpu_dsp.py pins the restatement, with one patch and no pooling,
to the CPU oracle's orc.sift_desc byte for byte; patches come from orc.extract_desc_patch."""
import importlib.util
import os

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
TWO_PI = 6.28318530718          # M_PI_DOUBLED of computeSiftDescriptor


def _lut():
    spec = importlib.util.spec_from_file_location("gen_atan_lut", os.path.join(ROOT, "tools", "gen_atan_lut.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return np.array([float(v) for v in mod.table()], np.float64)


LUT = _lut()
_masks, _weights = {}, {}


def coefficients(K, start, end):
    """c_k = start + k * ((end - start) / (K - 1)), in double"""
    step = (float(end) - float(start)) / (K - 1)
    return [float(start) + k * step for k in range(K)]


def mask(ps):
    if ps not in _masks:
        _masks[ps] = orc.circular_gauss_mask(ps, 0.0)
    return _masks[ps]


def spatial_weights(ps):
    """precomputeBinsAndWeights (siftdesc.cpp:22-71) as sift_tables holds it: w[b][i] = weight of pixel line i for spatial bin b"""
    if ps not in _weights:
        step = F32(5.0) / F32(2 * (ps >> 1))
        w = np.zeros((4, ps), F32)
        for i in range(ps):
            x = F32(step * F32(i))
            xi = int(x)
            w1 = F32(x - F32(xi))
            w0 = F32(F32(1.0) - w1)
            b0, b1 = xi - 1, xi
            if b0 < 0:
                b0, w0 = 0, F32(0)
            if b0 >= 4:
                b0, w0 = 3, F32(0)
            if b1 >= 4:
                b1, w1 = 3, F32(0)
            for b in range(4):
                acc = F32(0)
                if b0 == b:
                    acc = F32(acc + w0)
                if b1 == b:
                    acc = F32(acc + w1)
                w[b, i] = acc
        _weights[ps] = w
    return _weights[ps]


def photonorm(patch):
    """photometricallyNormalize (helpers.cpp:666-715) as photonorm_patch runs it: fp32, ordered sums over the masked pixels"""
    p = np.ascontiguousarray(patch, F32)
    m = mask(p.shape[0]) > 0
    g = p[m]                                        # raster order
    n = F32(len(g))
    mean = F32(np.cumsum(g, dtype=F32)[-1] / n)
    d = (mean - g).astype(F32)
    var = F32(np.sqrt(F32(np.cumsum((d * d).astype(F32), dtype=F32)[-1] / n)))
    if float(var) < 0.0001:
        return p.copy()
    fac = F32(F32(50.0) / var)
    v = (F32(128) + (fac * (p - mean).astype(F32)).astype(F32)).astype(F32)
    return np.clip(v, F32(0), F32(255)).astype(F32)


def _atan2_lut(y, x):
    """atan2LUTff (helpers.cpp:160-207), elementwise on fp32 arrays"""
    ax, ay = np.abs(x), np.abs(y)
    first = ax > ay
    num, den = np.where(first, ay, ax), np.where(first, ax, ay)
    zero = (~(x > 0)) & (~(y > 0)) & (~first) & (x == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ((F32(255.0) * num).astype(F32) / den).astype(F32)
    idx = np.where(zero, 0, np.nan_to_num(q, nan=0.0, posinf=0.0)).astype(np.int64)
    L = LUT[idx]
    pi2, pi = float(F32(1.57079632679489661923)), float(F32(3.14159265358979323846))
    xp, yp = x > 0, y > 0
    out = np.where(xp & yp, np.where(first, L, pi2 - L),
                   np.where(xp, np.where(first, -L, -pi2 + L),
                            np.where(yp, np.where(first, pi - L, pi2 + L), np.where(first, -pi + L, -pi2 - L))))
    return np.where(zero, 0.0, out).astype(F32)


def raw_histogram(patch):
    """vec[128] of computeSiftDescriptor after the samplePatch loop (bin = (br * 4 + bc) * 8 + bo), in double"""
    p = np.ascontiguousarray(patch, F32)
    ps = p.shape[0]
    xg, yg = np.empty_like(p), np.empty_like(p)
    xg[:, 1:-1] = p[:, 2:] - p[:, :-2]
    xg[:, 0] = p[:, 1] - p[:, 0]
    xg[:, -1] = p[:, -1] - p[:, -2]
    yg[1:-1, :] = p[2:, :] - p[:-2, :]
    yg[0, :] = p[1, :] - p[0, :]
    yg[-1, :] = p[-1, :] - p[-2, :]
    grad = np.sqrt(((xg * xg).astype(F32) + (yg * yg).astype(F32)).astype(F32)).astype(F32)
    ori = _atan2_lut(yg, xg)
    o = (8.0 * (ori.astype(np.float64) + TWO_PI) / TWO_PI).astype(F32)
    bo0 = o.astype(np.int32)
    wo1 = (o - bo0.astype(F32)).astype(F32)
    wo0 = (F32(1.0) - wo1).astype(F32)
    bo0 = bo0 % 8
    gm = (mask(ps) * grad).astype(F32)
    w = spatial_weights(ps)
    vec = np.zeros(128, np.float64)
    for br in range(4):
        rows = np.nonzero(w[br] > 0)[0]
        for bc in range(4):
            cols = np.nonzero(w[bc] > 0)[0]
            sl = (slice(rows[0], rows[-1] + 1), slice(cols[0], cols[-1] + 1))
            val = (w[br][sl[0], None] * (w[bc][None, sl[1]] * gm[sl]).astype(F32)).astype(F32)
            pos = val > 0
            b0, a0, a1 = bo0[sl], wo0[sl], wo1[sl]
            for bo in range(8):
                m0, m1 = b0 == bo, ((b0 + 1) & 7) == bo
                contrib = np.where(pos & m0, (val * a0).astype(F32), np.where(pos & m1, (val * a1).astype(F32), F32(0)))
                vec[(br * 4 + bc) * 8 + bo] = np.cumsum(contrib.ravel().astype(np.float64))[-1]
    return vec


def tail(vec, rootsift=True, max_bin=0.2, half=False):
    """the shared tail on a raw (pooled) histogram -> 128 bytes"""
    v = np.array(vec, np.float64)
    if half:        # doHalfSIFT (siftdesc.cpp:411-436): half[i*4 + j] = vec[i*8 + j] + vec[i*8 + j + 4]; the upper 64 are zero
        r = v.reshape(16, 8)
        v = np.concatenate([(r[:, :4] + r[:, 4:]).ravel(), np.zeros(64)])
    with np.errstate(divide="ignore", invalid="ignore"):
        for rnd in range(2):
            sq = v * v
            groups = ((sq[0::4] + sq[1::4]) + sq[2::4]) + sq[3::4]
            inv = 1.0 / np.sqrt(np.cumsum(groups)[-1])
            v = v * inv
            if rnd == 0:
                over = v > max_bin
                if not over.any():
                    break
                v = np.where(over, max_bin, v)
        if rootsift:
            v = np.sqrt(v / np.cumsum(np.abs(v))[-1])
        q = (512.0 * v + 0.5).astype(np.int64)
    return np.clip(q, 0, 255).astype(np.uint8)


def pooled_histogram(patches, photo=False):
    """((h_0 + h_1) + h_2) + ... of the patches' raw histograms, in double, in order"""
    acc = None
    for p in patches:
        h = raw_histogram(photonorm(p) if photo else p)
        acc = h if acc is None else acc + h
    return acc


def pooled_descriptor(patches, rootsift=True, max_bin=0.2, half=False, photo=False):
    """what mods_test_sift_pooled computes from K patches of one region"""
    return tail(pooled_histogram(patches, photo), rootsift, max_bin, half)


class Describer:
    """Pooled raw histograms of the regions of one image, computed once per (region, domain size) and shared by the tests"""

    def __init__(self, img, regions, mrsize=orc.DESC_MRSIZE, ps=orc.DESC_PATCH, photonorm=True):
        self.img, self.regions, self.mrsize, self.ps, self.photonorm = img, regions, float(mrsize), ps, photonorm
        self._hist, self._pooled = {}, {}

    def _h(self, i, mr):
        if (i, mr) not in self._hist:
            patch = orc.extract_desc_patch(self.img, self.regions[i:i + 1], mrsize=mr, ps=self.ps, photonorm=self.photonorm)
            self._hist[(i, mr)] = raw_histogram(patch)
        return self._hist[(i, mr)]

    def pooled(self, K, start, end):
        """[n][128] pooled raw histograms"""
        key = (K, float(start), float(end))
        if key not in self._pooled:
            out = np.zeros((len(self.regions), 128), np.float64)
            for i in range(len(self.regions)):
                acc = None
                for c in coefficients(K, start, end):
                    h = self._h(i, self.mrsize * c)
                    acc = h if acc is None else acc + h
                out[i] = acc
            self._pooled[key] = out
        return self._pooled[key]

    def descriptors(self, K, start, end, rootsift=True, max_bin=0.2, half=False):
        """[n][128] bytes of the pooled call"""
        pooled = self.pooled(K, start, end)
        return np.stack([tail(h, rootsift, max_bin, half) for h in pooled]) if len(pooled) else np.zeros((0, 128), np.uint8)
