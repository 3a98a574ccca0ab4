"""ctypes binding of libmodsgpu.so (include/mods_hip.h): the MI355X implementation of the MODS
detect -> describe -> match -> verify hot path.

The directory name carries a hyphen (repository contract), so load it with
`import importlib.util` (see `__graft_entry__.load_package()`), not with `import`.

There is no CPU path: every call fails loudly when the shared library or a HIP device is
missing."""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MODS_LIB") or os.path.join(PKG_DIR, "libmodsgpu.so")

MODS_OK = 0
STAGES = ["blur", "response", "resize", "nms", "localize", "baumberg", "sort", "orient", "describe", "match",
          "ransac_score", "synth", "blur_small", "pyramid", "match_nn1", "extract", "sift", "guided", "match_mutual",
          "overlap", "overlap_area"]
# MODS_STAGE_* added after that list was pinned by its users: their indices follow it
STAGES_LATER = ["local_affine", "reproject_h", "spatial_select", "knn", "knn_sweep", "distractor", "distractor_sweep", "refine", "propagate"]


def stage_index(name):
    """MODS_STAGE_* of a stage name"""
    return STAGES.index(name) if name in STAGES else len(STAGES) + STAGES_LATER.index(name)


class ModsError(RuntimeError):
    pass


class HessAffParams(C.Structure):
    """[HessianAffine] section of the reference .ini (io_mods.cpp:167-207)."""
    _fields_ = [("numberOfScales", C.c_int), ("initialSigma", C.c_float), ("threshold", C.c_float),
                ("edgeEigenValueRatio", C.c_float), ("border", C.c_int), ("maxIterations", C.c_int),
                ("convergenceThreshold", C.c_float), ("smmWindowSize", C.c_int), ("doBaumberg", C.c_int),
                ("mode", C.c_int), ("relativeThreshold", C.c_float), ("regionsNumber", C.c_int),
                ("relativeRegionsNumber", C.c_float), ("detectorType", C.c_int), ("iiDoGMode", C.c_int),
                ("sampleFromImage", C.c_int),
                ("mserMaxArea", C.c_double), ("mserMinMargin", C.c_double), ("mserMinSize", C.c_int), ("affBmbrgMethod", C.c_int)]

    @staticmethod
    def mser(mode=0, min_margin=8, max_area=0.05, min_size=30, reg_number=500, rel_threshold=-1.0, rel_reg_number=-1.0):
        """[MSER] of build/config_affori_classic.ini (DetectorType = DET_MSER, detectors/structures.hpp:19; io_mods.cpp:101-123)."""
        p = HessAffParams(3, 1.6, 5.33, 10.0, 5, 16, 0.05, 19, 1, mode, rel_threshold, reg_number, rel_reg_number, 3, 0, 0)
        p.mserMaxArea, p.mserMinMargin, p.mserMinSize = max_area, min_margin, min_size
        return p

    @staticmethod
    def default():
        # build/config_affori_classic.ini; mode FixedTh, the other selection keys at PyramidParams' defaults (-1)
        return HessAffParams(3, 1.6, 5.33, 10.0, 5, 16, 0.05, 19, 1, 0, -1.0, -1, -1.0, 0, 0, 0)

    @staticmethod
    def dog():
        """[DoG] of build/config_affori_classic.ini: the same detector searching the difference-of-Gaussians response
        (DetectorType = DET_DOG, io_mods.cpp:260-262)."""
        return HessAffParams(3, 1.6, 8.0, 10.0, 5, 32, 0.05, 19, 0, 0, 0.01, 3000, 0.5, 1, 0, 0)

    @staticmethod
    def harris():
        """[HarrisAffine] of build/config_affori_classic.ini (DetectorType = DET_HARRIS, io_mods.cpp:208-210)."""
        return HessAffParams(3, 1.6, 15.0, 10.0, 5, 16, 0.1, 19, 0, 0, 0.1, 1000, 0.5, 2, 0, 0)


AFFKEY_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("s", "f8"), ("a11", "f8"), ("a12", "f8"), ("a21", "f8"),
                         ("a22", "f8"), ("response", "f8"), ("sub_type", "i4"), ("octave", "i4"),
                         ("level", "i4"), ("r0", "i4"), ("c0", "i4"), ("pad", "i4")])
CAND_DTYPE = np.dtype([("octave", "i4"), ("level", "i4"), ("r0", "i4"), ("c0", "i4"), ("r", "i4"), ("c", "i4"),
                       ("x", "f4"), ("y", "f4"), ("s", "f4"), ("pixelDistance", "f4"), ("response", "f4"),
                       ("type", "i4")])

REGION_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("s", "f8"), ("a11", "f8"), ("a12", "f8"), ("a21", "f8"),
                         ("a22", "f8"), ("response", "f8"), ("sub_type", "i4"), ("id", "i4"), ("parent", "i4"),
                         ("pad", "i4"), ("desc", "u1", (128,))])


class DescribeParams(C.Structure):
    """[DominantOrientation] + [SIFTDescriptor] (io_mods.cpp:731-740, 423-436)."""
    _fields_ = [("ori_mrSize", C.c_double), ("ori_patchSize", C.c_int), ("ori_maxAngles", C.c_int),
                ("ori_threshold", C.c_double), ("desc_mrSize", C.c_double), ("desc_patchSize", C.c_int),
                ("photoNorm", C.c_int), ("rootSift", C.c_int), ("maxBinValue", C.c_double),
                ("ori_halfMode", C.c_int), ("addUpRight", C.c_int), ("halfDesc", C.c_int), ("fastExtraction", C.c_int)]

    @staticmethod
    def default():
        # config_affori_classic.ini; threshold is parsed into a float member (descriptors_parameters.hpp:10)
        return DescribeParams(5.1962, 32, 1, float(np.float32(0.8)), 5.1962, 41, 1, 1, 0.2, 0, 0, 0, 0)


_lib = None


def build():
    """Compile every HIP source for gfx950 into libmodsgpu.so (in-tree)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", PKG_DIR])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ModsError("libmodsgpu.so is not built (run __graft_entry__.build()); there is no CPU path")
        # PyTorch-ROCm bundles its own libamdhip64.so.7.  Two HIP runtimes in one process do not
        # share devices, so when torch is used for device memory / torch.distributed it must be
        # loaded first: libmodsgpu's NEEDED libamdhip64.so.7 then binds to the copy already mapped.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.mods_last_error.restype = C.c_char_p
        _lib.mods_ctx_stream.restype = C.c_void_p
    return _lib


def _check(rc):
    if rc != MODS_OK:
        raise ModsError("libmodsgpu error %d: %s" % (rc, lib().mods_last_error().decode()))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _tentatives(room, call):
    """room for tentatives, their correspondences and their frames; call(tent, u6, laf, n) runs the search that fills them and
    returns its code; returns (tent, u6, laf) cut to the count"""
    room = max(room, 1)
    out = np.zeros(room, TENT_DTYPE)
    u6 = np.zeros((room, 6), np.float64)
    laf = np.zeros((room, 14), np.float64)
    n = C.c_int()
    _check(call(_vp(out), _vp(u6), _vp(laf), C.byref(n)))
    return out[:n.value].copy(), u6[:n.value].copy(), laf[:n.value].copy()


def _overlap(fn, dtype, lists, params, cap):
    """one of the four overlap searches: fn(*lists, params, out, cap, n, counts) with room for cap rows of dtype; returns (matches
    cut to the count, OverlapCounts)"""
    out = np.zeros(max(cap, 1), dtype)
    n = C.c_int()
    counts = OverlapCounts()
    _check(fn(*lists, C.byref(params), _vp(out), cap, C.byref(n), C.byref(counts)))
    return out[:n.value].copy(), counts


def _mask_rows(mask):
    """a detection mask as the library takes it: (array that owns the bytes, row stride in bytes); a 2-D uint8 array whose rows are
    contiguous keeps its row stride, anything else is copied dense"""
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.ndim != 2 or m.size == 0:
        raise ValueError("a detection mask is a non-empty 2-D uint8 array")
    if m.strides[1] != 1 or m.strides[0] < m.shape[1]:
        m = np.ascontiguousarray(m)
    return m, m.strides[0]


def detection_mask_test(mask, x, y):
    """the on-mask rule (mods_detection_mask_test) for one point: True when (x, y) is on the mask; no device needed"""
    m, stride = _mask_rows(mask)
    return bool(lib().mods_detection_mask_test(_vp(m), m.shape[1], m.shape[0], stride, C.c_double(x), C.c_double(y)))


def u8_strips_layout(w, h):
    """(width limit, strips per image, bytes per strip, bytes per image) of the 8-bit strip copy of a w x h image (csrc/u8_strips.hpp;
    no device needed)"""
    lim, ns, pitch, nbytes = C.c_uint(), C.c_uint(), C.c_uint(), C.c_size_t()
    _check(lib().mods_u8_strips_layout(int(w), int(h), C.byref(lim), C.byref(ns), C.byref(pitch), C.byref(nbytes)))
    return lim.value, ns.value, pitch.value, nbytes.value


def u8_strips_strip_of(n):
    """the strip of each column 0 .. n - 1, by the multiply and shift the kernels use"""
    out = np.zeros(int(n), np.uint32)
    lib().mods_u8_strips_strip_of(C.c_uint(int(n)), C.c_void_p(out.ctypes.data))
    return out


def u8_strips_offsets(w, h):
    """byte offset in an image's strip copy of every pixel (x <= w - 2, y <= h - 2) that a pixel pair can start at: uint32 [h - 1][w - 1]"""
    out = np.zeros((int(h) - 1, int(w) - 1), np.uint32)
    _check(lib().mods_u8_strips_offsets(int(w), int(h), C.c_void_p(out.ctypes.data)))
    return out


class ViewGeom(C.Structure):
    """mods_view_geom: what GenerateSynthImageCorr derives before touching pixels."""
    _fields_ = [("identity", C.c_int), ("w_rot", C.c_int), ("h_rot", C.c_int), ("w_new", C.c_int), ("h_new", C.c_int),
                ("ksize_x", C.c_int), ("ksize_y", C.c_int), ("pad", C.c_int),
                ("rotation", C.c_double), ("tilt", C.c_double), ("zoom", C.c_double), ("sigma_x", C.c_double),
                ("sigma_y", C.c_double), ("H", C.c_double * 9), ("warpRot", C.c_double * 6), ("warpTilt", C.c_double * 6)]


def view_geometry(w, h, tilt, phi, zoom=1.0, init_sigma=0.2):
    g = ViewGeom()
    _check(lib().mods_view_geometry(w, h, C.c_double(tilt), C.c_double(phi), C.c_double(zoom), C.c_double(init_sigma), C.byref(g)))
    return g


def view_geometry_h(w, h, H, clip_w=None, clip_h=None, init_sigma=0.2):
    """mods_view_geometry_h: the geometry of the view of a w x h image through the homography H (original -> view), its size
    clipped to clip_w x clip_h (default: the image's own); no device needed"""
    g = ViewGeom()
    Hc = np.ascontiguousarray(H, np.float64).ravel()
    _check(lib().mods_view_geometry_h(w, h, _vp(Hc), clip_w or w, clip_h or h, C.c_double(init_sigma), C.byref(g)))
    return g


def view_ctx_dims(w, h):
    """Context size that holds every rotated intermediate of a w x h image."""
    d = int(np.ceil(np.hypot(w, h))) + 2
    return d, d


class ClaheParams(C.Structure):
    """mods_clahe_params: [Matching] doCLAHE of mods.cpp:133-189 (createCLAHE(), setClipLimit(4): 8 x 8 tiles)."""
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int)]

    @staticmethod
    def reference():
        return ClaheParams(4.0, 8, 8)


NET_KINDS = {"affnet": 0, "orinet": 1, "hardnet": 2}
NET_DIMS = {"affnet": 3, "orinet": 2, "hardnet": 128}
NET_PRECISIONS = {"fp32": 0, "bf16": 1}          # MODS_NET_FP32, MODS_NET_BF16
_NET_SLOTS = {"shape": "affnet", "orientation": "orinet", "descriptor": "hardnet"}


def net_tensor_spec(kind):
    """[(name, shape)] of the tensors a network of `kind` takes, in network order, under the names of the daemon's state dict
    (zmq_daemon.build_model; `<kind>.` stripped from the arrays of a --weights FILE.npz)."""
    if kind not in NET_KINDS:
        raise ModsError("unknown network kind %r (one of %s)" % (kind, ", ".join(sorted(NET_KINDS))))
    c = 32 if kind == "hardnet" else 16
    spec = []
    for i, (cin, cout) in enumerate([(1, c), (c, c), (c, 2 * c), (2 * c, 2 * c), (2 * c, 4 * c), (4 * c, 4 * c)]):
        spec += [("features.%d.weight" % (3 * i), (cout, cin, 3, 3)), ("features.%d.running_mean" % (3 * i + 1), (cout,)),
                 ("features.%d.running_var" % (3 * i + 1), (cout,))]
    if kind == "hardnet":
        spec += [("features.19.weight", (128, 128, 8, 8)), ("features.20.running_mean", (128,)), ("features.20.running_var", (128,))]
    else:
        spec += [("features.19.weight", (NET_DIMS[kind], 64, 8, 8)), ("features.19.bias", (NET_DIMS[kind],))]
    return spec


def net_tensors(kind, state):
    """The arrays of `state` (name -> array) in network order as contiguous float32, after checking that none is missing, surplus or
    wrongly shaped (BatchNorm's num_batches_tracked counters of a PyTorch state dict are not tensors of the network and are ignored)."""
    spec = net_tensor_spec(kind)
    have = {k: v for k, v in dict(state).items() if not k.endswith("num_batches_tracked")}
    missing = [n for n, _ in spec if n not in have]
    if missing:
        raise ModsError("%s: missing tensors: %s" % (kind, ", ".join(missing)))
    surplus = sorted(set(have) - {n for n, _ in spec})
    if surplus:
        raise ModsError("%s: tensors the network does not have: %s" % (kind, ", ".join(surplus)))
    out = []
    for n, shape in spec:
        a = have[n]
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        if tuple(a.shape) != shape:
            raise ModsError("%s: tensor %s has shape %s, %s expected" % (kind, n, tuple(a.shape), shape))
        out.append(np.ascontiguousarray(a, np.float32))
    return out


def _slot_check(slot, net):
    if net is not None and getattr(net, "kind", None) != _NET_SLOTS[slot]:
        raise ModsError("the built-in %s slot takes a Net of kind %r, not %r" % (slot, _NET_SLOTS[slot], getattr(net, "kind", None)))


def net_chunk():
    """patches one set of launches of a Net takes; a longer list is cut into chunks of this size"""
    return int(lib().mods_net_chunk())


class Net:
    """AffNet / OriNet / HardNet as HIP kernels (mods_net_*): kind "affnet" | "orinet" | "hardnet", state = the tensors by the
    names of the daemon's state dict.  Immutable; several contexts and threads may use one Net.
    precision "fp32" (the default) | "bf16": the bf16 mode runs the convolutions behind the first and HardNet's head on the matrix
    cores with bf16 operands and fp32 accumulators (the contract is in include/mods_hip.h); its outputs differ from fp32's."""

    def __init__(self, kind, state, device=0, precision="fp32"):
        self.h = C.c_void_p()
        tensors = net_tensors(kind, state)                     # raises before any device call
        if precision not in NET_PRECISIONS:
            raise ModsError("Net: precision %r, one of %s expected" % (precision, " | ".join(map(repr, NET_PRECISIONS))))
        self.kind, self.dim, self.device, self.precision = kind, NET_DIMS[kind], device, precision
        ptrs = (C.POINTER(C.c_float) * len(tensors))(*[_fp(t) for t in tensors])
        sizes = (C.c_size_t * len(tensors))(*[t.size for t in tensors])
        _check(lib().mods_net_create_ex(device, NET_KINDS[kind], ptrs, sizes, len(tensors), NET_PRECISIONS[precision], C.byref(self.h)))

    def forward(self, patches, quantise=True):
        """patches [n][32][32] (values 0..255) -> float32 [n][dim]; quantise: round to 8 bits first, as the wire to a daemon does."""
        p = np.ascontiguousarray(patches, np.float32)
        if p.ndim == 4 and p.shape[1] == 1:
            p = p[:, 0]
        if p.ndim != 3 or p.shape[1:] != (32, 32):
            raise ModsError("Net.forward: patches of shape %s, [n][32][32] expected" % (tuple(p.shape),))
        p = np.ascontiguousarray(p)
        out = np.zeros((len(p), self.dim), np.float32)
        _check(lib().mods_net_forward(self.h, _fp(p), len(p), 1 if quantise else 0, _fp(out)))
        return out

    def forward_dev(self, stream, patches_ptr, n, out_ptr, quantise=True):
        """device pointers ([n][32][32] fp32 in, [n][dim] fp32 out) on hipStream_t `stream` (an integer address); does not wait"""
        _check(lib().mods_net_forward_dev(self.h, C.c_void_p(stream), C.c_void_p(patches_ptr), n, 1 if quantise else 0, C.c_void_p(out_ptr)))

    def stage_times(self, stream, patches_ptr, n, out_ptr, quantise=True):
        """forward_dev with device events between the launches (mods_test_net_stage_times); waits; milliseconds of stages 0..7"""
        ms = np.zeros(8, np.float32)
        _check(lib().mods_test_net_stage_times(self.h, C.c_void_p(stream), C.c_void_p(patches_ptr), n, 1 if quantise else 0, C.c_void_p(out_ptr), _fp(ms)))
        return ms

    def stage_shapes(self, stage):
        """per-patch shapes (input, output) of stage 0 (normalisation), 1..6 (convolution blocks), 7 (head)"""
        c = 32 if self.kind == "hardnet" else 16
        maps = [(1, 32), (c, 32), (c, 32), (2 * c, 16), (2 * c, 16), (4 * c, 8), (4 * c, 8)]       # between the stages
        if stage not in range(8):
            raise ModsError("Net.stage: stage %r, 0..7 expected" % (stage,))
        i = maps[max(stage - 1, 0)]
        return (i[0], i[1], i[1]), ((self.dim,) if stage == 7 else (maps[stage][0], maps[stage][1], maps[stage][1]))

    def stage(self, stage, x, quantise=False):
        """One stage alone (mods_test_net_stage; self-test hook): x = n <= net_chunk() patches with the elements of the stage's
        input each -> (float32 [n] + output shape, guard_ok); guard_ok: nothing was written behind the n-th patch's output."""
        shape_in, shape_out = self.stage_shapes(stage)
        x = np.ascontiguousarray(x, np.float32)
        n = len(x)
        if n < 1 or n > net_chunk() or x.size != n * int(np.prod(shape_in)):
            raise ModsError("Net.stage: input of shape %s, [n <= %d] + %s expected" % (tuple(x.shape), net_chunk(), shape_in))
        out = np.zeros((n,) + shape_out, np.float32)
        ok = C.c_int(0)
        _check(lib().mods_test_net_stage(self.h, int(stage), _fp(x), n, 1 if quantise else 0, _fp(out), C.byref(ok)))
        return out, bool(ok.value)

    def close(self):
        if self.h:
            lib().mods_net_destroy.restype = None
            lib().mods_net_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, device=0, max_w=1920, max_h=1080, batch=1, nonblocking=False):
        self.h = C.c_void_p()
        if nonblocking:     # a stream without implicit ordering after the default stream (what the pipeline's workers use)
            _check(lib().mods_ctx_create_ex(device, max_w, max_h, batch, 1, C.byref(self.h)))
        else:
            _check(lib().mods_ctx_create(device, max_w, max_h, batch, C.byref(self.h)))
        self.batch = batch
        self.device = device

    def close(self):
        if self.h:
            lib().mods_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(lib().mods_ctx_sync(self.h))

    @property
    def stream(self):
        return lib().mods_ctx_stream(self.h)

    # ---- timing
    def timing_enable(self, stages):
        mask = 0
        for s in stages:
            mask |= 1 << stage_index(s)
        _check(lib().mods_ctx_timing_enable(self.h, mask))

    def timing_read(self, stage):
        ms, n, by = C.c_double(), C.c_int(), C.c_double()
        _check(lib().mods_ctx_timing_read(self.h, stage_index(stage), C.byref(ms), C.byref(n), C.byref(by)))
        return ms.value, n.value, by.value

    def baumberg_stats_enable(self, on=True):
        """count the keypoints that enter the Baumberg iteration and the iterations they run (mods_baumberg_stats)"""
        _check(lib().mods_baumberg_stats_enable(self.h, 1 if on else 0))

    def baumberg_stats(self, img):
        kp, it = C.c_ulonglong(), C.c_ulonglong()
        _check(lib().mods_baumberg_stats(self.h, img, C.byref(kp), C.byref(it)))
        return kp.value, it.value

    # ---- detection masks (include/mods_hip.h, "detection masks")
    def set_detection_mask(self, image, mask):
        """mask: a 2-D uint8 array of the image's size (0 = no regions here), copied into the context; rows may be strided (a
        column slice of a wider array); None clears the mask of that image of a call"""
        if mask is None:
            _check(lib().mods_ctx_detection_mask(self.h, int(image), None, 0, 0, 0))
            return
        m, stride = _mask_rows(mask)
        _check(lib().mods_ctx_detection_mask(self.h, int(image), _vp(m), m.shape[1], m.shape[0], stride))

    def set_detection_mask_dev(self, image, dev_ptr, w, h, stride=None):
        """the same for a mask in device memory, which the context borrows: it must stay valid while set (0 / None clears)"""
        _check(lib().mods_ctx_detection_mask_dev(self.h, int(image), C.c_void_p(dev_ptr or 0), w, h, stride or w))

    def clear_detection_masks(self):
        _check(lib().mods_ctx_detection_masks_clear(self.h))

    def detection_mask_counts(self, image):
        """(entries of that image that reached the gate in the last call, entries it kept); (-1, -1) when the image had no mask"""
        a, k = C.c_int(), C.c_int()
        _check(lib().mods_ctx_detection_mask_counts(self.h, int(image), C.byref(a), C.byref(k)))
        return a.value, k.value

    def graphs(self, on=True):
        """replay the launches of detect + describe as a hipGraph from the second call with the same arguments on"""
        _check(lib().mods_ctx_graphs(self.h, 1 if on else 0))

    def graph_replays(self):
        lib().mods_ctx_graph_replays.restype = C.c_long
        return int(lib().mods_ctx_graph_replays(self.h))

    def pyramid_streams(self, n):
        _check(lib().mods_ctx_pyramid_streams(self.h, int(n)))

    def timing_reset(self):
        _check(lib().mods_ctx_timing_reset(self.h))

    # ---- primitives (host arrays)
    def gauss_blur(self, img, sigma):
        a = np.ascontiguousarray(img, np.float32)
        out = np.empty_like(a)
        _check(lib().mods_gauss_blur(self.h, _fp(a), a.shape[1], a.shape[0], C.c_float(sigma), _fp(out)))
        return out

    def hessian_response(self, img, norm):
        a = np.ascontiguousarray(img, np.float32)
        out = np.empty_like(a)
        _check(lib().mods_hessian_response(self.h, _fp(a), a.shape[1], a.shape[0], C.c_float(norm), _fp(out)))
        return out

    def resize_half(self, img):
        a = np.ascontiguousarray(img, np.float32)
        out = np.empty(((a.shape[0] + 1) // 2 + 1, (a.shape[1] + 1) // 2 + 1), np.float32).ravel()
        dw, dh = C.c_int(), C.c_int()
        _check(lib().mods_resize_half(self.h, _fp(a), a.shape[1], a.shape[0], _fp(out), C.byref(dw), C.byref(dh)))
        return out[:dw.value * dh.value].reshape(dh.value, dw.value).copy()

    def upscale2x(self, img):
        """mods_upscale2x: double_image of the contract in mods_hip.h (restated in tests/upscale_ref.py), h x w -> 2h x 2w"""
        a = np.ascontiguousarray(img, np.float32)
        out = np.empty((2 * a.shape[0], 2 * a.shape[1]), np.float32)
        _check(lib().mods_upscale2x(self.h, _fp(a), a.shape[1], a.shape[0], _fp(out)))
        return out

    # ---- detector
    def detect_hessian_affine(self, img, params=None, max_out=1 << 18):
        params = params or HessAffParams.default()
        a = np.ascontiguousarray(img, np.float32)
        out = np.zeros(max_out, AFFKEY_DTYPE)
        n = C.c_int()
        _check(lib().mods_detect_hessian_affine(self.h, _fp(a), a.shape[1], a.shape[0], a.shape[1], C.byref(params),
                                                out.ctypes.data_as(C.c_void_p), max_out, C.byref(n)))
        return out[:n.value].copy()

    def detect_hessian_affine_dev(self, dev_ptr, n_img, w, h, params=None, max_out=1 << 18, fetch=True):
        """dev_ptr: device address of [n_img][h][w] fp32 (e.g. torch tensor .data_ptr())."""
        params = params or HessAffParams.default()
        counts = (C.c_int * n_img)()
        out = np.zeros((n_img, max_out), AFFKEY_DTYPE) if fetch else None
        _check(lib().mods_detect_hessian_affine_dev(self.h, C.c_void_p(dev_ptr), n_img, w, h, w, C.byref(params),
                                                    out.ctypes.data_as(C.c_void_p) if fetch else None, max_out, counts))
        if fetch:
            return [out[i, :counts[i]].copy() for i in range(n_img)]
        return list(counts)

    # ---- introspection for parity tests
    def pyramid_octaves(self):
        return lib().mods_pyramid_octaves(self.h)

    def pyramid_dims(self, o):
        w, h = C.c_int(), C.c_int()
        _check(lib().mods_pyramid_dims(self.h, o, C.byref(w), C.byref(h)))
        return w.value, h.value

    def pyramid_plane(self, img, o, level, kind):
        w, h = self.pyramid_dims(o)
        out = np.empty((h, w), np.float32)
        _check(lib().mods_pyramid_plane(self.h, img, o, level, kind, _fp(out)))
        return out

    def pyramid_candidates(self, img=0, max_out=1 << 20):
        out = np.zeros(max_out, CAND_DTYPE)
        n = C.c_int()
        _check(lib().mods_pyramid_candidates(self.h, img, out.ctypes.data_as(C.c_void_p), max_out, C.byref(n)))
        return out[:n.value].copy()

    def pyramid_nms_hits(self, img=0, max_out=1 << 22):
        """(hits[n, 4] int32 rows (octave, level, r0, c0), count): the raw NMS hit list of the last detection in list (arbitrary)
        order; count is the device's counter, n = min(count, the list's capacity) - they differ after "NMS hit list overflow"."""
        n = C.c_int()
        rc = lib().mods_pyramid_nms_hits(self.h, img, None, 0, C.byref(n))      # the count alone (E_CAPACITY: there are records)
        if rc not in (MODS_OK, -3):                                               # -3: MODS_E_CAPACITY
            _check(rc)
        out = np.full((min(max(n.value, 0), max_out), 4), -1, np.int32)         # the call fills the list's capacity at the most
        _check(lib().mods_pyramid_nms_hits(self.h, img, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
        return out[:int(np.count_nonzero(out[:, 1] >= 0))].copy(), n.value
    def orient_describe(self, img, keys, params=None, max_out=None):
        params = params or DescribeParams.default()
        a = np.ascontiguousarray(img, np.float32)
        k = np.ascontiguousarray(keys)
        max_out = max_out or len(k) + 1
        out = np.zeros(max_out, REGION_DTYPE)
        n = C.c_int()
        _check(lib().mods_orient_describe(self.h, _fp(a), a.shape[1], a.shape[0], a.shape[1], k.ctypes.data_as(C.c_void_p),
                                          len(k), C.byref(params), out.ctypes.data_as(C.c_void_p), max_out, C.byref(n)))
        return out[:n.value].copy()

    def orient_describe_u8(self, img_u8, keys, params=None, max_out=None):
        """orient_describe for an 8-bit grey image [h][w] (any row stride: a view with padded rows is passed as it is): the same
        regions, sampled from the 8-bit image in the kernels set_u8_kernels selects."""
        params = params or DescribeParams.default()
        a = np.asarray(img_u8)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("orient_describe_u8 takes a 2-d uint8 array")
        if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a)
        k = np.ascontiguousarray(keys)
        max_out = max_out or len(k) + 1
        out = np.zeros(max_out, REGION_DTYPE)
        n = C.c_int()
        _check(lib().mods_orient_describe_u8(self.h, C.c_void_p(a.ctypes.data), a.shape[1], a.shape[0], a.strides[0],
                                             k.ctypes.data_as(C.c_void_p), len(k), C.byref(params), out.ctypes.data_as(C.c_void_p),
                                             max_out, C.byref(n)))
        return out[:n.value].copy()

    def regions_fetch_half(self, img=0, max_out=1 << 18):
        """HalfRootSIFT twins of the regions of image slot img (desc[:64]; describe with DescribeParams.halfDesc = 1)."""
        out = np.zeros(max_out, REGION_DTYPE)
        n = C.c_int()
        _check(lib().mods_regions_fetch_half(self.h, img, out.ctypes.data_as(C.c_void_p), max_out, C.byref(n)))
        return out[:n.value].copy()

    def detect_describe_dev(self, dev_ptr, n_img, w, h, det=None, desc=None):
        det = det or HessAffParams.default()
        desc = desc or DescribeParams.default()
        nd, nr = (C.c_int * n_img)(), (C.c_int * n_img)()
        _check(lib().mods_detect_describe_dev(self.h, C.c_void_p(dev_ptr), n_img, w, h, w, C.byref(det), C.byref(desc), nd, nr))
        return list(nd), list(nr)

    def u8_source_calls(self):
        lib().mods_ctx_u8_source_calls.restype = C.c_long
        return int(lib().mods_ctx_u8_source_calls(self.h))

    def set_u8_kernels(self, mask):
        """bit 0 orient, 1 extract_small, 2 big_fused, 3 big_sample sample from the 8-bit images in detect_describe_dev_u8, bits 4 - 7:
        the same four from the strip copy of those images (it goes first); -1: default"""
        _check(lib().mods_ctx_u8_kernels(self.h, int(mask)))

    def u8_strip_calls(self):
        """calls so far whose 8-bit images were laid out in strips as well (a kernel of the mask samples from them)"""
        lib().mods_ctx_u8_strip_calls.restype = C.c_long
        return int(lib().mods_ctx_u8_strip_calls(self.h))

    def u8_strips_fetch(self, batch_u8, src_offset=0):
        """the strip copy (u8_strips_layout) of a packed uint8 batch [n][h][w] as the conversion launch makes it on the device, the batch
        staged src_offset bytes into the staging area: uint8 [n][n_strips][strip_pitch // 16][16]"""
        a = np.ascontiguousarray(batch_u8, np.uint8)
        n, h, w = a.shape
        _, ns, pitch, nbytes = u8_strips_layout(w, h)
        out = np.zeros(n * nbytes, np.uint8)
        _check(lib().mods_u8_strips_fetch(self.h, C.c_void_p(a.ctypes.data), n, w, h, int(src_offset), C.c_void_p(out.ctypes.data)))
        return out.reshape(n, ns, pitch // 16, 16)

    def set_match_mutual(self, mode):
        """mods_ctx_match_mutual: 0 off, 1 every FGINN tentative must be its train's nearest query, 2 and pass the ratio test backwards"""
        _check(lib().mods_ctx_match_mutual(self.h, int(mode)))

    def set_local_affine(self, params=None):
        """mods_ctx_local_affine: a LocalAffineParams switches the filter on for every list of the context that goes to the
        verification, None switches it off (the default)"""
        _check(lib().mods_ctx_local_affine(self.h, C.byref(params) if params is not None else None))

    def local_affine_counts(self):
        """(tentatives in, tentatives kept) of the last list the local affine filter saw on this context"""
        ni, nk = C.c_int(), C.c_int()
        _check(lib().mods_local_affine_counts(self.h, C.byref(ni), C.byref(nk)))
        return ni.value, nk.value

    def filter_local_affine(self, tent, u6, laf, params=None):
        """mods_filter_local_affine on copies of the three arrays: returns (tent, u6, laf) of the survivors in list order and a dict
        of the per-input diagnostics keep (bool), neighbours, support, backed (int32)"""
        return filter_local_affine(self, tent, u6, laf, params)

    def set_distractor_db(self, full=None, half=None):
        """mods_ctx_distractor_db: the DescDB every FGINN search of whole descriptors is vetoed by, and the one the ladder's
        HalfRootSIFT searches take; None detaches a slot.  The context keeps a reference to what it holds."""
        _check(lib().mods_ctx_distractor_db(self.h, full.h if full is not None else None, half.h if half is not None else None))
        self._distractor = (full, half)

    def distractor_counts(self):
        """(forward tentatives, tentatives the distractor databases kept) of the context's last single search"""
        nf, nk = C.c_int(), C.c_int()
        _check(lib().mods_distractor_counts(self.h, C.byref(nf), C.byref(nk)))
        return nf.value, nk.value

    def distractor_fetch(self, cap=None):
        """mods_distractor_fetch: dDB of the last single search's survivors, in list order (empty when it was not vetoed)"""
        cap = self.distractor_counts()[1] if cap is None else cap
        out = np.zeros(max(cap, 1), np.int32)
        n = C.c_int()
        _check(lib().mods_distractor_fetch(self.h, _vp(out), int(cap), C.byref(n)))
        return out[:n.value].copy()

    def descdb_splits(self, n):
        """mods_ctx_descdb_splits: database splits of the distractor sweep (0 = automatic); the result does not depend on it."""
        _check(lib().mods_ctx_descdb_splits(self.h, int(n)))

    def match_mutual_counts(self):
        """(forward tentatives, tentatives the mutual check kept) of the context's last single search"""
        nf, nk = C.c_int(), C.c_int()
        _check(lib().mods_match_mutual_counts(self.h, C.byref(nf), C.byref(nk)))
        return nf.value, nk.value

    def set_domain_pooling(self, num_scales, start_coef=0.5, end_coef=1.5):
        """mods_ctx_domain_pooling (DSP-SIFT): the raw SIFT histograms of num_scales (2 .. 8) domains desc_mrSize * c_k, c_k from
        start_coef to end_coef in equal steps, are summed before the normalisation; num_scales 0 or 1: off"""
        _check(lib().mods_ctx_domain_pooling(self.h, int(num_scales), C.c_double(start_coef), C.c_double(end_coef)))

    def domain_pooling(self):
        """(num_scales, start_coef, end_coef) of the context; (0, 0.0, 0.0) when pooling is off"""
        k, a, b = C.c_int(), C.c_double(), C.c_double()
        _check(lib().mods_ctx_domain_pooling_get(self.h, C.byref(k), C.byref(a), C.byref(b)))
        return k.value, a.value, b.value

    def spatial_selection(self, mode=1, robustness=0.9):
        """mods_ctx_spatial_selection (ANMS): the count modes keep the keys with the largest suppression radius instead of the
        strongest ones; mode 0 off, 1 on, 2 on for the calls it covers and off for the others"""
        _check(lib().mods_ctx_spatial_selection(self.h, int(mode), C.c_double(robustness)))

    def upscale_input(self, mode=1):
        """mods_ctx_upscale_input: the scale-space detectors start at the doubled image (pixel distance 0.5, assumed blur 1.0);
        mode 0 off, 1 on, 2 on with the first level made in two launches (what mode 1 is tested against)"""
        _check(lib().mods_ctx_upscale_input(self.h, int(mode)))

    def upscale_input_get(self):
        m = C.c_int()
        _check(lib().mods_ctx_upscale_input_get(self.h, C.byref(m)))
        return m.value

    def spatial_selection_get(self):
        """(mode, robustness) of the context"""
        m, r = C.c_int(), C.c_double()
        _check(lib().mods_ctx_spatial_selection_get(self.h, C.byref(m), C.byref(r)))
        return m.value, r.value

    def test_spatial_select(self, lists, keep, robustness=0.9):
        """mods_test_spatial_select: sorted AFFKEY_DTYPE lists (one per image slot) and their keep counts through the launches of a
        detect call; returns the selected indices of every list"""
        n_img = len(lists)
        max_n = max(1, max(len(k) for k in lists))
        keys = np.zeros((n_img, max_n), AFFKEY_DTYPE)
        for b, k in enumerate(lists):
            keys[b, :len(k)] = k
        n = (C.c_int * n_img)(*[len(k) for k in lists])
        kp = (C.c_int * n_img)(*[int(v) for v in keep])
        idx = np.full((n_img, max_n), -1, np.int32)
        n_out = (C.c_int * n_img)()
        _check(lib().mods_test_spatial_select(self.h, _vp(keys), n_img, n, max_n, kp, C.c_double(robustness), _vp(idx), n_out))
        return [idx[b, :n_out[b]].copy() for b in range(n_img)]

    def detect_describe_dev_u8(self, dev_ptr, n_img, w, h, det=None, desc=None, stride=None):
        """detect_describe_dev for a batch of 8-bit grey images [n_img][h][stride] in HBM (stride in bytes, default w): the same regions,
        sampled from the 8-bit images where the rows are packed, from their fp32 copy otherwise."""
        det = det or HessAffParams.default()
        desc = desc or DescribeParams.default()
        nd, nr = (C.c_int * n_img)(), (C.c_int * n_img)()
        _check(lib().mods_detect_describe_dev_u8(self.h, C.c_void_p(dev_ptr), n_img, w, h, w if stride is None else int(stride),
                                                 C.byref(det), C.byref(desc), nd, nr))
        return list(nd), list(nr)

    def regions_fetch(self, img, max_out=1 << 18):
        n = C.c_int()
        _check(lib().mods_regions_fetch(self.h, img, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), REGION_DTYPE)
        _check(lib().mods_regions_fetch(self.h, img, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n)))
        return out[:n.value].copy()

    def set_external_descriptor(self, fn_ptr, user, mr_size=3.0 * np.sqrt(3.0), patch_size=32):
        """fn_ptr: address of a mods_descriptor_fn (e.g. mods_zmq_descriptor_hook of libmodszmq.so), user: its void* argument
        (keep the object it points to alive).  fn_ptr = None restores RootSIFT."""
        _check(lib().mods_ctx_set_external_descriptor(self.h, C.c_void_p(fn_ptr), C.c_void_p(user), C.c_double(mr_size), patch_size))

    def set_external_shape(self, fn_ptr, user, mr_size=3.0 * np.sqrt(3.0), patch_size=32):
        """AffNet in the place of Baumberg (detect with doBaumberg = 0): fn returns (a11, a21, a22) per patch.  None: off."""
        _check(lib().mods_ctx_set_external_shape(self.h, C.c_void_p(fn_ptr), C.c_void_p(user), C.c_double(mr_size), patch_size))

    def set_external_orientation(self, fn_ptr, user, mr_size=3.0 * np.sqrt(3.0), patch_size=32):
        """OriNet in the place of the dominant gradient orientation: fn returns (y, x) per patch.  None: off."""
        _check(lib().mods_ctx_set_external_orientation(self.h, C.c_void_p(fn_ptr), C.c_void_p(user), C.c_double(mr_size), patch_size))

    def set_builtin_shape(self, net, mr_size=3.0 * np.sqrt(3.0), quantise=True):
        """AffNet in-process (a Net of kind "affnet") in the place of Baumberg; clears an external shape function.  None: off."""
        _slot_check("shape", net)
        _check(lib().mods_ctx_set_builtin_shape(self.h, net.h if net is not None else None, C.c_double(mr_size), 1 if quantise else 0))
        self._nets = dict(getattr(self, "_nets", {}), shape=net)          # keeps the network alive while the context uses it

    def set_builtin_orientation(self, net, mr_size=3.0 * np.sqrt(3.0), quantise=True):
        """OriNet in-process (a Net of kind "orinet") in the place of the dominant gradient orientation.  None: off."""
        _slot_check("orientation", net)
        _check(lib().mods_ctx_set_builtin_orientation(self.h, net.h if net is not None else None, C.c_double(mr_size), 1 if quantise else 0))
        self._nets = dict(getattr(self, "_nets", {}), orientation=net)

    def set_builtin_descriptor(self, net, mr_size=3.0 * np.sqrt(3.0), quantise=True):
        """HardNet in-process (a Net of kind "hardnet") in the place of RootSIFT.  None: off."""
        _slot_check("descriptor", net)
        _check(lib().mods_ctx_set_builtin_descriptor(self.h, net.h if net is not None else None, C.c_double(mr_size), 1 if quantise else 0))
        self._nets = dict(getattr(self, "_nets", {}), descriptor=net)

    def patches_fetch(self, img, ps, max_regions=1 << 17):
        n = C.c_int()
        out = np.zeros((max_regions, ps, ps), np.float32) if max_regions <= 4096 else None
        if out is None:
            cnt = C.c_int()
            _check(lib().mods_regions_fetch(self.h, img, None, 0, C.byref(cnt)))
            out = np.zeros((max(cnt.value, 1), ps, ps), np.float32)
        _check(lib().mods_patches_fetch(self.h, img, ps, _fp(out), out.shape[0], C.byref(n)))
        return out[:n.value].copy()

    def regions_copy_dev(self, img, dst_ptr, n):
        """Device-to-device copy of the first n regions of image slot img (e.g. into a torch tensor)."""
        _check(lib().mods_regions_copy_dev(self.h, img, C.c_void_p(dst_ptr), n))

    def dominant_angle(self, patch, th=float(np.float32(0.8))):
        a = np.ascontiguousarray(patch, np.float32)
        ang, found = C.c_float(), C.c_int()
        _check(lib().mods_dominant_angle(self.h, _fp(a), a.shape[0], C.c_double(th), C.byref(ang), C.byref(found)))
        return bool(found.value), ang.value

    def selftest_fast_sqrt(self):
        """(differs inside the stated domain, differs for 0 < x < 2^-96, everywhere-exact form differs on a non-negative operand,
        operands visited, negative operands where either form differs)"""
        out = (C.c_ulonglong * 5)()
        _check(lib().mods_selftest_fast_sqrt(self.h, out))
        return tuple(int(v) for v in out)

    def sift_patch(self, patch, rootsift=True, max_bin=0.2):
        a = np.ascontiguousarray(patch, np.float32)
        out = np.zeros(128, np.uint8)
        _check(lib().mods_sift_patch(self.h, _fp(a), a.shape[0], int(rootsift), C.c_double(max_bin),
                                     out.ctypes.data_as(C.c_void_p)))
        return out

    def sift_pooled(self, patches, rootsift=True, half=False, photo_norm=False, max_bin=0.2):
        """mods_test_sift_pooled: patches [K][ps][ps] of one region through the accumulate and finish kernels of the pooled
        description; 128 bytes (half: the 64 HalfSIFT values, then zeros)"""
        a = np.ascontiguousarray(patches, np.float32)
        out = np.zeros(128, np.uint8)
        _check(lib().mods_test_sift_pooled(self.h, _fp(a), a.shape[0], a.shape[1], int(rootsift), int(half), int(photo_norm),
                                           C.c_double(max_bin), out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- view synthesis
    def warp_affine(self, img, M, dw, dh, cval=128.0):
        a = np.ascontiguousarray(img, np.float32)
        Mc = np.ascontiguousarray(M, np.float64).ravel()
        out = np.empty((dh, dw), np.float32)
        _check(lib().mods_warp_affine(self.h, _fp(a), a.shape[1], a.shape[0], Mc.ctypes.data_as(C.c_void_p), dw, dh,
                                      C.c_float(cval), _fp(out)))
        return out

    def gauss_blur_xy(self, img, kx, ky, sx, sy):
        a = np.ascontiguousarray(img, np.float32)
        out = np.empty_like(a)
        _check(lib().mods_gauss_blur_xy(self.h, _fp(a), a.shape[1], a.shape[0], kx, ky, C.c_double(sx), C.c_double(sy), _fp(out)))
        return out

    def synth_view_dev(self, src_ptr, w, h, geom, dst_ptr, do_blur=1):
        _check(lib().mods_synth_view_dev(self.h, C.c_void_p(src_ptr), w, h, w, C.byref(geom), do_blur, C.c_void_p(dst_ptr)))

    def detect_describe_view_dev(self, src_ptr, w, h, tilt, phi, zoom=1.0, init_sigma=0.2, do_blur=1, det=None, desc=None):
        """One synthesised view of the w x h image at src_ptr (HBM): returns (geom, n_detected, n_regions); the
        regions (original frame) stay in the context (regions_fetch(0))."""
        det = det or HessAffParams.default()
        desc = desc or DescribeParams.default()
        g = ViewGeom()
        nd, nr = C.c_int(), C.c_int()
        _check(lib().mods_detect_describe_view_dev(self.h, C.c_void_p(src_ptr), w, h, w, C.c_double(tilt), C.c_double(phi),
                                                   C.c_double(zoom), C.c_double(init_sigma), do_blur, C.byref(det),
                                                   C.byref(desc), C.byref(g), C.byref(nd), C.byref(nr)))
        return g, nd.value, nr.value

    # ---- homography views (include/mods_hip.h, "homography views")
    def warp_perspective(self, img, H, dw, dh, cval=128.0, stride=None):
        """mods_warp_perspective: img (h x w) through H (original -> view) into dh x dw.  stride: the warp reads the first w columns
        of img's rows, which then are `stride` floats apart (mods_test_warp_perspective_strided)"""
        a = np.ascontiguousarray(img, np.float32)
        Hc = np.ascontiguousarray(H, np.float64).ravel()
        out = np.empty((dh, dw), np.float32)
        if stride is None:
            _check(lib().mods_warp_perspective(self.h, _fp(a), a.shape[1], a.shape[0], _vp(Hc), dw, dh, C.c_float(cval), _fp(out)))
        else:
            w = a.shape[1]
            padded = np.full((a.shape[0], stride), np.float32(np.nan), np.float32)   # the gap is never read
            padded[:, :w] = a
            _check(lib().mods_test_warp_perspective_strided(self.h, _fp(padded), w, a.shape[0], stride, _vp(Hc), dw, dh, C.c_float(cval),
                                                            _fp(out)))
        return out

    def synth_view_h_dev(self, src_ptr, w, h, geom, dst_ptr, do_blur=1, stride=None):
        _check(lib().mods_synth_view_h_dev(self.h, C.c_void_p(src_ptr), w, h, stride or w, C.byref(geom), do_blur, C.c_void_p(dst_ptr)))

    def detect_describe_view_h_dev(self, src_ptr, w, h, H, clip_w=None, clip_h=None, init_sigma=0.2, do_blur=1, det=None, desc=None,
                                   stride=None):
        """One homography view of the w x h image at src_ptr (HBM): returns (geom, n_detected, n_regions); the regions (original
        frame) stay in slot 0 of the context (regions_fetch(0))."""
        det = det or HessAffParams.default()
        desc = desc or DescribeParams.default()
        Hc = np.ascontiguousarray(H, np.float64).ravel()
        g = ViewGeom()
        nd, nr = C.c_int(), C.c_int()
        _check(lib().mods_detect_describe_view_h_dev(self.h, C.c_void_p(src_ptr), w, h, stride or w, _vp(Hc), clip_w or w, clip_h or h,
                                                     C.c_double(init_sigma), do_blur, C.byref(det), C.byref(desc), C.byref(g),
                                                     C.byref(nd), C.byref(nr)))
        return g, nd.value, nr.value

    def reproject_regions_h(self, regions, H, ow, oh, half=None):
        """mods_test_reproject_regions_h: the post-pass of a homography view over host regions (REGION_DTYPE, view frame) and
        optionally their HalfRootSIFT twins; returns the survivors in the original frame (and the twins' survivors when given)"""
        r = np.ascontiguousarray(regions, REGION_DTYPE).copy()
        hh = None if half is None else np.ascontiguousarray(half, REGION_DTYPE).copy()
        Hc = np.ascontiguousarray(H, np.float64).ravel()
        n = C.c_int()
        _check(lib().mods_test_reproject_regions_h(self.h, _vp(Hc), ow, oh, _vp(r) if len(r) else None,
                                                   _vp(hh) if hh is not None and len(hh) else None, len(r), C.byref(n)))
        return (r[:n.value].copy(), hh[:n.value].copy()) if hh is not None else r[:n.value].copy()

    def view_pixels(self, geom):
        """Host copy of the last synthesised view."""
        out = np.empty((geom.h_new, geom.w_new), np.float32)
        _check(lib().mods_view_fetch(self.h, C.byref(geom), _fp(out)))
        return out

    # ---- matching
    def match_fginn(self, q, t, ratio=0.8, contrad=10.0, nn=50):
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        cap = max(len(q), 1)
        tent, u6, self.last_laf = _tentatives(cap, lambda out, u6, laf, n: lib().mods_match_fginn(
            self.h, _vp(q), len(q), _vp(t), len(t), C.c_double(ratio), C.c_double(contrad), nn, out, u6, laf, cap, n))
        return tent, u6

    def match_distance(self, q, t, threshold):
        """MatchFLANNDistance (matching.cpp:572-633): nearest train by Hamming distance, kept within the threshold."""
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        cap = max(len(q), 1)
        return _tentatives(cap, lambda out, u6, laf, n: lib().mods_match_distance(
            self.h, _vp(q), len(q), _vp(t), len(t), C.c_double(threshold), out, u6, laf, cap, n))[:2]

    def match_guided(self, q, t, params):
        """mods_match_guided: the model-guided search of two host region lists (GuidedParams); returns (tent, u6, laf)."""
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        cap = max(len(q), 1)
        return _tentatives(cap, lambda out, u6, laf, n: lib().mods_match_guided(
            self.h, _vp(q), len(q), _vp(t), len(t), C.byref(params), out, u6, laf, cap, n))

    def match_overlap(self, q, t, params):
        """mods_match_overlap: ground-truth overlap matching of two host region lists (OverlapParams); returns (matches as
        OVERLAP_DTYPE rows in query order, OverlapCounts)."""
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        return _overlap(lib().mods_match_overlap, OVERLAP_DTYPE, (self.h, _vp(q), len(q), _vp(t), len(t)), params, max(len(q), 1))

    def match_overlap_area(self, q, t, params):
        """mods_match_overlap_area: area-overlap matching (1 - intersection over union on the lattice) of two host region lists
        (OverlapAreaParams); returns (matches as OVERLAP_AREA_DTYPE rows in query order, OverlapCounts)."""
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        return _overlap(lib().mods_match_overlap_area, OVERLAP_AREA_DTYPE, (self.h, _vp(q), len(q), _vp(t), len(t)), params,
                        max(len(q), 1))

    def overlap_splits(self, splits):
        """mods_ctx_overlap_splits: train splits of the overlap sweeps (0 = automatic); the result does not depend on it."""
        _check(lib().mods_ctx_overlap_splits(self.h, int(splits)))

    def match_knn(self, q, t, k):
        """mods_match_knn: the k nearest trains of every query of two host region lists, by exact squared L2 distance over the
        descriptor bytes, ties to the lower index; returns (dist[n_q, k] int32, index[n_q, k] int32), rows in (d, index) order,
        padded with (INT_MAX, -1) where the train list is shorter than k."""
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        return _knn_rows(len(q), k, lambda idx, d2: lib().mods_match_knn(self.h, _vp(q) if len(q) else None, len(q),
                                                                         _vp(t) if len(t) else None, len(t), int(k), idx, d2))

    def match_knn_dev(self, img_q, img_t, k):
        """mods_match_knn_dev: the same on the region lists of images img_q / img_t that the last detect_describe_dev left in HBM."""
        n = C.c_int()
        _check(lib().mods_regions_fetch(self.h, int(img_q), None, 0, C.byref(n)))
        return _knn_rows(n.value, k, lambda idx, d2: lib().mods_match_knn_dev(self.h, int(img_q), int(img_t), int(k), idx, d2))

    def match_knn_reps(self, rep_q, rep_t, k, q_begin=0, q_end=None):
        """mods_match_knn_reps: queries [q_begin, q_end) of ImgRep rep_q against all of ImgRep rep_t; rows are relative to q_begin,
        indices refer to the full bank."""
        q_end = len(rep_q) if q_end is None else q_end
        return _knn_rows(max(q_end - q_begin, 0), k, lambda idx, d2: lib().mods_match_knn_reps(
            self.h, rep_q.h, int(q_begin), int(q_end), rep_t.h, int(k), idx, d2))

    def knn_splits(self, n):
        """mods_ctx_knn_splits: train splits of the k-NN sweep (0 = automatic); the result does not depend on it."""
        _check(lib().mods_ctx_knn_splits(self.h, int(n)))

    def clahe(self, img_u8, clip_limit=4.0, tiles=(8, 8)):
        """mods_clahe: CLAHE of one 8-bit grey image [h, w] (host in, host out); tiles = (tiles_x, tiles_y)"""
        a = np.ascontiguousarray(img_u8, np.uint8)
        h, w = a.shape
        out = np.empty_like(a)
        par = ClaheParams(clip_limit, tiles[0], tiles[1])
        _check(lib().mods_clahe(self.h, a.ctypes.data_as(C.c_void_p), w, h, C.byref(par), out.ctypes.data_as(C.c_void_p)))
        return out

    def clahe_dev(self, src_ptr, n_img, w, h, dst_ptr, clip_limit=4.0, tiles=(8, 8), f32=True, src_stride=None, dst_stride=None):
        """mods_clahe_dev: n_img 8-bit images [n_img][h][src_stride] in HBM -> [n_img][h][dst_stride] fp32 (f32) or u8 in HBM;
        complete on return"""
        par = ClaheParams(clip_limit, tiles[0], tiles[1])
        _check(lib().mods_clahe_dev(self.h, C.c_void_p(src_ptr), n_img, w, h, src_stride or w, C.byref(par), C.c_void_p(dst_ptr),
                                    dst_stride or w, 1 if f32 else 0))

    def match_dev(self, img_q, img_t, ratio=0.8, contrad=10.0, nn=50, cap=1 << 18):
        out = np.zeros(cap, TENT_DTYPE)
        u6 = np.zeros((cap, 6), np.float64)
        laf = np.zeros((cap, 14), np.float64)
        n = C.c_int()
        _check(lib().mods_match_dev(self.h, img_q, img_t, C.c_double(ratio), C.c_double(contrad), nn,
                                    out.ctypes.data_as(C.c_void_p), u6.ctypes.data_as(C.c_void_p),
                                    laf.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        self.last_laf = laf[:n.value].copy()
        return out[:n.value].copy(), u6[:n.value].copy()

    def refine_matches(self, img1, img2, laf, params=None):
        """mods_refine_matches: the rows laf[n][14] refined by affine least-squares matching between the host images img1 and
        img2 (2-D float32; rows may be strided).  Returns a dict: laf, u6, status, iterations, zncc_before, zncc_after"""
        a, sa = _f32_rows(img1)
        b, sb = _f32_rows(img2)
        return _refine(lib().mods_refine_matches, self, (_vp(a), a.shape[1], a.shape[0], sa, _vp(b), b.shape[1], b.shape[0], sb), laf, params)

    def refine_matches_dev(self, img1_ptr, w1, h1, stride1, img2_ptr, w2, h2, stride2, laf, params=None):
        """mods_refine_matches_dev: as refine_matches on two fp32 images in device memory (strides in floats)"""
        return _refine(lib().mods_refine_matches_dev, self, (C.c_void_p(img1_ptr), int(w1), int(h1), int(stride1), C.c_void_p(img2_ptr),
                                                             int(w2), int(h2), int(stride2)), laf, params)

    def propagate_matches(self, img1, img2, laf, params=None, max_out=None):
        """mods_propagate_matches: the seed rows laf[n][14] grown into quasi-dense correspondences by match propagation between the
        host images img1 and img2 (2-D float32; rows may be strided).  max_out: the most rows returned (default: one per cell).
        Returns a dict: laf, u6, zncc, iterations, round, cell, parent, truncated, seed_status, stats[rounds + 1][8],
        tried_status[Gy][Gx], tried_iterations[Gy][Gx]"""
        a, sa = _f32_rows(img1)
        b, sb = _f32_rows(img2)
        return _propagate(lib().mods_propagate_matches, self, (_vp(a), a.shape[1], a.shape[0], sa, _vp(b), b.shape[1], b.shape[0], sb), laf, params,
                          max_out)

    def propagate_matches_dev(self, img1_ptr, w1, h1, stride1, img2_ptr, w2, h2, stride2, laf, params=None, max_out=None):
        """mods_propagate_matches_dev: as propagate_matches on two fp32 images in device memory (strides in floats)"""
        return _propagate(lib().mods_propagate_matches_dev, self, (C.c_void_p(img1_ptr), int(w1), int(h1), int(stride1), C.c_void_p(img2_ptr),
                                                                   int(w2), int(h2), int(stride2)), laf, params, max_out)

    def verified_lafs(self):
        """mods_ctx_verified_lafs: the frames [n][14] (x y a11 a12 a21 a22 s of region 1, then of region 2) of the verified
        correspondences of the last pair / ladder / verify call, in the order of its matches"""
        return _verified_lafs(lib().mods_ctx_verified_lafs, self.h)


TENT_DTYPE =np.dtype([("q", "i4"), ("t", "i4"), ("t_bad", "i4"), ("t_2nd", "i4"), ("d1", "f4"), ("d2", "f4"),
                       ("d2nd", "f4"), ("pad", "f4"), ("ratio", "f8")])


def duplicate_filter(tent, u6, r=2.0, mode=1, laf=None):
    """Host-side DuplicateFiltering (matching.cpp:2615-2679) on (tentatives, correspondences[, frames])."""
    tent = np.ascontiguousarray(tent).copy()
    u6 = np.ascontiguousarray(u6, np.float64).copy()
    lf = np.ascontiguousarray(laf, np.float64).copy() if laf is not None else None
    n = C.c_int()
    _check(lib().mods_duplicate_filter(tent.ctypes.data_as(C.c_void_p), u6.ctypes.data_as(C.c_void_p),
                                       lf.ctypes.data_as(C.c_void_p) if lf is not None else None, len(tent),
                                       C.c_double(r), mode, C.byref(n)))
    if lf is not None:
        return tent[:n.value].copy(), u6[:n.value].copy(), lf[:n.value].copy()
    return tent[:n.value].copy(), u6[:n.value].copy()


def duplicate_filter_gpu(ctx, tent, u6, laf, r=2.0, mode=1):
    """DuplicateFiltering on the context's GPU (csrc/dedup.hip); returns (tent, u6, laf, on_device)."""
    tent = np.ascontiguousarray(tent).copy()
    u6 = np.ascontiguousarray(u6, np.float64).copy()
    lf = np.ascontiguousarray(laf, np.float64).copy()
    n, dev = C.c_int(), C.c_int()
    _check(lib().mods_duplicate_filter_gpu(ctx.h, tent.ctypes.data_as(C.c_void_p), u6.ctypes.data_as(C.c_void_p),
                                           lf.ctypes.data_as(C.c_void_p), len(tent), C.c_double(r), mode, C.byref(n), C.byref(dev)))
    return tent[:n.value].copy(), u6[:n.value].copy(), lf[:n.value].copy(), bool(dev.value)


class LocalAffineParams(C.Structure):
    """mods_local_affine_params (include/mods_hip.h): the local affine consistency filter of a tentative list"""
    _fields_ = [("radius", C.c_double), ("minDist", C.c_double), ("absTol", C.c_double), ("relTol", C.c_double),
                ("areaTol", C.c_double), ("minSupport", C.c_int), ("rescue", C.c_int), ("keepSparse", C.c_int)]

    @staticmethod
    def default(**kw):
        p = LocalAffineParams(160.0, 3.0, 4.0, 0.2, 2.0, 3, 1, 1)
        for k, v in kw.items():
            if k not in dict(LocalAffineParams._fields_):
                raise TypeError("LocalAffineParams has no field %r" % k)
            setattr(p, k, v)
        return p


class LsmParams(C.Structure):
    """mods_lsm_params (include/mods_hip.h): the least-squares refinement of correspondences"""
    _fields_ = [("radius", C.c_int), ("max_iter", C.c_int), ("eps_shift", C.c_double), ("max_shift", C.c_double),
                ("max_scale_change", C.c_double), ("max_magnification", C.c_double), ("min_zncc", C.c_double), ("lam", C.c_double),
                ("affine", C.c_int), ("pad", C.c_int)]


LSM_STATUS = ("OK", "MAXITER", "BAD_FRAME", "OUTSIDE", "FLAT", "DIVERGED", "LOW_ZNCC")


def lsm_defaults(**kw):
    """mods_lsm_defaults, with fields replaced by keyword (lam = the header's lambda)"""
    p = LsmParams()
    lib().mods_lsm_defaults.restype = None
    lib().mods_lsm_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(LsmParams._fields_):
            raise TypeError("LsmParams has no field %r" % k)
        setattr(p, k, v)
    return p


def _f32_rows(img):
    """a host image as the library takes it: (array that owns the pixels, row stride in floats)"""
    a = np.asarray(img)
    if a.dtype != np.float32 or a.ndim != 2 or a.size == 0:
        raise ValueError("an image is a non-empty 2-D float32 array")
    if a.strides[1] != 4 or a.strides[0] % 4 or a.strides[0] < 4 * a.shape[1]:
        a = np.ascontiguousarray(a)
    return a, a.strides[0] // 4


def _refine(fn, ctx, images, laf, params):
    lf = np.ascontiguousarray(laf, np.float64).reshape(-1, 14)
    n = len(lf)
    out, u6 = np.zeros((max(n, 1), 14)), np.zeros((max(n, 1), 6))
    st, it = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    zb, za = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    _check(fn(ctx.h if ctx is not None else None, *images, _vp(lf), n, C.byref(params) if params is not None else None,
              _vp(out), _vp(u6), _vp(st), _vp(it), _vp(zb), _vp(za)))
    return {"laf": out[:n], "u6": u6[:n], "status": st[:n], "iterations": it[:n], "zncc_before": zb[:n], "zncc_after": za[:n]}


class PropagateParams(C.Structure):
    """mods_propagate_params (include/mods_hip.h): match propagation from refined correspondences"""
    _fields_ = [("cell", C.c_int), ("reach", C.c_int), ("rounds", C.c_int), ("model_type", C.c_int), ("lsm", LsmParams),
                ("model", C.c_double * 9), ("model_thr", C.c_double)]


PROP_STATUS = LSM_STATUS + ("OFF_MODEL",)


def propagate_defaults(**kw):
    """mods_propagate_defaults, with fields replaced by keyword: cell, reach, rounds, model_type, model (9 values), model_thr, lsm
    (an LsmParams), or a field of LsmParams (radius, min_zncc, ...) for the nested structure"""
    p = PropagateParams()
    lib().mods_propagate_defaults.restype = None
    lib().mods_propagate_defaults(C.byref(p))
    own, nested = dict(PropagateParams._fields_), dict(LsmParams._fields_)
    for k, v in kw.items():
        if k == "model":
            p.model = (C.c_double * 9)(*[float(x) for x in np.asarray(v, np.float64).reshape(9)])
        elif k in own:
            setattr(p, k, v)
        elif k in nested:
            setattr(p.lsm, k, v)
        else:
            raise TypeError("PropagateParams has no field %r" % k)
    return p


def _propagate(fn, ctx, images, laf, params, max_out):
    lf = np.ascontiguousarray(laf, np.float64).reshape(-1, 14)
    n = len(lf)
    par = params if params is not None else propagate_defaults()
    w1, h1 = images[1], images[2]
    gx, gy = max(w1 // max(par.cell, 1), 1), max(h1 // max(par.cell, 1), 1)
    cap = gx * gy if max_out is None else int(max_out)
    room = max(cap, 1)
    out, u6, z = np.zeros((room, 14)), np.zeros((room, 6)), np.zeros(room)
    it, rnd, par_ = np.zeros(room, np.int32), np.zeros(room, np.int32), np.zeros(room, np.int32)
    cell = np.zeros((room, 2), np.int32)
    n_out, trunc = C.c_int(0), C.c_int(0)
    seed = np.zeros(max(n, 1), np.int32)
    stats = np.zeros((max(par.rounds, 0) + 1, len(PROP_STATUS)), np.int32)
    ts, ti = np.full((gy, gx), -1, np.int32), np.full((gy, gx), -1, np.int32)
    _check(fn(ctx.h if ctx is not None else None, *images, _vp(lf), n, C.byref(params) if params is not None else None, cap, _vp(out), _vp(u6),
              _vp(z), _vp(it), _vp(rnd), _vp(cell), _vp(par_), C.byref(n_out), C.byref(trunc), _vp(seed), _vp(stats), _vp(ts), _vp(ti)))
    m = n_out.value
    return {"laf": out[:m], "u6": u6[:m], "zncc": z[:m], "iterations": it[:m], "round": rnd[:m], "cell": cell[:m], "parent": par_[:m],
            "truncated": bool(trunc.value), "seed_status": seed[:n], "stats": stats, "tried_status": ts, "tried_iterations": ti}


def test_propagate_round(ctx, w1, h1, cell, reach, front_laf, front_cell=None, state=None):
    """mods_test_propagate_round: one proposal and list pass.  Returns (winner[Gy][Gx], key[Gy][Gx], cand_cell[n_cand],
    cand_laf[n_cand][14])"""
    f = np.ascontiguousarray(front_laf, np.float64).reshape(-1, 14)
    gx, gy = max(int(w1) // max(int(cell), 1), 1), max(int(h1) // max(int(cell), 1), 1)
    fc = np.ascontiguousarray(front_cell, np.int32).reshape(-1, 2) if front_cell is not None else None
    st = np.ascontiguousarray(state, np.uint8).reshape(gy, gx) if state is not None else None
    win, key = np.full((gy, gx), -1, np.int32), np.zeros((gy, gx), np.uint64)
    cc, cl = np.zeros(gx * gy, np.int32), np.zeros((gx * gy, 14))
    n = C.c_int(0)
    _check(lib().mods_test_propagate_round(ctx.h if ctx is not None else None, int(w1), int(h1), int(cell), int(reach), _vp(f),
                                           _vp(fc) if fc is not None else None, len(f), _vp(st) if st is not None else None, _vp(win), _vp(key),
                                           _vp(cc), _vp(cl), C.byref(n)))
    return win, key, cc[:n.value], cl[:n.value]


test_propagate_round.__test__ = False


def refit_model(u6, model_type):
    """mods_refit_model: the least-squares H (model_type 0, row-major, image 1 -> image 2) or F (1, as a pair result holds it) over
    all rows x1 y1 1 x2 y2 1; no device needed"""
    u = np.ascontiguousarray(u6, np.float64).reshape(-1, 6)
    out = np.zeros(9)
    _check(lib().mods_refit_model(_vp(u), len(u), int(model_type), _vp(out)))
    return out


def test_lsm_iteration(ctx, img1, img2, row, params=None):
    """mods_test_lsm_iteration: (N[6][6], g[6], a, delta[6], status) of the first iteration of one row through the kernel"""
    a, sa = _f32_rows(img1)
    b, sb = _f32_rows(img2)
    r = np.ascontiguousarray(row, np.float64).reshape(14)
    N, g, d = np.zeros((6, 6)), np.zeros(6), np.zeros(6)
    gain, st = C.c_double(), C.c_int()
    _check(lib().mods_test_lsm_iteration(ctx.h if ctx is not None else None, _vp(a), a.shape[1], a.shape[0], sa, _vp(b), b.shape[1],
                                         b.shape[0], sb, _vp(r), C.byref(params) if params is not None else None, _vp(N), _vp(g),
                                         C.byref(gain), _vp(d), C.byref(st)))
    return N, g, gain.value, d, st.value


test_lsm_iteration.__test__ = False


def local_affine_grid():
    """(rows of a sweep block, columns of an LDS tile) of csrc/local_affine.hip"""
    r, t = C.c_int(), C.c_int()
    lib().mods_local_affine_grid.restype = None
    lib().mods_local_affine_grid(C.byref(r), C.byref(t))
    return r.value, t.value


def filter_local_affine(ctx, tent, u6, laf, params=None):
    """mods_filter_local_affine; ctx: a Context (None reaches the argument checks only).  Returns (tent, u6, laf, diagnostics)."""
    tent = np.ascontiguousarray(tent, TENT_DTYPE).copy()
    u6 = np.ascontiguousarray(u6, np.float64).reshape(-1, 6).copy()
    lf = np.ascontiguousarray(laf, np.float64).reshape(-1, 14).copy()
    n = len(tent)
    if len(u6) != n or len(lf) != n:
        raise ValueError("filter_local_affine: %d tentatives, %d correspondences, %d frames" % (n, len(u6), len(lf)))
    par = params if params is not None else LocalAffineParams.default()
    keep = np.zeros(max(n, 1), np.uint8)
    nb, sup, back = (np.zeros(max(n, 1), np.int32) for _ in range(3))
    m = C.c_int()
    _check(lib().mods_filter_local_affine(ctx.h if ctx is not None else None, tent.ctypes.data_as(C.c_void_p), u6.ctypes.data_as(C.c_void_p),
                                          lf.ctypes.data_as(C.c_void_p), n, C.byref(par), C.byref(m), keep.ctypes.data_as(C.c_void_p),
                                          nb.ctypes.data_as(C.c_void_p), sup.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p)))
    diag = {"keep": keep[:n].astype(bool), "neighbours": nb[:n], "support": sup[:n], "backed": back[:n]}
    return tent[:m.value].copy(), u6[:m.value].copy(), lf[:m.value].copy(), diag


# ---- verification (degensac C ABI + LORANSACFiltering) ---------------------------------------------
class Score(C.Structure):
    _fields_ = [("I", C.c_uint), ("J", C.c_double)]


class RansacParams(C.Structure):
    """[RANSAC] section (io_mods.cpp:437-455).  errorType 0 Sampson, 1 SymmMax, 2 SymmSum."""
    _fields_ = [("err_threshold", C.c_double), ("confidence", C.c_double), ("max_samples", C.c_int),
                ("localOptimization", C.c_int), ("LAFCoef", C.c_double), ("HLAFCoef", C.c_double),
                ("errorType", C.c_int), ("doSymmCheck", C.c_int), ("useF", C.c_int),
                ("groundTruth", C.c_int), ("ransacForStopping", C.c_int), ("gtH", C.c_double * 9)]

    @staticmethod
    def default(useF=0):
        return RansacParams(4.0, 0.99, 1000000, 1, 2.0, 12.0, 0, 1, useF, 0, 0)   # config_affori_classic.ini


_ERR = {"sampson": ("HDs", "HDsi", "HDsidx"), "symm_max": ("HDsSymMax", "HDsiSymMax", "HDsSymidxMax"),
        "symm_sum": ("HDsSym", "HDsiSym", "HDsSymidx")}


def ransac_pin_seed(seed):
    lib().mods_ransac_pin_seed.argtypes = [C.c_long]
    lib().mods_ransac_pin_seed(seed)


def match_grid(n_q, n_t):
    """mods_match_grid: (query blocks, train splits, tiles per split) of the first pass of an n_q x n_t FGINN search; needs no device."""
    out = (C.c_int * 3)()
    _check(lib().mods_match_grid(int(n_q), int(n_t), out))
    return out[0], out[1], out[2]


def knn_grid(n_q, n_t, k, forced_splits=0):
    """mods_match_knn_grid: (query blocks, train splits, tiles per split) of the sweep of an n_q x n_t k-NN search (forced_splits as
    Context.knn_splits sets them); needs no device."""
    out = (C.c_int * 3)()
    _check(lib().mods_match_knn_grid(int(n_q), int(n_t), int(k), int(forced_splits), out))
    return out[0], out[1], out[2]


def descdb_grid(m, n_queries, forced_splits=0):
    """mods_descdb_grid: (query blocks, database splits, tiles per split) of the distractor sweep of n_queries queries against m rows
    (forced_splits as Context.descdb_splits sets them); needs no device."""
    out = (C.c_int * 3)()
    _check(lib().mods_descdb_grid(C.c_long(int(m)), int(n_queries), int(forced_splits), out))
    return out[0], out[1], out[2]


class DescDB:
    """mods_descdb_*: an immutable database of distractor descriptors on one device, packed once for the distance kernels; any number
    of contexts and pipelines of the device may share it (Context.set_distractor_db, Pipeline.set_distractor_db).  desc: (n, 128)
    uint8, n = 0 allowed; or DescDB.from_reps(ctx, reps) from the descriptors of ImgRep banks."""

    def __init__(self, desc=None, device=0, _handle=None):
        self.h = C.c_void_p()
        self.device = device
        if _handle is not None:
            self.h = _handle
            return
        d = np.ascontiguousarray(desc if desc is not None else np.zeros((0, 128), np.uint8))
        if d.dtype != np.uint8 or d.ndim != 2 or d.shape[1] != 128:
            raise ModsError("DescDB: descriptors of shape %s and type %s, (n, 128) uint8 expected" % (tuple(d.shape), d.dtype))
        _check(lib().mods_descdb_create(int(device), _vp(d) if len(d) else None, C.c_long(len(d)), C.byref(self.h)))

    @staticmethod
    def from_reps(ctx, reps):
        h = C.c_void_p()
        arr = (C.c_void_p * max(len(reps), 1))(*[r.h for r in reps])
        _check(lib().mods_descdb_create_from_reps(ctx.h, arr, len(reps), C.byref(h)))
        return DescDB(_handle=h)

    def __len__(self):
        lib().mods_descdb_count.restype = C.c_long
        return int(lib().mods_descdb_count(self.h))

    def close(self):
        """gives up this object's reference; a context that holds the database keeps it alive"""
        if self.h:
            lib().mods_descdb_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def min_dist(self, ctx, desc):
        """mods_descdb_min_dist: the exact squared L2 distance of every row of desc (n, 128) uint8 to its nearest database row
        (INT_MAX for an empty database)"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 128)
        out = np.zeros(max(len(d), 1), np.int32)
        _check(lib().mods_descdb_min_dist(ctx.h, self.h, _vp(d) if len(d) else None, len(d), _vp(out)))
        return out[:len(d)].copy()


def filter_distractor(ctx, db, q, tent, u6, laf, ratio=0.8):
    """mods_filter_distractor on copies of the three arrays: the veto of DescDB db on a host list whose q indices name rows of the
    region list q; returns (tent, u6, laf, dDB) of the survivors in list order"""
    q = np.ascontiguousarray(q)
    tent = np.ascontiguousarray(tent, TENT_DTYPE).copy()
    u6 = np.ascontiguousarray(u6, np.float64).reshape(-1, 6).copy()
    laf = np.ascontiguousarray(laf, np.float64).reshape(-1, 14).copy()
    n = len(tent)
    ddb = np.zeros(max(n, 1), np.int32)
    n_out = C.c_int()
    _check(lib().mods_filter_distractor(ctx.h, db.h, _vp(q) if len(q) else None, len(q), C.c_double(ratio), _vp(tent) if n else None,
                                        _vp(u6) if n else None, _vp(laf) if n else None, n, _vp(ddb), C.byref(n_out)))
    k = n_out.value
    return tent[:k], u6[:k], laf[:k], ddb[:k]


def _knn_rows(n_q, k, call):
    """room for the rows of a k-NN search; call(idx, d2) fills them and returns its code; returns (dist, index)"""
    k = int(k)
    dist = np.zeros((n_q, max(k, 1)), np.int32)
    index = np.zeros((n_q, max(k, 1)), np.int32)
    _check(call(index.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p)))
    return dist, index


def list_search_grid(search, n_q, n_t, forced_splits=0):
    """mods_list_search_grid: (query blocks, train splits, tiles per split) of the sweep of an n_q x n_t search of two region lists
    (search 0: guided, 1: overlap and area-overlap, with forced_splits as Context.overlap_splits sets them); needs no device."""
    out = (C.c_int * 3)()
    _check(lib().mods_list_search_grid(int(search), int(n_q), int(n_t), int(forced_splits), out))
    return out[0], out[1], out[2]


def ransac_h(u6, th_sq, conf=0.99, max_sam=1000000, err="sampson", sym_check=1, seed_time=12345, errfn=None):
    """exp_ransacHcustom exactly as LORANSACFiltering calls it (matching.cpp:731).  errfn: a ctypes callback with HDs's signature
    passed in place of the library's own function - a foreign error function, which the run evaluates on the host."""
    L = lib()
    L.exp_ransacHcustom.restype = Score
    ransac_pin_seed(seed_time)
    u = np.ascontiguousarray(u6, np.float64).copy()
    n = len(u)
    H = np.zeros(9, np.float64)
    inl = np.zeros(max(n, 1), np.uint8)
    data_out = np.zeros(max(18 * n, 8), np.int32)
    resids = C.POINTER(C.c_double)()
    f = [C.cast(getattr(L, name), C.c_void_p) for name in _ERR[err]]
    if errfn is not None:
        f[0] = C.cast(errfn, C.c_void_p)
    S = L.exp_ransacHcustom(u.ctypes.data_as(C.c_void_p), n, C.c_double(th_sq), C.c_double(conf), max_sam,
                            H.ctypes.data_as(C.c_void_p), inl.ctypes.data_as(C.c_void_p), 4,
                            data_out.ctypes.data_as(C.c_void_p), 1, C.c_uint(0), C.byref(resids), f[0], f[1], f[2],
                            sym_check)
    C.CDLL(None).free(resids)
    return dict(I=S.I, J=S.J, H=H, inl=inl[:n], samples=int(data_out[0]), lo=int(data_out[1]), rej=int(data_out[2]))


_FERR = {"sampson": ("FDs", "exFDs"), "symm": ("FDsSym", "exFDsSym")}


def ransac_f(u6, th_sq, conf=0.99, max_sam=100000, err="sampson", sym_check=0, do_lo=1, inl_limit=0, seed_time=12345, errfn=None):
    """exp_ransacFcustom exactly as LORANSACFiltering calls it (matching.cpp:722).  errfn: a ctypes callback with FDs's signature
    passed in place of the library's own function (evaluated on the host)."""
    L = lib()
    L.exp_ransacFcustom.restype = C.c_int
    ransac_pin_seed(seed_time)
    u = np.ascontiguousarray(u6, np.float64).copy()
    n = len(u)
    F = np.zeros(9, np.float64)
    Hb = np.zeros(9, np.float64)
    inl = np.zeros(max(n, 1), np.uint8)
    data_out = np.zeros(max(18 * n, 16), np.int32)
    resids = C.POINTER(C.c_double)()
    Ih = C.c_int(0)
    fds, exfds = (C.cast(getattr(L, name), C.c_void_p) for name in _FERR[err])
    if errfn is not None:
        fds = C.cast(errfn, C.c_void_p)
    I = L.exp_ransacFcustom(u.ctypes.data_as(C.c_void_p), n, C.c_double(th_sq), C.c_double(conf), max_sam,
                            F.ctypes.data_as(C.c_void_p), inl.ctypes.data_as(C.c_void_p), data_out.ctypes.data_as(C.c_void_p),
                            do_lo, C.c_uint(inl_limit), C.byref(resids), Hb.ctypes.data_as(C.c_void_p), C.byref(Ih), exfds, fds,
                            sym_check)
    C.CDLL(None).free(resids)
    return dict(I=I, F=F, inl=inl[:n], samples=int(data_out[0]), lo=int(data_out[1]), Ih=Ih.value, hist=data_out[2:n + 3].copy())


def _score_round(fn, u6, models, err_type, do_sym, th, th_check, with_records):
    u = np.ascontiguousarray(u6, np.float64)
    m = np.ascontiguousarray(models, np.float64).reshape(-1, 9)
    if u.ndim != 2 or u.shape[1] != 6:
        raise ValueError("u6 must be len x 6 (x1 y1 1 x2 y2 1)")
    n, ln = len(m), len(u)
    d = np.zeros((n, ln), np.float64)
    J = np.zeros(n, np.float64)
    counts = np.zeros((n, 2), np.int32)
    args = [_vp(u), ln, _vp(m), n, int(err_type), int(do_sym), C.c_double(th), C.c_double(th_check), _vp(d), _vp(J), _vp(counts)]
    rec = np.zeros((n, 27), np.float64) if with_records else None
    if with_records:
        args.append(_vp(rec))
    _check(fn(*args))
    out = dict(d=d, J=J, I=counts[:, 0].copy(), Isym=counts[:, 1].copy())
    if with_records:
        out.update(h=rec[:, 0:9].copy(), Hinv=rec[:, 9:18].copy(), H1=rec[:, 18:27].copy())
    return out


def host_sym_prepare(h):
    """mods_test_host_sym_prepare: (Hinv, H1) of a model h[9] as a scored record carries them; needs no device."""
    h = np.ascontiguousarray(h, np.float64).reshape(9)
    Hinv, H1 = np.zeros(9), np.zeros(9)
    _check(lib().mods_test_host_sym_prepare(_vp(h), _vp(Hinv), _vp(H1)))
    return Hinv, H1


def ransac_test_score_h(u6, h, err_type, do_sym, th, th_check):
    """mods_test_ransac_score_h: one scoring round of the models h (n x 9, column-major) over u6 through the calling thread's
    workspace and gpu_score.  err_type 0 Sampson, 1 symmetric sum, 2 symmetric max.  Returns dict(d [n][len], J, I, Isym, and the
    records as uploaded: h, Hinv, H1 [n][9] each)."""
    return _score_round(lib().mods_test_ransac_score_h, u6, h, err_type, do_sym, th, th_check, True)


def ransac_test_score_f(u6, f, err_type, do_sym, th, th_check):
    """mods_test_ransac_score_f: the same for matrices f (n x 9) through gpu_score_f; err_type 0 Sampson, 1 symmetric epipolar."""
    return _score_round(lib().mods_test_ransac_score_f, u6, f, err_type, do_sym, th, th_check, False)


def ransac_test_count_pairs(uN, us, Ht, limit, pairs0, pairs1):
    """mods_test_ransac_count_pairs: counts of two blocks of plane-and-parallax candidates (k x 2 indices into the off-plane set
    each), slot 0 and slot 1 in flight together."""
    uN = np.ascontiguousarray(uN, np.float64); us = np.ascontiguousarray(us, np.float64)
    Ht = np.ascontiguousarray(Ht, np.float64).reshape(9)
    p0 = np.ascontiguousarray(pairs0, np.uint32).reshape(-1, 2); p1 = np.ascontiguousarray(pairs1, np.uint32).reshape(-1, 2)
    if uN.shape != us.shape or uN.ndim != 2 or uN.shape[1] != 6:
        raise ValueError("uN and us must be n x 6")
    c0, c1 = np.zeros(len(p0), np.uint32), np.zeros(len(p1), np.uint32)
    _check(lib().mods_test_ransac_count_pairs(_vp(uN), _vp(us), len(uN), _vp(Ht), C.c_double(limit), _vp(p0), len(p0), _vp(p1), len(p1),
                                              _vp(c0), _vp(c1)))
    return c0, c1


def ransac_test_count_models(u6, Fs, limit):
    """mods_test_ransac_count_models: #{i : FDs(u6_i, Fs_j) < limit} of k matrices (k x 9) through gpu_count_models."""
    u = np.ascontiguousarray(u6, np.float64)
    F = np.ascontiguousarray(Fs, np.float64).reshape(-1, 9)
    if u.ndim != 2 or u.shape[1] != 6:
        raise ValueError("u6 must be len x 6")
    c = np.zeros(len(F), np.uint32)
    _check(lib().mods_test_ransac_count_models(_vp(u), len(u), _vp(F), len(F), C.c_double(limit), _vp(c)))
    return c


def loransac_h(u6, laf, params=None, seed_time=12345):
    params = params or RansacParams.default()
    ransac_pin_seed(seed_time)
    u = np.ascontiguousarray(u6, np.float64)
    n = len(u)
    lf = np.ascontiguousarray(laf, np.float64) if laf is not None else None
    mask = np.zeros(max(n, 1), np.uint8)
    H = np.zeros(9, np.float64)
    ninl = C.c_int()
    stats = (C.c_int * 3)()
    _check(lib().mods_loransac_h(u.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p) if lf is not None else None,
                                 n, C.byref(params), mask.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p),
                                 C.byref(ninl), stats))
    return mask[:n].astype(bool), H.reshape(3, 3), ninl.value, list(stats)


def loransac_f(u6, laf, params=None, seed_time=12345):
    """useF branch of LORANSACFiltering: DEGENSAC + F_LAF_check.  Returns (mask, F as stored, n, stats)."""
    params = params or RansacParams.default(useF=1)
    ransac_pin_seed(seed_time)
    u = np.ascontiguousarray(u6, np.float64)
    n = len(u)
    lf = np.ascontiguousarray(laf, np.float64) if laf is not None else None
    mask = np.zeros(max(n, 1), np.uint8)
    F = np.zeros(9, np.float64)
    ninl = C.c_int()
    stats = (C.c_int * 3)()
    _check(lib().mods_loransac_f(u.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p) if lf is not None else None,
                                 n, C.byref(params), mask.ctypes.data_as(C.c_void_p), F.ctypes.data_as(C.c_void_p),
                                 C.byref(ninl), stats))
    return mask[:n].astype(bool), F, ninl.value, list(stats)


def orsa_f(u6, laf, w, h, params=None, seed_time=12345, on_device=True, batch=0, wg_keys=0):
    """ORSAFiltering (useF = 2): ORSA a-contrario F verification, hypotheses scored on the GPU (on_device=False: the host
    scoring path, no device needed).  Returns dict(mask, F as ransac_corresp.H holds it, n, log_nfa, index, stats)."""
    params = params or RansacParams.default(useF=2)
    if seed_time is not None:
        ransac_pin_seed(seed_time)
    u = np.ascontiguousarray(u6, np.float64)
    if u.ndim != 2 or u.shape[1] != 6:
        raise ValueError("u6 must be n x 6 (x1 y1 1 x2 y2 1)")
    n = len(u)
    lf = np.ascontiguousarray(laf, np.float64) if laf is not None else None
    if lf is not None and lf.shape != (n, 14):
        raise ValueError("laf must be n x 14")
    mask = np.zeros(max(n, 1), np.uint8)
    F = np.zeros(9, np.float64)
    index = np.zeros(max(n, 1), np.int32)
    ninl, nidx, nfa = C.c_int(), C.c_int(), C.c_float()
    stats = (C.c_int * 3)()
    _check(lib().mods_orsa_f_ex(u.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p) if lf is not None else None, n,
                                int(w), int(h), C.byref(params), mask.ctypes.data_as(C.c_void_p), F.ctypes.data_as(C.c_void_p),
                                C.byref(ninl), C.byref(nfa), index.ctypes.data_as(C.c_void_p), C.byref(nidx), stats,
                                1 if on_device else 0, int(batch), int(wg_keys)))
    return dict(mask=mask[:n].astype(bool), F=F, n=ninl.value, log_nfa=np.float32(nfa.value), index=index[:nidx.value].copy(),
                stats=list(stats))


def orsa_h(u6, laf, w, h, params=None, seed_time=12345, on_device=True, batch=0, wg_keys=0):
    """ORSA-H (useF = 3): a-contrario homography verification, samples solved and scored on the GPU (on_device=False: the host
    path, no device needed).  Returns dict(mask, H row-major img1 -> img2 in pixels, n, log_nfa, thr_px, index, stats, refit)
    with refit = (the loop's nfa, the refit model's nfa, taken)."""
    params = params or RansacParams.default(useF=3)
    if seed_time is not None:
        ransac_pin_seed(seed_time)
    u = np.ascontiguousarray(u6, np.float64)
    if u.ndim != 2 or u.shape[1] != 6:
        raise ValueError("u6 must be n x 6 (x1 y1 1 x2 y2 1)")
    n = len(u)
    lf = np.ascontiguousarray(laf, np.float64) if laf is not None else None
    if lf is not None and lf.shape != (n, 14):
        raise ValueError("laf must be n x 14")
    mask = np.zeros(max(n, 1), np.uint8)
    H = np.zeros(9, np.float64)
    index = np.zeros(max(n, 1), np.int32)
    ninl, nidx, nfa, thr = C.c_int(), C.c_int(), C.c_float(), C.c_double()
    stats = (C.c_int * 3)()
    _check(lib().mods_orsa_h_ex(u.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p) if lf is not None else None, n,
                                int(w), int(h), C.byref(params), mask.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p),
                                C.byref(ninl), C.byref(nfa), C.byref(thr), index.ctypes.data_as(C.c_void_p), C.byref(nidx), stats,
                                1 if on_device else 0, int(batch), int(wg_keys)))
    a, b, taken = C.c_float(), C.c_float(), C.c_int()
    _check(lib().mods_orsa_h_last_refit(C.byref(a), C.byref(b), C.byref(taken)))
    return dict(mask=mask[:n].astype(bool), H=H, n=ninl.value, log_nfa=np.float32(nfa.value), thr_px=thr.value,
                index=index[:nidx.value].copy(), stats=list(stats), refit=(np.float32(a.value), np.float32(b.value), taken.value))


def orsa_h_test_tables(n):
    a, b = np.zeros(n + 1, np.float32), np.zeros(n + 1, np.float32)
    _check(lib().mods_test_orsa_h_tables(int(n), _fp(a), _fp(b)))
    return a, b


def orsa_h_test_score(p1, p2, w, h, samples4, on_device=True, wg_keys=0):
    """per-sample (nfa bits, first argmin, logalpha bits, invalid flag) and the solved models (m x 9 float32) of samples4
    (m x 4 indices) over normalised points p1 / p2 (n x 2 float32 each, flattened)"""
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1); p2 = np.ascontiguousarray(p2, np.float32).reshape(-1)
    s = np.ascontiguousarray(samples4, np.int32).reshape(-1, 4)
    out = np.zeros((len(s), 4), np.int32)
    Hs = np.zeros((len(s), 9), np.float32)
    _check(lib().mods_test_orsa_h_score(_fp(p1), _fp(p2), len(p1) // 2, int(w), int(h), s.ctypes.data_as(C.c_void_p), len(s),
                                        1 if on_device else 0, int(wg_keys), out.ctypes.data_as(C.c_void_p), _fp(Hs)))
    return out, Hs


def model_kind(useF):
    """0: useF verifies a homography (0, 3); 1: a fundamental matrix (1, 2)"""
    kind = lib().mods_model_kind(int(useF))
    if kind < 0:
        _check(kind)
    return kind


def orsa_last_profile():
    """ms of the calling thread's last orsa_f call: solve, score, kernel, replay, total; and the scoring launches."""
    ms = (C.c_double * 5)()
    launches = C.c_long()
    _check(lib().mods_orsa_last_profile(ms, C.byref(launches)))
    return dict(zip(("solve", "score", "kernel", "replay", "total"), list(ms)), launches=launches.value)


def orsa_test_epipolar(p1, p2, k7):
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
    k = np.ascontiguousarray(k7, np.int32)
    F1, F2, z = np.zeros(9, np.float32), np.zeros(9, np.float32), np.zeros(3, np.float32)
    m = lib().mods_test_orsa_epipolar(_fp(p1), _fp(p2), k.ctypes.data_as(C.c_void_p), _fp(F1), _fp(F2), _fp(z))
    return F1, F2, z, m


def orsa_test_tables(n):
    a, b = np.zeros(n + 1, np.float32), np.zeros(n + 1, np.float32)
    _check(lib().mods_test_orsa_tables(int(n), _fp(a), _fp(b)))
    return a, b


def orsa_test_log10(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    _check(lib().mods_test_orsa_log10(_fp(x), len(x), _fp(out)))
    return out


def orsa_test_score(p1, p2, w, h, F, on_device=True, wg_keys=0):
    """per-model (nfa, first argmin, logalpha, NaN flag) of models F (m x 9) over normalised points"""
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
    F = np.ascontiguousarray(F, np.float32).reshape(-1, 9)
    out = np.zeros((len(F), 4), np.int32)
    _check(lib().mods_test_orsa_score(_fp(p1), _fp(p2), len(p1) // 2, int(w), int(h), _fp(F), len(F), 1 if on_device else 0,
                                      int(wg_keys), out.ctypes.data_as(C.c_void_p)))
    return out


def orsa_log10_sweep(begin, count, max_list=1024):
    L = lib()
    L.mods_test_orsa_log10_sweep.restype = C.c_longlong
    lst = np.zeros(max_list, np.uint32)
    bad = L.mods_test_orsa_log10_sweep(C.c_uint(begin), C.c_uint(count), lst.ctypes.data_as(C.c_void_p), max_list)
    if bad < 0:
        _check(int(bad))
    return int(bad), lst[:min(bad, max_list)].copy()


def verify_tentatives(tent, u6, laf, params, device=0, seed_time=None, wh=None):
    """mods_verify_tentatives: duplicate filtering + LORANSACFiltering in the order [DuplicateFiltering] doBeforeRANSAC asks for
    (mods.cpp:278-368).  Returns (verified tentatives, their u6, their laf, n_unique, H, stats).  wh = (w, h): the image size,
    required by useF = 2 and 3 (ORSA F and H; mods_verify_tentatives_wh)."""
    if seed_time is not None:
        ransac_pin_seed(seed_time)
    tent = np.ascontiguousarray(tent).copy()
    u = np.ascontiguousarray(u6, np.float64).copy()
    lf = np.ascontiguousarray(laf, np.float64).copy()
    nu, nv = C.c_int(), C.c_int()
    H = np.zeros(9, np.float64)
    stats = (C.c_int * 3)()
    if wh is None:
        _check(lib().mods_verify_tentatives(device, C.byref(params), tent.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p),
                                            lf.ctypes.data_as(C.c_void_p), len(tent), C.byref(nu), C.byref(nv),
                                            H.ctypes.data_as(C.c_void_p), stats, None, None))
    else:
        _check(lib().mods_verify_tentatives_wh(device, C.byref(params), tent.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p),
                                               lf.ctypes.data_as(C.c_void_p), len(tent), int(wh[0]), int(wh[1]), C.byref(nu),
                                               C.byref(nv), H.ctypes.data_as(C.c_void_p), stats, None, None, None))
    m = nv.value
    return tent[:m].copy(), u[:m].copy(), lf[:m].copy(), nu.value, H, list(stats)


# ---- multi-view representation and the MODS step loop --------------------------------------------------------
class ViewPar(C.Structure):
    _fields_ = [("zoom", C.c_double), ("tilt", C.c_double), ("phi", C.c_double)]


class LadderStep(C.Structure):
    """One [HessianAffine<i>] section of an iterations .ini (io_mods.cpp:457-492)."""
    _fields_ = [("scale_set", C.c_double * 8), ("n_scales", C.c_int), ("tilt_set", C.c_double * 8), ("n_tilts", C.c_int),
                ("phi", C.c_double), ("initSigma", C.c_double), ("doBlur", C.c_int), ("fginn_ratio", C.c_double),
                ("half_orientation", C.c_int), ("fginn_ratio_half", C.c_double), ("dist_threshold", C.c_double),
                ("dist_threshold_half", C.c_double)]

    @staticmethod
    def make(tilts, phi, scales=(1.0,), init_sigma=0.2, do_blur=1, fginn=0.8, half_orientation=0, fginn_half=0.0, dist=0.0, dist_half=0.0):
        """half_orientation: the step's descriptor list names a Half* descriptor; fginn_half > 0: HalfRootSIFT lists are built and
        matched too (SeparateDescriptors = RootSIFT,HalfRootSIFT)."""
        s = LadderStep()
        for i, v in enumerate(scales):
            s.scale_set[i] = v
        for i, v in enumerate(tilts):
            s.tilt_set[i] = v
        s.n_scales, s.n_tilts, s.phi, s.initSigma, s.doBlur, s.fginn_ratio = len(scales), len(tilts), phi, init_sigma, do_blur, fginn
        s.half_orientation, s.fginn_ratio_half = half_orientation, fginn_half
        s.dist_threshold, s.dist_threshold_half = dist, dist_half     # DistanceThreshold: MatchFLANNDistance replaces the FGINN list
        return s


def iters_mods_steps(half=True):
    """[HessianAffine2] and [HessianAffine3] of build/iters_MODS.ini (the HessianAffine steps of the MODS ladder):
    Descriptors = RootSIFT,HalfRootSIFT with FGINNThreshold = 0.8 for the first of them only, i.e. the orientation runs in
    doHalfSIFT mode and the RootSIFT lists are matched (the reference reads the missing second threshold past the end of a
    one-element vector; it is 0 here: HalfRootSIFT lists are not matched)."""
    return [LadderStep.make((1, 2, 4, 6, 8), 360.0, half_orientation=int(half)), LadderStep.make((1, 2, 4, 6, 8), 120.0, half_orientation=int(half))]


class LadderResult(C.Structure):
    _fields_ = [("steps_done", C.c_int), ("n_views", C.c_int), ("n_detected", C.c_int * 2), ("n_described", C.c_int * 2),
                ("n_unoriented", C.c_int * 2), ("n_tentatives", C.c_int), ("n_unique", C.c_int), ("n_inliers", C.c_int),
                ("ransac_samples", C.c_int), ("ransac_lo", C.c_int), ("ransac_rejects", C.c_int), ("H", C.c_double * 9),
                ("ms_detect_describe", C.c_double), ("ms_match", C.c_double), ("ms_duplicates", C.c_double),
                ("ms_ransac", C.c_double), ("gt_true", C.c_int), ("gt_ransac_inliers", C.c_int), ("gt_true_of_ransac", C.c_int)]


def hmatrix_filter(u6, H, ransac=None):
    """HMatrixFiltering (matching.cpp:917-1012): mask of the correspondences within err_threshold of the row-major homography H."""
    u = np.ascontiguousarray(u6, np.float64)
    Hm = np.ascontiguousarray(H, np.float64).reshape(9)
    par = ransac or RansacParams.default()
    mask = np.zeros(max(len(u), 1), np.uint8)
    n = C.c_int()
    _check(lib().mods_hmatrix_filter(u.ctypes.data_as(C.c_void_p), len(u), Hm.ctypes.data_as(C.c_void_p), C.byref(par),
                                     mask.ctypes.data_as(C.c_void_p), C.byref(n)))
    return mask[:len(u)].astype(bool), n.value


def view_schedule(step, history):
    """SetVSPars for one step; `history` (list of (zoom, tilt, phi)) is extended in place.  Returns the new views."""
    prev = (ViewPar * 1024)()
    for i, v in enumerate(history):
        prev[i] = ViewPar(*v)
    n_prev = C.c_int(len(history))
    out = (ViewPar * 256)()
    n = lib().mods_view_schedule(step.scale_set, step.n_scales, step.tilt_set, step.n_tilts, C.c_double(step.phi), prev,
                                 C.byref(n_prev), 1024, out, 256)
    _check(min(n, 0))
    views = [(out[i].zoom, out[i].tilt, out[i].phi) for i in range(n)]
    history.extend(views)
    return views


class ImgRep:
    """Accumulated regions of one image in HBM (ImageRepresentation::AddRegions)."""

    def __init__(self, ctx, capacity=1 << 19):
        self.h = C.c_void_p()
        self.ctx = ctx
        _check(lib().mods_imgrep_create(ctx.h, capacity, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().mods_imgrep_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        _check(lib().mods_imgrep_clear(self.h))

    def __len__(self):
        return lib().mods_imgrep_count(self.h)

    @property
    def dev_ptr(self):
        lib().mods_imgrep_regions_dev.restype = C.c_void_p
        return lib().mods_imgrep_regions_dev(self.h)

    def append_ctx(self, img=0):
        _check(lib().mods_imgrep_append_ctx(self.h, self.ctx.h, img))

    def append_dev(self, dev_ptr, n):
        _check(lib().mods_imgrep_append_dev(self.h, C.c_void_p(dev_ptr), n))

    def append_host(self, regions):
        r = np.ascontiguousarray(regions)
        _check(lib().mods_imgrep_append_host(self.h, r.ctypes.data_as(C.c_void_p), len(r)))

    def fetch(self, begin=0, count=None):
        count = len(self) - begin if count is None else count
        out = np.zeros(max(count, 1), REGION_DTYPE)
        _check(lib().mods_imgrep_fetch(self.h, begin, count, out.ctypes.data_as(C.c_void_p)))
        return out[:count].copy()


def match_reps(ctx, q, t, q_begin=0, q_end=None, ratio=0.8, contrad=10.0, nn=50):
    """MatchImgReps for the query slice [q_begin, q_end) of ImgRep q against all of ImgRep t."""
    q_end = len(q) if q_end is None else q_end
    cap = max(q_end - q_begin, 1)
    return _tentatives(cap, lambda out, u6, laf, n: lib().mods_match_reps(
        ctx.h, q.h, q_begin, q_end, t.h, C.c_double(ratio), C.c_double(contrad), nn, out, u6, laf, cap, n))


class GuidedParams(C.Structure):
    """mods_guided_params: the model-guided search behind a verification (no counterpart in the reference)."""
    _fields_ = [("model_type", C.c_int), ("model", C.c_double * 9), ("radius", C.c_double), ("ratio", C.c_double),
                ("contradDist", C.c_double), ("max_dist", C.c_int), ("one_to_one", C.c_int)]

    @staticmethod
    def default(model=None, model_type=0, radius=4.0, ratio=0.9, contrad=10.0, max_dist=0, one_to_one=1):
        """radius = [RANSAC] err_threshold, contradDist = [Matching] contradDist of config_affori_classic.ini; model: 9 values as
        PairResult.H / LadderResult.H deliver them (model_type 1: F in degensac's layout)"""
        p = GuidedParams(model_type, (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), radius, ratio, contrad, max_dist, one_to_one)
        if model is not None:
            p.model = (C.c_double * 9)(*[float(v) for v in np.asarray(model, np.float64).reshape(9)])
        return p


def match_guided_reps(ctx, rep_q, rep_t, params, cap=None):
    """mods_match_guided_reps: the guided search of ImgRep rep_q against ImgRep rep_t (HBM resident); returns (tent, u6, laf).
    cap: room for that many tentatives (default: one per query, which always suffices)."""
    cap = max(len(rep_q), 1) if cap is None else cap
    return _tentatives(cap, lambda out, u6, laf, n: lib().mods_match_guided_reps(
        ctx.h, rep_q.h, rep_t.h, C.byref(params), out, u6, laf, cap, n))


OVERLAP_DTYPE = np.dtype([("q", "i4"), ("t", "i4"), ("E", "f8"), ("dist", "f8"), ("diff", "f8")])


class OverlapParams(C.Structure):
    """mods_overlap_params: ground-truth overlap matching ([OverlapMatching] of the reference's configuration)."""
    _fields_ = [("H", C.c_double * 9), ("max_error", C.c_double), ("oriented", C.c_int), ("one_to_one", C.c_int),
                ("w1", C.c_int), ("h1", C.c_int), ("w2", C.c_int), ("h2", C.c_int)]

    @staticmethod
    def default(H=None, max_error=0.09, oriented=1, one_to_one=1, w1=0, h1=0, w2=0, h2=0):
        """max_error = [OverlapMatching] overlapError of config_affori_classic.ini; H: 9 values row-major, image 1 -> image 2;
        sizes 0: no common-area test"""
        p = OverlapParams((C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), max_error, oriented, one_to_one, w1, h1, w2, h2)
        if H is not None:
            p.H = (C.c_double * 9)(*[float(v) for v in np.asarray(H, np.float64).reshape(9)])
        return p


class OverlapCounts(C.Structure):
    """mods_overlap_counts; the customary repeatability figure is the one with one_to_one = 1."""
    _fields_ = [("n_q_common", C.c_int), ("n_t_common", C.c_int), ("n_matches", C.c_int), ("repeatability", C.c_double)]


def match_overlap_reps(ctx, rep_q, rep_t, params, cap=None):
    """mods_match_overlap_reps: overlap matching of ImgRep rep_q against ImgRep rep_t (HBM resident); returns (matches, counts).
    cap: room for that many matches (default: one per query, which always suffices)."""
    cap = max(len(rep_q), 1) if cap is None else cap
    return _overlap(lib().mods_match_overlap_reps, OVERLAP_DTYPE, (ctx.h, rep_q.h, rep_t.h), params, cap)


OVERLAP_AREA_DTYPE = np.dtype([("q", "i4"), ("t", "i4"), ("E", "f8"), ("n_q_px", "i4"), ("n_t_px", "i4"), ("n_both", "i4"), ("pad", "i4")])


class OverlapAreaParams(C.Structure):
    """mods_overlap_area_params: area-overlap matching, the repeatability measure of Mikolajczyk et al."""
    _fields_ = [("H", C.c_double * 9), ("max_error", C.c_double), ("one_to_one", C.c_int),
                ("w1", C.c_int), ("h1", C.c_int), ("w2", C.c_int), ("h2", C.c_int)]

    @staticmethod
    def default(H=None, max_error=0.4, one_to_one=2, w1=0, h1=0, w2=0, h2=0):
        """the customary protocol: error below 0.4, greedy one-to-one assignment (one_to_one = 2; 0: per query the best train,
        1: the rule of OverlapParams); H: 9 values row-major, image 1 -> image 2; sizes 0: no common-area test"""
        p = OverlapAreaParams((C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), max_error, one_to_one, w1, h1, w2, h2)
        if H is not None:
            p.H = (C.c_double * 9)(*[float(v) for v in np.asarray(H, np.float64).reshape(9)])
        return p


def match_overlap_area_reps(ctx, rep_q, rep_t, params, cap=None):
    """mods_match_overlap_area_reps: area-overlap matching of ImgRep rep_q against ImgRep rep_t (HBM resident); returns (matches,
    counts).  cap: room for that many matches (default: one per query, which always suffices)."""
    cap = max(len(rep_q), 1) if cap is None else cap
    return _overlap(lib().mods_match_overlap_area_reps, OVERLAP_AREA_DTYPE, (ctx.h, rep_q.h, rep_t.h), params, cap)


def _verified_lafs(fn, handle):
    n = C.c_int()
    _check(fn(handle, None, 0, C.byref(n)))
    out = np.zeros((max(n.value, 1), 14), np.float64)
    _check(fn(handle, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    return out[:n.value].copy()


# ---- match and region images (csrc/draw.hip) --------------------------------------------------------------------------
DRAW_ELEM_DTYPE = np.dtype([("kind", "i4"), ("ax", "i4"), ("ay", "i4"), ("bx", "i4"), ("by", "i4"), ("t", "i4"), ("rgb", "u4"),
                            ("group", "i4")])
DRAW_NONE, DRAW_DISC, DRAW_LINE, DRAW_SEG = -1, 0, 1, 2
DRAW_TABLE_REGIONS, DRAW_TABLE_MATCHES = 0, 1
DRAW_COLOUR_REGIONS = 0xA0FFFF           # DrawRegions' Scalar(255, 255, 160), B G R, as 0xRRGGBB


class DrawMatchesParams(C.Structure):
    """mods_draw_matches_params; M: H (row-major, image 1 -> image 2) with reproject_to_one_image, F with draw_epipolar_lines"""
    _fields_ = [("draw_only_centers", C.c_int), ("reproject_to_one_image", C.c_int), ("draw_epipolar_lines", C.c_int),
                ("r1", C.c_int), ("r2", C.c_int), ("pad", C.c_int), ("M", C.c_double * 9)]

    @staticmethod
    def default(M=None, centers_only=0, reproject=0, epipolar=0, r1=5, r2=4):
        """mods.cpp:461-465: r1 = 5, r2 = 4"""
        p = DrawMatchesParams(int(centers_only), int(reproject), int(epipolar), int(r1), int(r2), 0)
        m = np.eye(3) if M is None else np.asarray(M, np.float64)
        p.M[:] = [float(v) for v in m.reshape(9)]
        return p


class Canvas:
    """mods_canvas: an RGB8 image [h][w][3] in HBM that the tile rasteriser draws on"""

    def __init__(self, ctx, w, h, handle=None):
        self.ctx = ctx
        self.h = C.c_void_p()
        if handle is not None:
            self.h = handle
        else:
            _check(lib().mods_canvas_create(ctx.h, int(w), int(h), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().mods_canvas_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        """(w, h)"""
        return lib().mods_canvas_width(self.h), lib().mods_canvas_height(self.h)

    def fill(self, rgb=0xFFFFFF):
        _check(lib().mods_canvas_fill(self.h, C.c_uint(rgb)))
        return self

    def blit(self, img_u8, x0=0, y0=0):
        """an 8-bit host image [h][w] (grey, replicated) or [h][w][3] (R G B) with its corner at (x0, y0)"""
        a = np.ascontiguousarray(img_u8, np.uint8)
        ch = 1 if a.ndim == 2 else a.shape[2]
        _check(lib().mods_canvas_blit_u8(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], ch, int(x0), int(y0)))
        return self

    def blit_f32_dev(self, dev_ptr, w, h, stride=None, x0=0, y0=0):
        """an fp32 grey image in HBM, rounded and clamped to 8 bits"""
        _check(lib().mods_canvas_blit_f32_dev(self.h, C.c_void_p(dev_ptr), int(w), int(h), int(stride or w), int(x0), int(y0)))
        return self

    def blit_canvas(self, src, x0=0, y0=0):
        _check(lib().mods_canvas_blit_canvas(self.h, src.h, int(x0), int(y0)))
        return self

    def fetch(self):
        w, h = self.size
        out = np.empty((h, w, 3), np.uint8)
        _check(lib().mods_canvas_fetch(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def draw(self, elems):
        """mods_canvas_draw: the elements (DRAW_ELEM_DTYPE rows) in order; returns n_dropped"""
        e = np.ascontiguousarray(elems, DRAW_ELEM_DTYPE)
        nd = C.c_int()
        _check(lib().mods_canvas_draw(self.h, e.ctypes.data_as(C.c_void_p), len(e), C.byref(nd)))
        return nd.value

    def draw_regions(self, rep, begin=0, count=None, dx=0, dy=0, thickness=2, rgb=DRAW_COLOUR_REGIONS, table=DRAW_TABLE_REGIONS):
        """mods_canvas_draw_regions: the contours of regions [begin, begin + count) of ImgRep rep, built on the device; returns
        n_dropped"""
        count = len(rep) - begin if count is None else count
        nd = C.c_int()
        _check(lib().mods_canvas_draw_regions(self.h, rep.h, int(begin), int(count), int(dx), int(dy), int(thickness), C.c_uint(rgb),
                                              int(table), C.byref(nd)))
        return nd.value

    def regions_elems(self, rep, begin=0, count=None, dx=0, dy=0, thickness=2, rgb=DRAW_COLOUR_REGIONS, table=DRAW_TABLE_REGIONS):
        """mods_canvas_regions_elems: (the element list draw_regions would draw, n_dropped); nothing is drawn"""
        count = len(rep) - begin if count is None else count
        out = np.zeros(max(21 * count, 1), DRAW_ELEM_DTYPE)
        nd = C.c_int()
        _check(lib().mods_canvas_regions_elems(self.h, rep.h, int(begin), int(count), int(dx), int(dy), int(thickness), C.c_uint(rgb),
                                               int(table), out.ctypes.data_as(C.c_void_p), C.byref(nd)))
        return out[:21 * count].copy(), nd.value


def draw_matches_elems(which, w1, h1, w2, h2, laf14, params):
    """mods_draw_matches_elems: the element list of image `which` (0, 1) of draw_matches (host only)"""
    laf = np.ascontiguousarray(laf14, np.float64).reshape(-1, 14)
    cap = 64 * len(laf) + 1
    out = np.zeros(cap, DRAW_ELEM_DTYPE)
    n = C.c_int()
    _check(lib().mods_draw_matches_elems(int(which), int(w1), int(h1), int(w2), int(h2), laf.ctypes.data_as(C.c_void_p), len(laf),
                                         C.byref(params), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    return out[:n.value].copy()


def draw_matches(ctx, src1, src2, laf14, params):
    """mods_draw_matches: DrawMatches' two images of the verified frames laf14 [n][14] over the source canvases; returns
    (Canvas out1, Canvas out2, [n_dropped of out1, of out2])"""
    laf = np.ascontiguousarray(laf14, np.float64).reshape(-1, 14)
    o1, o2 = C.c_void_p(), C.c_void_p()
    nd = (C.c_int * 2)()
    _check(lib().mods_draw_matches(ctx.h, src1.h, src2.h, laf.ctypes.data_as(C.c_void_p), len(laf), C.byref(params), C.byref(o1),
                                   C.byref(o2), nd))
    return Canvas(ctx, 0, 0, o1), Canvas(ctx, 0, 0, o2), [nd[0], nd[1]]


def match_ladder_dev(ctx, img_ptr, w, h, steps, rep1, rep2, params=None, min_matches=15, max_matches=0, img2_ptr=None, w2=None, h2=None):
    """The step loop of mods.cpp:202-383 on one GPU; img_ptr: [2][h][w] fp32 in HBM (or two separate images)."""
    if img2_ptr is None:
        img2_ptr, w2, h2 = img_ptr + 4 * w * h, w, h
    params = params or PairParams.default()
    arr = (LadderStep * len(steps))(*steps)
    res = LadderResult()
    m = np.zeros((max(max_matches, 1), 4), np.float64)
    _check(lib().mods_match_ladder_dev(ctx.h, C.c_void_p(img_ptr), w, h, C.c_void_p(img2_ptr), w2, h2, arr, len(steps), min_matches,
                                       C.byref(params), rep1.h, rep2.h,
                                       C.byref(res), m.ctypes.data_as(C.c_void_p) if max_matches else None, max_matches))
    return res, m[:min(res.n_inliers, max_matches)]


class LadderGroup(C.Structure):
    """[Matching<i>] GroupDetectors / GroupDescriptors of one step (mods_ladder_group)."""
    _fields_ = [("n_dets", C.c_int), ("dets", C.c_int * 8), ("fginn_ratio", C.c_double), ("fginn_ratio_half", C.c_double),
                ("dist_threshold", C.c_double), ("dist_threshold_half", C.c_double)]

    @staticmethod
    def make(dets=(), ratio=0.0, ratio_half=-1.0, dist=0.0, dist_half=0.0):
        g = LadderGroup()
        g.n_dets = len(dets)
        for i, d in enumerate(dets):
            g.dets[i] = d
        g.fginn_ratio, g.fginn_ratio_half, g.dist_threshold, g.dist_threshold_half = ratio, ratio_half, dist, dist_half
        return g


def match_ladder_dets_dev(ctx, img_ptr, w, h, det_steps, det_params, reps1, reps2, params=None, min_matches=15, max_matches=0,
                          groups=None, group_pos=0):
    """mods_match_ladder_dets_dev: det_steps[d] = the steps of detector d (LadderStep, or None where the detector has no section),
    det_params[d] its HessAffParams; list the detectors sorted by name.  img_ptr: [2][h][w] fp32 in HBM."""
    n_det, n_steps = len(det_steps), max(len(x) for x in det_steps)
    arr = (LadderStep * (n_steps * n_det))()
    for d, steps in enumerate(det_steps):
        for i in range(n_steps):
            st = steps[i] if i < len(steps) and steps[i] is not None else None
            if st is None:
                st = LadderStep(); st.n_tilts = st.n_scales = -1
            arr[i * n_det + d] = st
    dets = (HessAffParams * n_det)(*det_params)
    r1 = (C.c_void_p * n_det)(*[r.h for r in reps1]); r2 = (C.c_void_p * n_det)(*[r.h for r in reps2])
    params = params or PairParams.default()
    res = LadderResult()
    m = np.zeros((max(max_matches, 1), 4), np.float64)
    garr = None
    if groups is not None:
        garr = (LadderGroup * n_steps)(*[g if g is not None else LadderGroup.make() for g in list(groups) + [None] * (n_steps - len(groups))])
    _check(lib().mods_match_ladder_groups_dev(ctx.h, C.c_void_p(img_ptr), w, h, C.c_void_p(img_ptr + 4 * w * h), w, h, arr, dets, garr, group_pos,
                                              n_steps, n_det, min_matches, C.byref(params), r1, r2, C.byref(res),
                                              m.ctypes.data_as(C.c_void_p) if max_matches else None, max_matches))
    return res, m[:min(res.n_inliers, max_matches)]


class Multi:
    """mods_multi_*: one hard pair on several GPUs (views sharded, one all-gather of the regions per step)."""

    def __init__(self, devices, w, h, rep_capacity=1 << 19):
        self.h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        _check(lib().mods_multi_create(arr, len(devices), w, h, rep_capacity, C.byref(self.h)))
        self.uses_rccl = bool(lib().mods_multi_uses_rccl(self.h))

    def match_ladder(self, img1, img2, steps, params=None, min_matches=15, max_matches=0):
        a = np.ascontiguousarray(img1, np.float32); b = np.ascontiguousarray(img2, np.float32)
        params = params or PairParams.default()
        arr = (LadderStep * len(steps))(*steps)
        res = LadderResult()
        m = np.zeros((max(max_matches, 1), 4), np.float64)
        _check(lib().mods_match_ladder_multi(self.h, _fp(a), a.shape[1], a.shape[0], _fp(b), b.shape[1], b.shape[0], arr, len(steps),
                                             min_matches, C.byref(params), C.byref(res),
                                             m.ctypes.data_as(C.c_void_p) if max_matches else None, max_matches))
        return res, m[:min(res.n_inliers, max_matches)]

    def match_ladder_dets(self, img1, img2, det_steps, det_params, params=None, min_matches=15, max_matches=0, groups=None, group_pos=0):
        """mods_match_ladder_groups_multi: the arguments of match_ladder_dets_dev with the images in host memory."""
        a = np.ascontiguousarray(img1, np.float32); b = np.ascontiguousarray(img2, np.float32)
        n_det, n_steps = len(det_steps), max(len(x) for x in det_steps)
        arr = (LadderStep * (n_steps * n_det))()
        for d, steps in enumerate(det_steps):
            for i in range(n_steps):
                st = steps[i] if i < len(steps) and steps[i] is not None else None
                if st is None:
                    st = LadderStep(); st.n_tilts = st.n_scales = -1
                arr[i * n_det + d] = st
        dets = (HessAffParams * n_det)(*det_params)
        params = params or PairParams.default()
        res = LadderResult()
        m = np.zeros((max(max_matches, 1), 4), np.float64)
        garr = None
        if groups is not None:
            garr = (LadderGroup * n_steps)(*[g if g is not None else LadderGroup.make() for g in list(groups) + [None] * (n_steps - len(groups))])
        _check(lib().mods_match_ladder_groups_multi(self.h, _fp(a), a.shape[1], a.shape[0], _fp(b), b.shape[1], b.shape[0], arr, dets, garr, group_pos,
                                                    n_steps, n_det, min_matches, C.byref(params), C.byref(res),
                                                    m.ctypes.data_as(C.c_void_p) if max_matches else None, max_matches))
        return res, m[:min(res.n_inliers, max_matches)]

    def bank(self, image, det=0):
        """Regions of image 1 (0) / 2 (1) of detector `det` after a run."""
        lib().mods_multi_bank_det.restype = C.c_void_p
        hnd = C.c_void_p(lib().mods_multi_bank_det(self.h, image, det))
        n = lib().mods_imgrep_count(hnd)
        out = np.zeros(max(n, 1), REGION_DTYPE)
        if n:
            _check(lib().mods_imgrep_fetch(hnd, 0, n, out.ctypes.data_as(C.c_void_p)))
        return out[:n].copy()

    def verified_lafs(self):
        """mods_multi_verified_lafs: the frames [n][14] of the last run's verified correspondences (its joint list)"""
        return _verified_lafs(lib().mods_multi_verified_lafs, self.h)

    def close(self):
        if self.h:
            lib().mods_multi_destroy(self.h)
            self.h = C.c_void_p()


def multi_assign(areas, n_dev):
    """Host logic of the view sharding: owner device of every view job (largest first onto the least loaded device)."""
    a = np.ascontiguousarray(areas, np.float64)
    owner = np.zeros(len(a), np.int32)
    _check(lib().mods_multi_assign(a.ctypes.data_as(C.c_void_p), len(a), n_dev, owner.ctypes.data_as(C.c_void_p)))
    return owner


def match_verify_reps(ctx, rep1, rep2, fginn_ratio=0.8, params=None, max_matches=0):
    """Pre-extracted mode (mods.cpp:196-229): match + duplicate filter + verification on banks filled by the caller."""
    params = params or PairParams.default()
    res = LadderResult()
    m = np.zeros((max(max_matches, 1), 4), np.float64)
    _check(lib().mods_match_verify_reps(ctx.h, rep1.h, rep2.h, C.c_double(fginn_ratio), C.byref(params), C.byref(res),
                                        m.ctypes.data_as(C.c_void_p) if max_matches else None, max_matches))
    return res, m[:min(res.n_inliers, max_matches)]


def rematch_under_h_dev(ctx, img1_ptr, w1, h1, img2_ptr, w2, h2, H, rep1, rep2, both=0, init_sigma=0.2, do_blur=1, fginn_ratio=0.8,
                        params=None, max_matches=0):
    """mods_rematch_under_h_dev: image 1 seen through the verified H (img1 -> img2) is detected and described, its regions join
    rep1 (both: image 2 through inv(H) joins rep2), and the banks are matched and verified as match_verify_reps does."""
    params = params or PairParams.default()
    Hc = np.ascontiguousarray(H, np.float64).ravel()
    res = LadderResult()
    m = np.zeros((max(max_matches, 1), 4), np.float64)
    _check(lib().mods_rematch_under_h_dev(ctx.h, C.c_void_p(img1_ptr), w1, h1, C.c_void_p(img2_ptr), w2, h2, _vp(Hc), int(both),
                                          C.c_double(init_sigma), int(do_blur), C.byref(params), rep1.h, rep2.h, C.c_double(fginn_ratio),
                                          C.byref(res), m.ctypes.data_as(C.c_void_p) if max_matches else None, max_matches))
    return res, m[:min(res.n_inliers, max_matches)]


# ---- one pair end to end ------------------------------------------------------------------------------
class PairParams(C.Structure):
    _fields_ = [("det", HessAffParams), ("desc", DescribeParams), ("fginn_ratio", C.c_double),
                ("contradDist", C.c_double), ("nn", C.c_int), ("dup_before_ransac", C.c_int),
                ("dup_dist", C.c_double), ("dup_mode", C.c_int), ("ransac", RansacParams)]

    @staticmethod
    def default():
        """build/config_affori_classic.ini + build/iters_HessianSIFT.ini with vector_matcher = linear."""
        return PairParams(HessAffParams.default(), DescribeParams.default(), 0.8, 10.0, 50, 1, 2.0, 1,
                          RansacParams.default())


class PairResult(C.Structure):
    _fields_ = [("n_detected", C.c_int * 2), ("n_described", C.c_int * 2), ("n_tentatives", C.c_int),
                ("n_unique", C.c_int), ("n_inliers", C.c_int), ("ransac_samples", C.c_int), ("ransac_lo", C.c_int),
                ("ransac_rejects", C.c_int), ("H", C.c_double * 9), ("ms_detect_describe", C.c_double),
                ("ms_match", C.c_double), ("ms_duplicates", C.c_double), ("ms_ransac", C.c_double)]


def match_pair_dev(ctx, dev_ptr, w, h, params=None, max_matches=0):
    """Whole hot path on [2][h][w] fp32 images resident in HBM; returns (PairResult, matches[n,4])."""
    params = params or PairParams.default()
    res = PairResult()
    m = np.zeros((max(max_matches, 1), 4), np.float64)
    _check(lib().mods_match_pair_dev(ctx.h, C.c_void_p(dev_ptr), w, h, w, C.byref(params), C.byref(res),
                                     m.ctypes.data_as(C.c_void_p) if max_matches else None, max_matches))
    return res, m[:min(res.n_inliers, max_matches)]


class PinnedBuffer:
    """Page-locked host memory (mods_host_alloc) viewed as a numpy array: uploads from it are asynchronous."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = C.c_void_p()
        _check(lib().mods_host_alloc(C.c_size_t(self.nbytes), C.byref(self.ptr)))
        buf = (C.c_char * self.nbytes).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=self.dtype).reshape(self.shape)

    def close(self):
        if self.ptr:
            self.array = None
            lib().mods_host_free(self.ptr)
            self.ptr = C.c_void_p()


class Pipeline:
    """mods_pipeline_*: GPU workers (detect/describe/match) overlapped with verify workers (duplicate
    filter + LO-RANSAC) across pairs; results in submission order."""

    def __init__(self, device, w, h, params=None, gpu_workers=1, verify_workers=1, pairs_per_batch=1, clahe=None, mutual=0,
                 local_affine=None):
        """clahe: a ClaheParams - 8-bit submissions are equalised with CLAHE on the GPU, fp32 submissions are refused; mutual: the
        mutual check of every search (mods_pipeline_match_mutual: 0, 1 or 2); local_affine: a LocalAffineParams - every list is
        filtered by local affine consistency ahead of the verification (mods_pipeline_local_affine)"""
        self.params = params or PairParams.default()
        self.h = C.c_void_p()
        if clahe is not None:
            self.clahe = clahe
            _check(lib().mods_pipeline_create_clahe(device, w, h, C.byref(self.params), gpu_workers, verify_workers, pairs_per_batch,
                                                    C.byref(self.clahe), C.byref(self.h)))
        else:
            _check(lib().mods_pipeline_create_ex(device, w, h, C.byref(self.params), gpu_workers, verify_workers, pairs_per_batch,
                                                 C.byref(self.h)))
        self.capacity = lib().mods_pipeline_capacity(self.h)
        if mutual:
            try:
                self.set_match_mutual(mutual)
            except ModsError:
                self.close()
                raise
        if local_affine is not None:
            try:
                self.set_local_affine(local_affine)
            except ModsError:
                self.close()
                raise

    def set_local_affine(self, params=None):
        """before the first submit; None switches the filter off"""
        _check(lib().mods_pipeline_local_affine(self.h, C.byref(params) if params is not None else None))

    def set_match_mutual(self, mode):
        """before the first submit"""
        _check(lib().mods_pipeline_match_mutual(self.h, int(mode)))

    def set_distractor_db(self, full=None):
        """mods_pipeline_distractor_db: the DescDB every search of the pipeline is vetoed by (None: none), before the first submit"""
        _check(lib().mods_pipeline_distractor_db(self.h, full.h if full is not None else None))
        self._distractor = full

    def set_u8_kernels(self, mask):
        """Context.set_u8_kernels on every GPU worker's context, before the first submit"""
        _check(lib().mods_pipeline_u8_kernels(self.h, int(mask)))

    def u8_strip_calls(self):
        lib().mods_pipeline_u8_strip_calls.restype = C.c_long
        return int(lib().mods_pipeline_u8_strip_calls(self.h))

    def spatial_selection(self, mode=1, robustness=0.9):
        """mods_pipeline_spatial_selection: Context.spatial_selection on every GPU worker's context, before the first submit"""
        _check(lib().mods_pipeline_spatial_selection(self.h, int(mode), C.c_double(robustness)))

    def upscale_input(self, mode=1):
        """mods_pipeline_upscale_input: Context.upscale_input on every GPU worker's context, before the first submit"""
        _check(lib().mods_pipeline_upscale_input(self.h, int(mode)))

    def set_domain_pooling(self, num_scales, start_coef=0.5, end_coef=1.5):
        """mods_pipeline_domain_pooling: Context.set_domain_pooling on every GPU worker's context, before the first submit"""
        _check(lib().mods_pipeline_domain_pooling(self.h, int(num_scales), C.c_double(start_coef), C.c_double(end_coef)))

    def submit(self, dev_ptr, tag=0):
        _check(lib().mods_pipeline_submit(self.h, C.c_void_p(dev_ptr), C.c_long(tag)))

    def submit_host(self, host_ptr, tag=0, u8=False, mask=None):
        """The pair in host memory ([2][h][w] fp32, or 8-bit grey with u8=True): uploaded on the worker's stream.
        mask (8-bit pairs only): the address of the pair's two stacked detection masks ([2][h][w] bytes in host memory, valid as
        long as the images), see Context.set_detection_mask."""
        if mask is not None:
            if not u8:
                raise ValueError("detection masks go with 8-bit pairs (u8=True)")
            _check(lib().mods_pipeline_submit_host_u8_masked(self.h, C.c_void_p(host_ptr), C.c_void_p(mask), C.c_long(tag)))
            return
        fn = lib().mods_pipeline_submit_host_u8 if u8 else lib().mods_pipeline_submit_host
        _check(fn(self.h, C.c_void_p(host_ptr), C.c_long(tag)))

    def next(self):
        res, tag = PairResult(), C.c_long()
        _check(lib().mods_pipeline_next(self.h, C.byref(res), C.byref(tag)))
        return res, tag.value

    def next_matches(self, max_matches=1 << 16):
        """(PairResult, tag, matches[n,4]) of the oldest submitted pair: the verified matches as mods_match_pair_dev returns them."""
        res, tag = PairResult(), C.c_long()
        m = np.zeros((max_matches, 4), np.float64)
        _check(lib().mods_pipeline_next_matches(self.h, C.byref(res), C.byref(tag), m.ctypes.data_as(C.c_void_p), max_matches))
        return res, tag.value, m[:min(res.n_inliers, max_matches)]

    def timing_enable(self, stages):
        mask = 0
        for s in stages:
            mask |= 1 << stage_index(s)
        _check(lib().mods_pipeline_timing_enable(self.h, mask))

    def timing_read(self, stage):
        ms, n, by = C.c_double(), C.c_int(), C.c_double()
        _check(lib().mods_pipeline_timing_read(self.h, stage_index(stage), C.byref(ms), C.byref(n), C.byref(by)))
        return ms.value, n.value, by.value

    def graph_replays(self):
        lib().mods_pipeline_graph_replays.restype = C.c_long
        return int(lib().mods_pipeline_graph_replays(self.h))

    def u8_source_calls(self):
        """batches (warm-up included) that were described from their staged 8-bit images"""
        lib().mods_pipeline_u8_source_calls.restype = C.c_long
        return int(lib().mods_pipeline_u8_source_calls(self.h))

    def cpu_seconds(self, reset=False):
        """(GPU workers, verify workers): CPU seconds their threads spent inside their stages since the last reset"""
        g, v = C.c_double(), C.c_double()
        _check(lib().mods_pipeline_cpu_seconds(self.h, C.byref(g), C.byref(v), 1 if reset else 0))
        return g.value, v.value

    def close(self):
        if self.h:
            lib().mods_pipeline_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
