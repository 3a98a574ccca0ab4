"""CPU tests (no GPU) of the in-process networks (csrc/nets.hip, pkg.Net): the interface is declared and exported, and tensors
that are missing, surplus or wrongly shaped, a network in the wrong slot and an unknown kind are refused before any device call."""
import ctypes as C
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nets.npz")
NAMES = ["mods_net_create", "mods_net_destroy", "mods_net_dim", "mods_net_chunk", "mods_net_forward", "mods_net_forward_dev",
         "mods_ctx_set_builtin_shape", "mods_ctx_set_builtin_orientation", "mods_ctx_set_builtin_descriptor", "mods_test_net_stage"]


def _state(kind):
    g = np.load(GOLDEN)
    return {k[len(kind) + 1:]: g[k] for k in g.files if k.startswith(kind + ".")}


def test_header_and_exports_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "mods_hip.h")).read()
    lib = pkg.lib()
    for n in NAMES:
        assert n + "(" in hdr, n
        assert hasattr(lib, n), n
    assert "MODS_NET_AFFNET = 0, MODS_NET_ORINET = 1, MODS_NET_HARDNET = 2" in hdr
    assert pkg.NET_KINDS == {"affnet": 0, "orinet": 1, "hardnet": 2}
    assert lib.mods_net_chunk() >= 64 and lib.mods_net_dim(None) == 0


def test_tensor_lists_follow_the_architecture(pkg):
    for kind, n, dim in (("affnet", 20, 3), ("orinet", 20, 2), ("hardnet", 21, 128)):
        spec = pkg.net_tensor_spec(kind)
        assert len(spec) == n and pkg.NET_DIMS[kind] == dim
        assert spec[-1][0] == ("features.20.running_var" if kind == "hardnet" else "features.19.bias")
    c = 32
    assert dict(pkg.net_tensor_spec("hardnet"))["features.6.weight"] == (2 * c, c, 3, 3)
    assert dict(pkg.net_tensor_spec("orinet"))["features.19.weight"] == (2, 64, 8, 8)
    # the golden arrays are exactly the tensors of the two small networks, and come out as contiguous float32 in network order
    for kind in ("affnet", "orinet"):
        t = pkg.net_tensors(kind, _state(kind))
        assert [a.shape for a in t] == [s for _, s in pkg.net_tensor_spec(kind)]
        assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in t)
    # a PyTorch state dict carries BatchNorm's batch counters: not tensors of the network
    st = dict(_state("affnet"), **{"features.1.num_batches_tracked": np.zeros((), np.int64)})
    assert len(pkg.net_tensors("affnet", st)) == 20


def test_bad_state_dicts_raise_before_any_device_call(pkg):
    st = _state("affnet")
    missing = {k: v for k, v in st.items() if k != "features.7.running_var"}
    with pytest.raises(pkg.ModsError, match="missing.*features.7.running_var"):
        pkg.Net("affnet", missing)
    with pytest.raises(pkg.ModsError, match="does not have.*features.99.weight"):
        pkg.Net("affnet", dict(st, **{"features.99.weight": np.zeros(3, np.float32)}))
    with pytest.raises(pkg.ModsError, match=r"features.6.weight has shape \(32, 16, 3\), \(32, 16, 3, 3\) expected"):
        pkg.Net("affnet", dict(st, **{"features.6.weight": st["features.6.weight"][..., 0]}))
    with pytest.raises(pkg.ModsError, match="features.19.weight"):
        pkg.Net("orinet", st)                                  # AffNet's head in an OriNet
    with pytest.raises(pkg.ModsError, match="missing"):
        pkg.Net("hardnet", st)
    with pytest.raises(pkg.ModsError, match="unknown network kind"):
        pkg.Net("resnet", st)


def test_kind_has_to_fit_the_slot(pkg):
    """the check runs before the context or the library is touched: a stand-in without a handle is enough"""
    ctx = types.SimpleNamespace()
    for slot, kind in (("shape", "affnet"), ("orientation", "orinet"), ("descriptor", "hardnet")):
        for other in ("affnet", "orinet", "hardnet"):
            if other == kind:
                continue
            with pytest.raises(pkg.ModsError, match="%s slot takes a Net of kind '%s', not '%s'" % (slot, kind, other)):
                getattr(pkg.Context, "set_builtin_" + slot)(ctx, types.SimpleNamespace(kind=other, h=None))


def test_c_entry_points_check_their_arguments(pkg):
    lib = pkg.lib()
    lib.mods_last_error.restype = C.c_char_p
    t = pkg.net_tensors("affnet", _state("affnet"))
    ptrs = (C.POINTER(C.c_float) * len(t))(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in t])
    sizes = (C.c_size_t * len(t))(*[a.size for a in t])
    h = C.c_void_p()
    assert lib.mods_net_create(0, 7, ptrs, sizes, len(t), C.byref(h)) == -2 and b"unknown kind" in lib.mods_last_error()
    assert lib.mods_net_create(0, 0, ptrs, sizes, len(t) - 1, C.byref(h)) == -2 and b"20 tensors" in lib.mods_last_error()
    assert lib.mods_net_create(0, 1, ptrs, sizes, len(t), C.byref(h)) == -2       # AffNet's head has 3 outputs, OriNet's 2
    assert b"tensor 18 of OriNet" in lib.mods_last_error() and not h.value
    bad = (C.c_size_t * len(t))(*[a.size for a in t])
    bad[3] += 1
    assert lib.mods_net_create(0, 0, ptrs, bad, len(t), C.byref(h)) == -2 and b"tensor 3 of AffNet" in lib.mods_last_error()
    if lib.mods_device_count() == 0:              # well-formed tensors: only now the device is looked for, and there is no CPU path
        assert lib.mods_net_create(0, 0, ptrs, sizes, len(t), C.byref(h)) == -1 and b"no CPU path" in lib.mods_last_error()
    assert lib.mods_net_forward(None, None, 1, 0, None) == -2
    assert lib.mods_ctx_set_builtin_shape(None, None, C.c_double(5.0), 1) == -2
    lib.mods_net_destroy.restype = None
    lib.mods_net_destroy(None)
