"""CPU tests (no GPU) of tests/nets_ref.py, the float64 reference the network kernels are compared with stage by stage
(tests/test_gpu_nets_stages.py): it reproduces the reference project's own outputs for its trained weights, its stages compose to
the whole, and its HardNet is the daemon's model."""
import os

import numpy as np
import pytest
import torch

import nets_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nets.npz")


def _golden_state(kind):
    g = np.load(GOLDEN)
    return {k[len(kind) + 1:]: g[k] for k in g.files if k.startswith(kind + ".")}


@pytest.mark.parametrize("kind", ["affnet", "orinet"])
def test_forward_reproduces_the_golden_outputs(kind):
    g = np.load(GOLDEN)
    got = nets_ref.forward(kind, _golden_state(kind), g["patches"])
    assert got.dtype == np.float64 and got.shape == g[kind + "_out"].shape
    err = np.max(np.abs(got - g[kind + "_out"]))
    e32 = np.max(np.abs(nets_ref.forward32(kind, _golden_state(kind), g["patches"]) - got))
    print("%s: float64 reference against the golden outputs %.3g, float32 evaluation against float64 %.3g" % (kind, err, e32))
    assert err <= 1e-6
    assert 0 < e32 <= 1e-5          # the float32 evaluation is one, and it is an evaluation of the same network


@pytest.mark.parametrize("kind", nets_ref.KINDS)
def test_stages_compose_to_forward(kind):
    st = nets_ref.synthetic_state(kind, 3)
    p = nets_ref.special_patches()[[0, 3, 9, 12, 20]]
    for dtype in (torch.float64, torch.float32):
        for quantise in (False, True):
            x = p.reshape(len(p), 1024)
            for s in range(8):
                assert x.shape[1:] == nets_ref.in_shape(kind, s) or s in (0, 7)
                x = nets_ref.stage(kind, st, s, x, dtype, quantise)      # (quantise concerns stage 0 alone)
                assert x.shape[1:] == nets_ref.out_shape(kind, s) and x.dtype == (np.float64 if dtype == torch.float64 else np.float32)
            assert np.array_equal(x, nets_ref.forward(kind, st, p, dtype, quantise))
    assert not np.array_equal(nets_ref.forward(kind, st, p, quantise=True), nets_ref.forward(kind, st, p, quantise=False))
    q = np.clip(np.rint(p), 0, 255)
    assert np.array_equal(nets_ref.forward(kind, st, p, quantise=True), nets_ref.forward(kind, st, q))


def test_abs_terms_bound_the_stage():
    """S is the sum of magnitudes: it dominates the pre-activation, and equals it where nothing cancels"""
    kind, st = "affnet", nets_ref.synthetic_state("affnet", 3)
    rng = np.random.default_rng(0)
    for s in range(1, 7):
        x = rng.normal(0, 1, (2,) + nets_ref.in_shape(kind, s))
        S = nets_ref.abs_terms(kind, st, s, x)
        y = nets_ref.stage(kind, st, s, x)
        assert S.shape == y.shape and np.all(S >= y - 1e-12) and np.all(S > 0)
    pos = {k: (np.abs(v) if k.endswith("weight") else -np.abs(v) if k.endswith("running_mean") else v) for k, v in st.items()}
    x = np.abs(rng.normal(0, 1, (2,) + nets_ref.in_shape(kind, 3)))
    assert np.allclose(nets_ref.abs_terms(kind, pos, 3, x), nets_ref.stage(kind, pos, 3, x), rtol=1e-13, atol=0)


def test_synthetic_states_use_every_bias():
    """running_var in [0.5, 2], running_mean of the activations' size: each block's ReLU keeps some and drops some of every patch"""
    for kind in nets_ref.KINDS:
        st = nets_ref.synthetic_state(kind, 3)
        x = nets_ref.stage(kind, st, 0, nets_ref.special_patches()[9:14])
        for s in range(1, 7):
            x = nets_ref.stage(kind, st, s, x)
            share = np.mean(x > 0)
            assert 0.2 < share < 0.8, (kind, s, share)
            var, mean = st["features.%d.running_var" % (3 * s - 2)], st["features.%d.running_mean" % (3 * s - 2)]
            assert var.min() >= 0.5 and var.max() <= 2.0 and np.abs(mean).max() > 0.1
        out = nets_ref.stage(kind, st, 7, x)
        assert np.all(np.isfinite(out)) and out.std() > 0.01
        if kind != "hardnet":
            assert np.abs(out - (np.array([1.0, 0.0, 1.0]) if kind == "affnet" else 0.0)).max() < 0.999      # tanh not saturated


def test_hardnet_is_the_daemons_model():
    from test_gpu_nets import _module_of, _zd, hardnet_state
    p = np.concatenate([np.load(GOLDEN)["patches"][:12].astype(np.float32), nets_ref.special_patches()[[0, 3, 4, 8, 9, 12]]])
    for st in (hardnet_state(5), nets_ref.synthetic_state("hardnet", 3)):
        model = _module_of(_zd().build_model("hardnet", st, 0, "cpu")).double()
        with torch.no_grad():
            d = model(torch.from_numpy(p.astype(np.float64)).view(-1, 1, 32, 32)).numpy()
        want = np.clip(210 * (d + 0.45), 0, 255).astype(np.uint8)                   # zmq_daemon.py's quantisation
        mine = nets_ref.forward("hardnet", st, p)
        assert np.max(np.abs(mine - d)) < 1e-13
        assert np.array_equal(nets_ref.hardnet_bytes(mine), want.astype(np.float64))
        assert want.std() > 5
        wrong, exempt = nets_ref.check_hardnet_bytes(want, mine, 1e-9)
        assert wrong == 0 and exempt < 1e-3
        assert nets_ref.check_hardnet_bytes(np.where(want > 100, want - 1, want), mine, 1e-9)[0] > 0
