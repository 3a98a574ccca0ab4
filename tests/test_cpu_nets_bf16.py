"""No GPU: the CPU reference of the networks' bf16 mode (tests/nets_bf16_ref.py) and the argument checks of the mode's interface
(mods_net_create_ex, the command line's `precision` key)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import nets_bf16_ref as br
import nets_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")


def _torch_bf16(x):
    return torch.tensor(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_bf16_rounding_equals_torch():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.normal(0, 1, 20000), rng.normal(0, 1, 2000) * 10.0 ** rng.uniform(-30, 30, 2000)]).astype(np.float32)
    assert _same_bits(br.bf16(x), _torch_bf16(x))
    # exact ties: a bf16 value plus half of its last place (bit 15 set, nothing below); the even neighbour is below for an even
    # last bit and above for an odd one
    base = (rng.integers(0x0080, 0x7F00, 4000).astype(np.uint32) << 16) | (rng.integers(0, 2, 4000).astype(np.uint32) << 31)
    ties = (base | 0x8000).view(np.float32)
    got = br.bf16(ties).view(np.uint32)
    even = (base >> 16) & 1 == 0
    assert even.any() and (~even).any()
    assert np.array_equal(got[even], base[even]) and np.array_equal(got[~even], base[~even] + 0x10000)
    assert _same_bits(got.view(np.float32), _torch_bf16(ties))
    # just off a tie on either side, and the neighbours of powers of two
    near = np.concatenate([(base | 0x8001).view(np.float32), (base | 0x7FFF).view(np.float32)])
    p2 = np.float32(2.0) ** np.arange(-20, 21, dtype=np.float32)
    near = np.concatenate([near, p2, np.nextafter(p2, np.float32(0)), np.nextafter(p2, np.float32(np.inf)), -p2,
                           p2 * np.float32(1 - 2.0 ** -9), p2 * np.float32(1 + 2.0 ** -8), p2 * np.float32(1 - 2.0 ** -10)])
    assert _same_bits(br.bf16(near), _torch_bf16(near))
    z = br.bf16(np.array([0.0, -0.0], np.float32))
    assert list(z.view(np.uint32)) == [0, 0x80000000]
    assert br.bf16(np.float32(1.00390625)) == 1.0 and br.bf16(np.float32(1.01171875)) == np.float32(1.015625)     # 1 + 2^-8 down, 1 + 3 * 2^-8 up


@pytest.mark.parametrize("kind", nets_ref.KINDS)
def test_folded_weights_reproduce_the_fold(kind):
    """The fold spelled out once more in numpy, element by element as mods_net_create writes it, equals nets_bf16_ref.fold; and a
    convolution with the folded float32 tensors is nets_ref's BatchNorm behind the convolution up to the one rounding of each
    folded value: (9 cin + 1) 2^-24 S, S the sum of the magnitudes (nets_ref.abs_terms)."""
    st = nets_ref.synthetic_state(kind, 3)
    f = br.folded(kind, st)
    for s in range(1, 7):
        i = 3 * (s - 1)
        W, mean, var = st["features.%d.weight" % i], st["features.%d.running_mean" % (i + 1)], st["features.%d.running_var" % (i + 1)]
        wf = np.empty_like(W)
        bf = np.empty_like(mean)
        for co in range(W.shape[0]):
            inv = 1.0 / np.sqrt(np.float64(var[co]) + 1e-5)
            bf[co] = np.float32(-np.float64(mean[co]) * inv)
            wf[co] = (W[co].astype(np.float64) * inv).astype(np.float32)
        assert _same_bits(f[s][1], bf)
        assert _same_bits(f[s][0], wf if s == 1 else br.bf16(wf))
        if s >= 2:
            assert not np.array_equal(f[s][0], wf) and np.max(np.abs(f[s][0] - wf) / np.abs(wf)) <= 2.0 ** -8
        x = br.dense_input(kind, s, 2)
        cin, _, stride, _ = nets_ref.blocks(kind)[s - 1]
        with torch.no_grad():
            y = torch.relu(torch.nn.functional.conv2d(torch.tensor(x).double(), torch.tensor(wf).double(), stride=stride, padding=1)
                           + torch.tensor(bf).double().view(1, -1, 1, 1)).numpy()
        ref = nets_ref.stage(kind, st, s, x)
        bound = (9 * cin + 1) * 2.0 ** -24 * nets_ref.abs_terms(kind, st, s, x)
        assert np.all(np.abs(y - ref) <= bound) and np.abs(y - ref).max() > 0
    if kind == "hardnet":
        W, mean, var = st["features.19.weight"], st["features.20.running_mean"], st["features.20.running_var"]
        inv = 1.0 / np.sqrt(var.astype(np.float64) + 1e-5)
        assert _same_bits(f[7][0], br.bf16((W.astype(np.float64) * inv[:, None, None, None]).astype(np.float32)))
        assert _same_bits(f[7][1], (-mean.astype(np.float64) * inv).astype(np.float32))
    else:
        assert 7 not in f


def test_reference_chain_rounds_between_the_stages():
    """forward_bf16 is the stages chained; the activations it passes on are bf16 values; float32 and float64 differ a little"""
    st = nets_ref.synthetic_state("affnet", 3)
    p = nets_ref.special_patches()[8:11]
    x = p.reshape(3, 1024)
    for s in range(8):
        x = br.stage_bf16("affnet", st, s, x)
        if 1 <= s <= 6:
            assert x.dtype == np.float32 and _same_bits(x, br.bf16(x)) and 0.05 < np.mean(x > 0) < 0.95
            if s == 1:
                assert _same_bits(x, br.bf16(nets_ref.stage("affnet", st, 1, nets_ref.stage("affnet", st, 0, p.reshape(3, 1024)))))
    assert np.array_equal(x, br.forward_bf16("affnet", st, p))
    e = np.max(np.abs(br.forward_bf16("affnet", st, p, torch.float32) - x))
    d = np.max(np.abs(nets_ref.forward("affnet", st, p) - x))
    print("affnet synthetic: float32 against float64 in bf16 mode %.3g, bf16 mode against fp32 mode %.3g" % (e, d))
    assert 0 < e < d < 0.1


def test_create_ex_refuses_an_unknown_precision(pkg):
    """before the device is looked for: this machine need not have one"""
    lib = pkg.lib()
    tensors = pkg.net_tensors("orinet", nets_ref.synthetic_state("orinet", 3))
    ptrs = (C.POINTER(C.c_float) * len(tensors))(*[t.ctypes.data_as(C.POINTER(C.c_float)) for t in tensors])
    sizes = (C.c_size_t * len(tensors))(*[t.size for t in tensors])
    h = C.c_void_p(1)
    lib.mods_last_error.restype = C.c_char_p
    assert lib.mods_net_create_ex(0, 1, ptrs, sizes, len(tensors), 7, C.byref(h)) == -2           # MODS_E_ARG
    assert not h.value
    msg = lib.mods_last_error()
    assert b"precision" in msg and b"7" in msg, msg
    assert lib.mods_net_precision(None) == 0
    with pytest.raises(pkg.ModsError, match="precision"):
        pkg.Net("orinet", nets_ref.synthetic_state("orinet", 3), precision="int8")


def _run_mods(tmp_path, tail):
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    (tmp_path / "c.ini").write_text(open(os.path.join(CFG, "classic.ini")).read() + "\n" + tail)
    return subprocess.run([MODS, "no_such_1.png", "no_such_2.png", "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                           os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("section", ["AffNet", "OriNet", "zmqDescriptor"])
def test_cli_refuses_an_unknown_precision_at_parse_time(pkg, tmp_path, section):
    """neither image exists: the message comes before they are looked for"""
    p = _run_mods(tmp_path, "[%s]\nweights = w.npz\nprecision = int8\n" % section)
    err = p.stderr.decode()
    assert p.returncode == 1 and "precision" in err and "[%s]" % section in err and "int8" in err and "no_such_1.png" not in err, err


def test_cli_notes_a_precision_without_weights(pkg, tmp_path):
    """a valid value passes the parser (the run then stops at the first missing image); without weights= it only gets a note"""
    p = _run_mods(tmp_path, "[OriNet]\nprecision = bf16\n")
    err = p.stderr.decode()
    assert p.returncode == 1 and "no_such_1.png" in err
    assert "Note: [OriNet] precision" in err and "[AffNet]" not in err, err
    p = _run_mods(tmp_path, "")
    assert p.returncode == 1 and "precision" not in p.stderr.decode()


@pytest.mark.parametrize("n", br.HEAD_N)
def test_head_inputs_leave_few_bytes_exempt(n):
    """The GPU test of HardNet's head allows a byte on either side of an integer of 210 (d + 0.45) within 210 * 8 * e_cpu, for at
    most 1 % of the bytes: its inputs keep the reference's own float32 evaluation inside that."""
    st, x, d64, d32, e_cpu = br.head_case(n)
    assert x.shape == (n, 128, 8, 8) and _same_bits(x, br.bf16(x))
    wrong, exempt = nets_ref.check_hardnet_bytes(nets_ref.hardnet_bytes(d32), d64, e_cpu)
    print("n = %d: e_cpu %.3g, exempt share %.3g, bytes std %.1f" % (n, e_cpu, exempt, nets_ref.hardnet_bytes(d64).std()))
    assert 0 < e_cpu and wrong == 0 and exempt <= 0.01
    assert nets_ref.hardnet_bytes(d64).std() > 5
