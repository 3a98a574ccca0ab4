"""Domain-size pooling of SIFT descriptors (mods_ctx_domain_pooling) without a GPU: the numpy restatement (tests/dsp_ref.py) pinned,
with one patch and no pooling, to the CPU oracle's descriptor byte for byte; the coefficient arithmetic; the refusals that need no
device; the command line's [SIFTDescriptor] domainSizePooling / numScales / startCoef / endCoef; the header's declarations."""
import os
import subprocess

import numpy as np
import pytest

import dsp_ref
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")


@pytest.fixture(scope="module")
def graf_patches():
    """description patches of 240 regions of graf1 spread over the response order, with and without photometric normalisation"""
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "graf1.png")).convert("L"), np.float32)
    regs, _ = orc.detect_describe(img)
    assert len(regs) > 1000
    pick = regs[np.linspace(0, len(regs) - 1, 240).astype(int)]
    raw = [orc.extract_desc_patch(img, pick[i:i + 1], photonorm=False) for i in range(len(pick))]
    normed = [orc.extract_desc_patch(img, pick[i:i + 1], photonorm=True) for i in range(len(pick))]
    return pick, raw, normed


def _synthetic(ps=41):
    yy, xx = np.mgrid[0:ps, 0:ps].astype(np.float32)
    step = np.where(xx < ps // 2, 40.0, 200.0).astype(np.float32)
    dot = np.zeros((ps, ps), np.float32)
    dot[ps // 2 - 3, ps // 2 + 5] = 255.0
    ramp = (3.0 * xx + 1.5 * yy).astype(np.float32)
    diag = np.where(xx + yy < ps, 10.0, 250.0).astype(np.float32)
    rng = np.random.RandomState(5)
    noise = rng.randint(0, 256, (ps, ps)).astype(np.float32)
    return dict(step=step, dot=dot, ramp=ramp, diag=diag, noise=noise)


@pytest.mark.parametrize("rootsift", [True, False])
def test_restatement_equals_the_oracle_on_graf_patches(graf_patches, rootsift):
    """one patch, no pooling: raw histogram + tail = orc.sift_desc, on the normalised patches the describe stage feeds it; the
    descriptors of the RootSIFT branch are also the ones the oracle's whole describe call gave those regions"""
    pick, _, normed = graf_patches
    assert len(normed) >= 200
    for i, p in enumerate(normed):
        want = orc.sift_desc(p, rootsift, 0.2)
        got = dsp_ref.tail(dsp_ref.raw_histogram(p), rootsift, 0.2)
        assert np.array_equal(got, want), (i, np.nonzero(got != want)[0][:8])
        if rootsift:
            assert np.array_equal(want, pick["desc"][i])


@pytest.mark.parametrize("rootsift", [True, False])
@pytest.mark.parametrize("name", ["step", "dot", "ramp", "diag", "noise"])
def test_restatement_equals_the_oracle_on_synthetic_patches(name, rootsift):
    p = _synthetic()[name]
    for max_bin in (0.2, 0.05, 1.0):
        want = orc.sift_desc(p, rootsift, max_bin)
        assert want.any()
        assert np.array_equal(dsp_ref.tail(dsp_ref.raw_histogram(p), rootsift, max_bin), want), (name, max_bin)


def test_restatement_at_another_patch_size():
    rng = np.random.RandomState(9)
    for ps in (33, 45, 47):
        p = rng.randint(0, 256, (ps, ps)).astype(np.float32)
        assert np.array_equal(dsp_ref.tail(dsp_ref.raw_histogram(p), True, 0.2), orc.sift_desc(p, True, 0.2)), ps


def test_photonorm_restatement_equals_the_oracle(graf_patches):
    """dsp_ref.photonorm (used where a test hands raw patches to mods_test_sift_pooled) on the raw patches = the oracle's normalised ones"""
    _, raw, normed = graf_patches
    for i in range(0, len(raw), 4):
        assert np.array_equal(dsp_ref.photonorm(raw[i]), normed[i]), i
    flat = np.full((41, 41), 77.0, np.float32)
    assert np.array_equal(dsp_ref.photonorm(flat), flat)


def test_half_fold_and_pooling_order():
    rng = np.random.RandomState(3)
    h = [rng.rand(128) * 10 ** rng.randint(-3, 4) for _ in range(4)]
    p = _synthetic()
    got = dsp_ref.pooled_histogram([p["step"], p["ramp"], p["noise"]])
    a, b, c = (dsp_ref.raw_histogram(p[k]) for k in ("step", "ramp", "noise"))
    assert np.array_equal(got, (a + b) + c)
    full = dsp_ref.tail(h[0], True, 0.2)
    half = dsp_ref.tail(h[0], True, 0.2, half=True)
    assert half[64:].max() == 0 and half[:64].any() and full[64:].any()
    # K equal patches: the L2 normalisation removes the factor K when K is a power of two (exact scaling)
    one = dsp_ref.pooled_descriptor([p["noise"]])
    assert np.array_equal(dsp_ref.pooled_descriptor([p["noise"]] * 2), one) and np.array_equal(dsp_ref.pooled_descriptor([p["noise"]] * 4), one)


def test_coefficients():
    assert dsp_ref.coefficients(2, 1.0, 2.0) == [1.0, 2.0]
    assert dsp_ref.coefficients(3, 0.5, 1.5) == [0.5, 1.0, 1.5]
    c8 = dsp_ref.coefficients(8, 0.5, 4.0)
    assert len(c8) == 8 and c8[0] == 0.5 and c8 == [0.5 + k * (3.5 / 7) for k in range(8)] and c8[-1] == 4.0
    c = dsp_ref.coefficients(8, 0.3, 1.7)
    step = (1.7 - 0.3) / 7
    assert c == [0.3 + k * step for k in range(8)]          # start + k * step, not a running sum
    assert abs(c[-1] - 1.7) < 1e-15


def test_setters_refuse_bad_values_without_a_device(pkg):
    import ctypes as C
    lib = pkg.lib()
    ctx = C.c_void_p(0x1000)        # never dereferenced: the values are checked first
    d = C.c_double
    bad = [(9, 0.5, 1.5, b"numScales"), (-1, 0.5, 1.5, b"numScales"), (3, 0.0, 1.5, b"startCoef"), (3, -0.5, 1.5, b"startCoef"),
           (3, float("nan"), 1.5, b"startCoef"), (3, 1.5, 1.5, b"endCoef"), (3, 1.5, 0.5, b"endCoef"), (3, 0.5, 4.5, b"endCoef"),
           (3, 0.5, float("nan"), b"endCoef"), (3, 0.5, float("inf"), b"endCoef"), (3, float("inf"), 1.5, b"startCoef")]
    for K, a, b, word in bad:
        assert lib.mods_ctx_domain_pooling(ctx, K, d(a), d(b)) == -2 and word in lib.mods_last_error(), (K, a, b)
    assert lib.mods_ctx_domain_pooling(None, 3, d(0.5), d(1.5)) == -2 and b"null context" in lib.mods_last_error()
    assert lib.mods_pipeline_domain_pooling(None, 3, d(0.5), d(1.5)) == -2 and b"null pipeline" in lib.mods_last_error()
    assert lib.mods_ctx_domain_pooling_get(None, None, None, None) == -2
    assert lib.mods_test_sift_pooled(None, None, 3, 41, 1, 0, 0, d(0.2), None) == -2


def _run_cli(tmp_path, lines):
    assert os.path.exists(MODS), "mods CLI not built (make -C mods-light-zmq_amd)"
    ini = open(os.path.join(CFG, "classic.ini")).read()
    assert "[SIFTDescriptor]\n" in ini
    (tmp_path / "c.ini").write_text(ini.replace("[SIFTDescriptor]\n", "[SIFTDescriptor]\n" + "\n".join(lines) + "\n"))
    return subprocess.run([MODS, "no_such_1.png", "no_such_2.png", "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                           os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("lines,key", [(["numScales = 9"], "numScales"), (["numScales = -1"], "numScales"), (["startCoef = 0"], "startCoef"),
                                       (["startCoef = 1.5", "endCoef = 1.5"], "endCoef"), (["startCoef = 1.0", "endCoef = 0.5"], "endCoef"),
                                       (["endCoef = 4.5"], "endCoef")])
def test_cli_rejects_bad_pooling_values_at_parse_time(pkg, tmp_path, lines, key):
    """with the gate on; before the images are read and before any device call: neither image exists"""
    p = _run_cli(tmp_path, ["domainSizePooling = 1"] + lines)
    err = p.stderr.decode()
    assert p.returncode == 1 and "[SIFTDescriptor] " + key in err and "no_such_1.png" not in err, err


def test_cli_rejects_pooling_with_fast_extraction(pkg, tmp_path):
    ini = open(os.path.join(CFG, "classic.ini")).read()
    assert "FastPatchExtraction=false\n" in ini
    (tmp_path / "c.ini").write_text(ini.replace("FastPatchExtraction=false\n", "FastPatchExtraction=true\ndomainSizePooling = 1\n"))
    p = subprocess.run([MODS, "no_such_1.png", "no_such_2.png", "o1", "o2", "k1", "k2", "m", "log", "0", "0", "H", str(tmp_path / "c.ini"),
                        os.path.join(CFG, "iters_one_view.ini")], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and "domainSizePooling" in err and "FastPatchExtraction" in err and "no_such_1.png" not in err, err


@pytest.mark.parametrize("lines", [["domainSizePooling = 1"], ["domainSizePooling = 1", "numScales = 8", "startCoef = 0.5", "endCoef = 4"],
                                   ["numScales = 9", "startCoef = 0", "endCoef = -1"],
                                   ["domainSizePooling = 0", "numScales = 9", "startCoef = 0", "endCoef = -1"]])
def test_cli_accepts_pooling_and_ignores_the_keys_behind_a_closed_gate(pkg, tmp_path, lines):
    """valid values get past the parser (the run then stops at the first missing image); with the gate 0 or absent the reference's
    three keys are ignored whatever they hold, as the reference ignores them"""
    p = _run_cli(tmp_path, lines)
    err = p.stderr.decode()
    assert p.returncode == 1 and "no_such_1.png" in err and "SIFTDescriptor" not in err, err


def test_header_declares_the_interface():
    hdr = open(os.path.join(ROOT, "include", "mods_hip.h")).read()
    for decl in ("int mods_ctx_domain_pooling(mods_ctx *ctx, int numScales, double startCoef, double endCoef);",
                 "int mods_ctx_domain_pooling_get(const mods_ctx *ctx, int *numScales, double *startCoef, double *endCoef);",
                 "int mods_pipeline_domain_pooling(mods_pipeline *p, int numScales, double startCoef, double endCoef);",
                 "int mods_test_sift_pooled(mods_ctx *ctx, const float *patches, int K, int ps, int rootsift, int half, int photoNorm, double maxBinValue,"):
        assert decl in hdr, decl
