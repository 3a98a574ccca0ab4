"""-m gpu: [MatchRefinement] through the mods command line, on the synthetic planar pair of tests/test_gpu_lsm.py written as PNG files:
off and absent are the same run to the byte; on, the matches file keeps its rows and takes refined coordinates, the verbose line
appears and the H file takes the refit model; the section is ignored with a Note in pre-extracted mode; a value outside its range
is an error before an image is opened."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import lsm_cases as K
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
OUTPUTS = ("m.txt", "H.txt", "k1.txt", "k2.txt")


def _config(path, section):
    path.write_text(open(os.path.join(CFG, "classic.ini")).read() + "\n" + section)
    return str(path)


def _run(out, imgs, config, tail=(), check=True):
    out.mkdir(exist_ok=True)
    p = subprocess.run([MODS, imgs[0], imgs[1], "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt", config,
                        os.path.join(CFG, "iters_one_view.ini")] + list(tail), cwd=out, env=dict(os.environ, MODS_RANSAC_SEED="4242"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    if check:
        assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_refine")
    a, b, H = synth.pair(400, 300, seed=K.PAIR_SEED)
    imgs = []
    for k, im in enumerate((a, b)):
        imgs.append(str(d / ("img%d.png" % k)))
        Image.fromarray(np.repeat(im.astype(np.uint8)[:, :, None], 3, axis=2)).save(imgs[-1])
    cfg_off = _config(d / "off.ini", "[MatchRefinement]\ndoRefinement = 0;\nradius = 7;\n")
    cfg_on = _config(d / "on.ini", "[MatchRefinement]\ndoRefinement = 1;\nradius = 10;\nmaxIter = 20;\nminZNCC = 0.8;\nmaxShift = 3.0;\naffine = 1;\nrefitModel = 1;\n")
    out = {"dir": d, "imgs": imgs, "H": H, "cfg_on": cfg_on}
    for name, cfg in (("absent", os.path.join(CFG, "classic.ini")), ("off", cfg_off), ("on", cfg_on)):
        out[name] = _run(d / name, imgs, cfg).stderr.decode()
    return out


def test_off_and_absent_are_the_same_to_the_byte(runs):
    d = runs["dir"]
    for fn in OUTPUTS:
        assert (d / "absent" / fn).read_bytes() == (d / "off" / fn).read_bytes(), fn
    assert (d / "absent" / "log.txt").read_text().split()[1:] == (d / "off" / "log.txt").read_text().split()[1:]      # (the first figure is the time)
    assert "Match refinement" not in runs["absent"] + runs["off"] and "MatchRefinement" not in runs["absent"] + runs["off"]


def test_on_refines_the_rows_and_refits_the_model(runs):
    d = runs["dir"]
    m0, m1 = np.loadtxt(d / "off" / "m.txt"), np.loadtxt(d / "on" / "m.txt")
    assert m0.shape == m1.shape and len(m0) > 100
    assert (m0 != m1).any(axis=1).mean() > 0.9                        # nearly every row moved ...
    assert np.abs(m0 - m1).max() <= 3.0 + 1e-3                        # ... by no more than maxShift (+ the 6 digits of the file)
    assert not ((m0[:, :2] != m1[:, :2]).any(axis=1) & (m0[:, 2:] != m1[:, 2:]).any(axis=1)).any()       # ... on one side only
    line = [ln for ln in runs["on"].splitlines() if ln.startswith("Match refinement (radius 10): ")]
    assert len(line) == 1 and ("%d correspondences" % len(m0)) in line[0] and " ok," in line[0] and "model refit" in line[0]
    H0, H1 = np.loadtxt(d / "off" / "H.txt"), np.loadtxt(d / "on" / "H.txt")
    assert H0.shape == H1.shape == (3, 3) and not np.array_equal(H0, H1)
    # the log row's counts do not change; the keypoint files are the same
    assert (d / "off" / "log.txt").read_text().split()[1:] == (d / "on" / "log.txt").read_text().split()[1:]
    for fn in ("k1.txt", "k2.txt"):
        assert (d / "off" / fn).read_bytes() == (d / "on" / fn).read_bytes()
    # a condition, not an accuracy figure: the rows sit closer to the generating homography than before
    def err(m):
        p = np.c_[m[:, :2], np.ones(len(m))] @ runs["H"].T
        return np.hypot(*(p[:, :2] / p[:, 2:] - m[:, 2:]).T)
    print("median transfer error of the matches file: %.3f -> %.3f px" % (np.median(err(m0)), np.median(err(m1))))
    assert np.median(err(m1)) < np.median(err(m0))


def test_pre_extracted_mode_ignores_the_section_with_a_note(runs):
    d = runs["dir"]
    before = (d / "on" / "m.txt").read_bytes()
    p = _run(d / "on", runs["imgs"], runs["cfg_on"], tail=("1",))
    err = p.stderr.decode()
    assert "Note: [MatchRefinement] is ignored in pre-extracted mode and with MODS_DEVICES" in err and "Match refinement (" not in err
    assert (d / "on" / "m.txt").read_bytes() != before                # the unrefined rows


@pytest.mark.parametrize("section,part", [("radius = 16;", "radius"), ("radius = 0;", "radius"), ("maxIter = 0;", "maxIter"), ("minZNCC = 2;", "minZNCC"),
                                          ("maxShift = 0;", "maxShift"), ("affine = 3;", "affine"), ("doRefinement = 2;", "doRefinement"),
                                          ("refitModel = -1;", "refitModel")])
def test_a_value_outside_its_range_is_an_error_before_an_image_is_opened(tmp_path, section, part):
    cfg = _config(tmp_path / "bad.ini", "[MatchRefinement]\n" + ("" if part == "doRefinement" else "doRefinement = 1;\n") + section + "\n")
    p = _run(tmp_path / "bad", ["no_such_image_1.png", "no_such_image_2.png"], cfg, check=False)
    err = p.stderr.decode()
    assert p.returncode != 0 and ("[MatchRefinement] " + part) in err and "no_such_image" not in err
