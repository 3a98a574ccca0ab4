"""-m gpu: [MatchPropagation] through the mods command line, on the synthetic planar pair of tests/test_gpu_cli_refine.py: off and
absent are the same run to the byte; on, the output file holds more rows than the matches file, every one within modelThreshold of
the written H, while the matches file, the H file, the keypoint files and the log are those of the run without the section; the
section is ignored with a Note in pre-extracted mode, under MODS_DEVICES, under verification type 1 and with guidedMatching, and
every output is then that of the run without the section; a value outside its range, or doPropagation = 1
without an output file, is an error before an image is opened."""
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
THR = 1.5
ON = "[MatchPropagation]\ndoPropagation = 1;\ncell = 4;\nreach = 1;\nrounds = 8;\nradius = 5;\nminZNCC = 0.8;\nmaxShift = 3.0;\nuseModel = 1;\n" \
     "modelThreshold = %g;\noutput = prop.txt;\n" % THR


def _config(path, section, edit=None):
    ini = open(os.path.join(CFG, "classic.ini")).read()
    path.write_text((edit(ini) if edit else ini) + "\n" + section)
    return str(path)


def _run(out, imgs, config, tail=(), check=True, ver="0", env=None):
    out.mkdir(exist_ok=True)
    p = subprocess.run([MODS, imgs[0], imgs[1], "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", ver, "H.txt", config,
                        os.path.join(CFG, "iters_one_view.ini")] + list(tail), cwd=out, env=dict(os.environ, MODS_RANSAC_SEED="4242", **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    if check:
        assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_propagate")
    a, b, H = synth.pair(400, 300, seed=K.PAIR_SEED)
    imgs = []
    for k, im in enumerate((a, b)):
        imgs.append(str(d / ("img%d.png" % k)))
        Image.fromarray(np.repeat(im.astype(np.uint8)[:, :, None], 3, axis=2)).save(imgs[-1])
    cfg_off = _config(d / "off.ini", "[MatchPropagation]\ndoPropagation = 0;\ncell = 8;\noutput = prop.txt;\n")
    cfg_on = _config(d / "on.ini", ON)
    out = {"dir": d, "imgs": imgs, "H": H, "cfg_on": cfg_on}
    for name, cfg in (("absent", os.path.join(CFG, "classic.ini")), ("off", cfg_off), ("on", cfg_on)):
        out[name] = _run(d / name, imgs, cfg).stderr.decode()
    return out


def _same_run(d, one, two):
    for fn in OUTPUTS:
        assert (d / one / fn).read_bytes() == (d / two / fn).read_bytes(), fn
    assert (d / one / "log.txt").read_text().split()[1:] == (d / two / "log.txt").read_text().split()[1:]      # (the first figure is the time)


def test_off_and_absent_are_the_same_to_the_byte(runs):
    d = runs["dir"]
    _same_run(d, "absent", "off")
    assert "ropagation" not in runs["absent"] + runs["off"]
    assert not (d / "off" / "prop.txt").exists() and not (d / "absent" / "prop.txt").exists()


def test_on_writes_the_propagated_rows_and_changes_nothing_else(runs):
    d = runs["dir"]
    _same_run(d, "absent", "on")
    m, p = np.loadtxt(d / "on" / "m.txt"), np.loadtxt(d / "on" / "prop.txt")
    assert p.ndim == 2 and p.shape[1] == 6 and len(p) > len(m) > 100
    Hw = np.loadtxt(d / "on" / "H.txt")
    q = np.c_[p[:, :2], np.ones(len(p))] @ Hw.T
    e = np.hypot(*(q[:, :2] / q[:, 2:] - p[:, 2:4]).T)
    g = np.c_[p[:, :2], np.ones(len(p))] @ runs["H"].T
    eg = np.hypot(*(g[:, :2] / g[:, 2:] - p[:, 2:4]).T)
    print("%d matches, %d propagated rows in %d rounds; distance to the written H %.3f max; to the generating homography %.3f median %.3f max"
          % (len(m), len(p), p[:, 5].max(), e.max(), np.median(eg), eg.max()))
    assert e.max() <= THR
    assert (p[:, 4] >= 0.8).all() and (p[:, 4] <= 1.0 + 1e-9).all() and p[:, 5].min() == 1 and (np.diff(p[:, 5]) >= 0).all()
    lines = runs["on"].splitlines()
    head = [ln for ln in lines if ln.startswith("Match propagation (cell 4, reach 1, radius 5): ")]
    assert len(head) == 1 and ("%d correspondences" % len(p)) in head[0]
    rounds = [ln for ln in lines if ln.startswith("  round ")]
    assert rounds[0] == "  round 0: %d rows tried, %d accepted" % (len(m), int(rounds[0].split()[-2]))
    assert sum(int(ln.split()[-2]) for ln in rounds[1:]) == len(p)


def test_ignored_in_pre_extracted_mode_and_with_guided_matching(runs, tmp_path):
    d = runs["dir"]
    for name, cfg in (("pre_absent", os.path.join(CFG, "classic.ini")), ("pre_on", runs["cfg_on"])):
        _run(d / name, runs["imgs"], os.path.join(CFG, "classic.ini"))  # writes the keypoint files ...
        p = _run(d / name, runs["imgs"], cfg, tail=("1",))             # ... that the pre-extracted mode reads
    err = p.stderr.decode()
    assert "Note: [MatchPropagation] is ignored in pre-extracted mode and with MODS_DEVICES" in err and "Match propagation (" not in err
    assert not (d / "pre_on" / "prop.txt").exists()
    _same_run(d, "pre_absent", "pre_on")
    edit = lambda ini: ini.replace("[Matching]\n", "[Matching]\nguidedMatching = 1\n")
    _run(d / "guided_absent", runs["imgs"], _config(tmp_path / "guided_absent.ini", "", edit))
    err = _run(d / "guided_on", runs["imgs"], _config(tmp_path / "guided_on.ini", ON, edit)).stderr.decode()
    assert "Note: [MatchPropagation] is ignored with guidedMatching" in err and "Match propagation (" not in err
    assert not (d / "guided_on" / "prop.txt").exists()
    _same_run(d, "guided_absent", "guided_on")


def test_ignored_under_mods_devices(runs):
    """the multi-GPU ladder on one GPU taken twice, as tests/test_gpu_distributed.py runs it"""
    d = runs["dir"]
    env = {"MODS_DEVICES": "0,0"}
    _run(d / "multi_absent", runs["imgs"], os.path.join(CFG, "classic.ini"), env=env)
    err = _run(d / "multi_on", runs["imgs"], runs["cfg_on"], env=env).stderr.decode()
    assert "Note: [MatchPropagation] is ignored in pre-extracted mode and with MODS_DEVICES" in err and "Match propagation (" not in err
    assert not (d / "multi_on" / "prop.txt").exists()
    _same_run(d, "multi_absent", "multi_on")
    assert len((d / "multi_on" / "m.txt").read_text().splitlines()) > 100


def test_ignored_under_verification_type_1(runs):
    """the ground-truth verification: H.txt holds the generating homography when the run starts"""
    d = runs["dir"]
    for name, cfg in (("gt_absent", os.path.join(CFG, "classic.ini")), ("gt_on", runs["cfg_on"])):
        (d / name).mkdir(exist_ok=True)
        np.savetxt(d / name / "H.txt", runs["H"])
        err = _run(d / name, runs["imgs"], cfg, ver="1").stderr.decode()
    assert "Note: [MatchPropagation] is ignored unless RANSAC or ORSA verifies (verification type 0 or 2)" in err and "Match propagation (" not in err
    assert "Ground truth verification is used" in err
    assert not (d / "gt_on" / "prop.txt").exists()
    _same_run(d, "gt_absent", "gt_on")


@pytest.mark.parametrize("section,part", [("cell = 1;", "cell"), ("cell = 65;", "cell"), ("reach = 0;", "reach"), ("reach = 5;", "reach"), ("rounds = 0;", "rounds"),
                                          ("rounds = 65;", "rounds"), ("radius = 16;", "radius"), ("minZNCC = 2;", "minZNCC"), ("maxShift = 0;", "maxShift"),
                                          ("useModel = 2;", "useModel"), ("modelThreshold = 0;", "modelThreshold"), ("doPropagation = 2;", "doPropagation"),
                                          ("", "doPropagation = 1 needs output")])
def test_a_value_outside_its_range_is_an_error_before_an_image_is_opened(tmp_path, section, part):
    body = "[MatchPropagation]\n" + ("" if part == "doPropagation" else "doPropagation = 1;\n") + ("" if part.endswith("output") else "output = prop.txt;\n")
    cfg = _config(tmp_path / "bad.ini", body + section + "\n")
    p = _run(tmp_path / "bad", ["no_such_image_1.png", "no_such_image_2.png"], cfg, check=False)
    err = p.stderr.decode()
    assert p.returncode != 0 and ("[MatchPropagation] " + part) in err and "no_such_image" not in err
