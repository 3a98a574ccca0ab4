"""-m gpu: [HessianAffine] upscaleInputImage = 1 through the mods command line, on graf1 / graf6 cut down to every second pixel
(400 x 320, the small images a doubled first octave is for): the keypoint files hold the regions the library gives with
mods_ctx_upscale_input on, and more of them than the same run without the key."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = os.path.join(ROOT, "mods-light-zmq_amd", "mods")
CFG = os.path.join(ROOT, "tests", "configs")
GRAF = [os.path.join(ROOT, "tests", "golden", n) for n in ("graf1.png", "graf6.png")]


def _run(out, imgs, config, extra_env=None):
    out.mkdir()
    p = subprocess.run([MODS, imgs[0], imgs[1], "o1.png", "o2.png", "k1.txt", "k2.txt", "m.txt", "log.txt", "0", "0", "H.txt",
                        os.path.join(CFG, config), os.path.join(CFG, "iters_one_view.ini")], cwd=out,
                       env=dict(os.environ, MODS_RANSAC_SEED="4242", **(extra_env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return [(out / fn).read_text().splitlines() for fn in ("k1.txt", "k2.txt")], p.stderr.decode()


def test_cli_upscale_input(pkg, tmp_path):
    import torch
    thumbs = []
    for k, fn in enumerate(GRAF):
        rgb = np.asarray(Image.open(fn).convert("RGB"))[::2, ::2]
        thumbs.append(str(tmp_path / ("graf%d_half.png" % k)))
        Image.fromarray(np.ascontiguousarray(rgb)).save(thumbs[-1])
    grey = [orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB"))) for fn in thumbs]
    h, w = grey[0].shape
    assert (w, h) == (400, 320) and grey[1].shape == (h, w)
    on, err_on = _run(tmp_path / "on", thumbs, "classic_upscale.ini")
    off, err_off = _run(tmp_path / "off", thumbs, "classic.ini")
    assert "Doubled first octave (upscaleInputImage)" in err_on and "upscaleInputImage" not in err_off
    assert "Note: [HessianAffine] upscaleInputImage" not in err_on          # (one GPU, images given: nothing is ignored)

    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    reps = [pkg.ImgRep(ctx) for _ in range(4)]
    try:
        t = torch.from_numpy(np.stack(grey)).cuda()
        torch.cuda.synchronize()
        steps = [pkg.LadderStep.make((1,), 360.0)]
        for mode, (r1, r2) in ((0, reps[:2]), (1, reps[2:])):
            ctx.upscale_input(mode)
            pkg.ransac_pin_seed(4242)
            pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, r1, r2, pkg.PairParams.default(), max_matches=1 << 16)
        for files, banks in ((off, reps[:2]), (on, reps[2:])):
            for lines, bank in zip(files, banks):
                r = bank.fetch()
                assert lines[1] == "HessianAffine 1" and lines[2] == "RootSIFT %d" % len(r) and len(lines) == 4 + len(r)
                rows = np.array([ln.split() for ln in lines[4:]], float)
                # (the files carry the 6 significant digits of the stream's default format)
                want = np.array([[float("%g" % r[f][i]) for f in ("x", "y", "s", "a11", "a12", "a21", "a22")] for i in range(len(r))])
                assert np.array_equal(rows[:, :7], want) and np.array_equal(rows[:, 8:], r["desc"].astype(float))
        n_off, n_on = [len(b.fetch()) for b in reps[:2]], [len(b.fetch()) for b in reps[2:]]
        print("regions without / with upscaleInputImage:", n_off, n_on)
        assert n_on[0] > n_off[0] > 500 and n_on[1] > n_off[1] > 500
    finally:
        pkg.ransac_pin_seed(-1)
        for r in reps:
            r.close()
        ctx.close()
