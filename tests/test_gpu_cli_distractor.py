"""-m gpu: [Matching] distractorDB through the mods command line.  A first run of the program on graf1 / graf6 cut down to every second
pixel writes its keypoint files as .npz; the second run, on the full images, takes the two files as its distractor database
(tests/configs/classic_distractor.ini) and must give what the library gives with a DescDB of the same rows attached - fewer
tentatives than the run without the key, and not none."""
import os
import re
import shutil
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


def _run(out, imgs, config, keys):
    out.mkdir(exist_ok=True)
    p = subprocess.run([MODS, imgs[0], imgs[1], "o1.png", "o2.png", keys[0], keys[1], "m.txt", "log.txt", "0", "0", "H.txt",
                        os.path.join(CFG, config), os.path.join(CFG, "iters_one_view.ini")], cwd=out,
                       env=dict(os.environ, MODS_RANSAC_SEED="4242"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    err = p.stderr.decode()
    tent = int(re.search(r"(\d+) tentatives found", err).group(1))
    unique = int(re.search(r"(\d+) unique tentatives left", err).group(1))
    text = (out / "m.txt").read_text().split()           # (no rows when nothing was verified)
    return err, tent, unique, np.array(text, np.float64).reshape(-1, 4)


def test_cli_distractor_db(pkg, tmp_path):
    import torch
    thumbs = []
    for k, fn in enumerate(GRAF):
        rgb = np.asarray(Image.open(fn).convert("RGB"))[::2, ::2]
        thumbs.append(str(tmp_path / ("graf%d_half.png" % k)))
        Image.fromarray(np.ascontiguousarray(rgb)).save(thumbs[-1])
    # the database files: written by the program itself
    _run(tmp_path / "db", thumbs, "classic.ini", ("db_a.npz", "db_b.npz"))
    on_dir = tmp_path / "on"
    on_dir.mkdir()
    rows = []
    for fn in ("db_a.npz", "db_b.npz"):
        shutil.copy(tmp_path / "db" / fn, on_dir / fn)
        rows.append(np.load(on_dir / fn)["descs"])
        assert rows[-1].dtype == np.uint8 and rows[-1].shape[1] == 128 and len(rows[-1]) > 300
    rows = np.ascontiguousarray(np.concatenate(rows))
    err_on, tent_on, unique_on, m_on = _run(on_dir, GRAF, "classic_distractor.ini", ("k1.txt", "k2.txt"))
    err_off, tent_off, unique_off, m_off = _run(tmp_path / "off", GRAF, "classic.ini", ("k1.txt", "k2.txt"))
    assert "[Matching] distractorDB: %d descriptors" % len(rows) in err_on and "distractorDB" not in err_off
    assert 0 < tent_on < tent_off, (tent_on, tent_off)

    grey = [orc.grey_of_rgb(np.asarray(Image.open(fn).convert("RGB"))) for fn in GRAF]
    h, w = grey[0].shape
    d = pkg.view_ctx_dims(w, h)
    ctx = pkg.Context(0, d[0], d[1], 1)
    db = pkg.DescDB(rows)
    try:
        t = torch.from_numpy(np.stack(grey)).cuda()
        torch.cuda.synchronize()
        steps = [pkg.LadderStep.make((1,), 360.0)]
        for attach, tent, unique, m in ((db, tent_on, unique_on, m_on), (None, tent_off, unique_off, m_off)):
            ctx.set_distractor_db(attach, None)
            r1, r2 = pkg.ImgRep(ctx), pkg.ImgRep(ctx)
            pkg.ransac_pin_seed(4242)
            res, lm = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, r1, r2, pkg.PairParams.default(), max_matches=1 << 16)
            assert (res.n_tentatives, res.n_unique) == (tent, unique), (res.n_tentatives, tent, res.n_unique, unique)
            assert len(m) == res.n_inliers and np.allclose(m, lm, rtol=1e-5, atol=1e-3)      # text output carries 6 significant digits
            r1.close(); r2.close()
    finally:
        pkg.ransac_pin_seed(-1)
        ctx.set_distractor_db(None, None)
        db.close(); ctx.close()
