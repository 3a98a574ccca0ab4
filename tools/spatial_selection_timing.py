#!/usr/bin/env python3
"""The spatial selection of the count modes' cut (mods_ctx_spatial_selection; csrc/spatial_select.hip) measured on an MI355X:
  - its three launches (stage `spatial_select`, HIP events of the context) beside the SORT stage of the same calls, for one 1080p
    image and a 16-image 1080p batch through mods_detect_hessian_affine_dev, FixedRegNumber 500 / 2000 / 5000 of the candidates
    those images give;
  - detect + describe of the 16-image batch with the selection off, by the host clock (the call ends in a synchronise), this build
    against another build of the library (the parent commit's, --against) in alternating fresh processes;
  - graf1 / graf6 through mods_match_pair_dev (one view, homography, pinned RANSAC seed), FixedRegNumber 500 / 1000 / 2000 with the
    selection off and on: tentatives, verified inliers, RANSAC samples.
  python tools/spatial_selection_timing.py [reps] [--against PARENT.so]   the report (profiles/spatial_selection_timing.txt)
  python tools/spatial_selection_timing.py [reps] --one CASE              one run in this process: a JSON line"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, N_IMG, ROUNDS = 1920, 1080, 16, 3
KEEPS = (500, 2000, 5000)
GRAF_KEEPS = (500, 1000, 2000)
ROBUSTNESS = 0.9


def images():
    import synth
    base = [synth.texture(W, H, seed=s) for s in (0, 1)]
    out = []
    for k in range(N_IMG):                      # 16 different images from two textures: flips and row shifts
        im = base[k & 1]
        if k & 2:
            im = im[:, ::-1]
        if k & 4:
            im = im[::-1]
        out.append(np.roll(im, 37 * (k >> 3), axis=0))
    return np.ascontiguousarray(np.stack(out), np.float32)


def one_stage(reps):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    t = torch.from_numpy(images()).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, W, H, N_IMG)
    rows = []
    for n_img in (1, N_IMG):
        par = pkg.HessAffParams.default()
        par.mode, par.regionsNumber = 2, 10 ** 6
        cand = ctx.detect_hessian_affine_dev(t.data_ptr(), n_img, W, H, par, fetch=False)
        for keep in KEEPS:
            par.regionsNumber = keep
            ms = {}
            for on in (0, 1):
                ctx.spatial_selection(on, ROBUSTNESS)
                call = lambda: ctx.detect_hessian_affine_dev(t.data_ptr(), n_img, W, H, par, fetch=False)
                ctx.timing_enable(["sort", "spatial_select"]); call(); call(); ctx.timing_reset()
                for _ in range(reps):
                    call()
                ms[on] = {s: ctx.timing_read(s)[0] / reps for s in ("sort", "spatial_select")}
                ctx.timing_enable([])
            ctx.spatial_selection(0)
            rows.append({"n_img": n_img, "keep": keep, "cand_min": int(min(cand)), "cand_max": int(max(cand)), "sort_off": ms[0]["sort"],
                         "sort_on": ms[1]["sort"], "select_on": ms[1]["spatial_select"], "select_off": ms[0]["spatial_select"]})
    print(json.dumps({"rows": rows}))
    ctx.close()


def one_call(reps):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    t = torch.from_numpy(images()).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, W, H, N_IMG)
    call = lambda: ctx.detect_describe_dev(t.data_ptr(), N_IMG, W, H)
    call(); nd, nr = call()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    print(json.dumps({"call_ms": (time.perf_counter() - t0) / reps * 1e3, "regions": int(sum(nr))}))
    ctx.close()


def one_graf():
    import torch
    import __graft_entry__ as ge
    import orc
    from PIL import Image
    pkg = ge.load_package()
    # (B + G + R) / 3.0 as the command line reads a colour image
    a, b = (orc.grey_of_rgb(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", fn)).convert("RGB"))) for fn in ("graf1.png", "graf6.png"))
    h, w = a.shape
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, w, h, 2)
    rows = []
    for keep in GRAF_KEEPS:
        par = pkg.PairParams.default()
        par.det.mode, par.det.regionsNumber = 2, keep
        for on in (0, 1):
            ctx.spatial_selection(on, ROBUSTNESS)
            pkg.ransac_pin_seed(4242)
            res, _ = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, par)
            rows.append({"keep": keep, "on": on, "described": list(res.n_described), "tentatives": res.n_tentatives, "unique": res.n_unique,
                         "inliers": res.n_inliers, "samples": res.ransac_samples})
    print(json.dumps({"rows": rows}))
    ctx.close()


def spawn(case, reps, lib=None):
    env = dict(os.environ)
    if lib:
        env["MODS_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(reps), "--one", case], env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode or not lines:
        raise SystemExit("run of case %s failed:\n%s" % (case, (p.stdout + p.stderr)[-2000:]))
    return json.loads(lines[-1])


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args and args[0].isdigit() else 20
    if "--one" in args:
        case = args[args.index("--one") + 1]
        return {"stage": lambda: one_stage(reps), "call": lambda: one_call(reps), "graf": one_graf}[case]()
    other = args[args.index("--against") + 1] if "--against" in args else None
    out = ["spatial selection (ANMS, robustness %.1f) on %d x %d images, mods_detect_hessian_affine_dev, FixedRegNumber; ms per call, HIP events of"
           % (ROBUSTNESS, W, H), "the context, %d calls; SORT: rank + export (+ the prefix cut when the selection is off); SELECT: radius + rank + compaction" % reps, "",
           "%-7s %-7s %-19s %-10s %-10s %-10s %-12s" % ("images", "keep", "candidates / image", "SORT off", "SORT on", "SELECT on", "SELECT off")]
    for r in spawn("stage", reps)["rows"]:
        out.append("%-7d %-7d %-19s %-10.4f %-10.4f %-10.4f %-12.4f" % (r["n_img"], r["keep"], "%d .. %d" % (r["cand_min"], r["cand_max"]), r["sort_off"],
                                                                   r["sort_on"], r["select_on"], r["select_off"]))
    runs = {"this build": [], "parent": []}
    for _ in range(ROUNDS):
        runs["this build"].append(spawn("call", reps))
        if other:
            runs["parent"].append(spawn("call", reps, other))
    out += ["", "detect + describe of the %d-image batch, selection off (FixedTh), host clock, ms per call; %d rounds of fresh processes, alternating" % (N_IMG, ROUNDS)]
    for name, rs in runs.items():
        if rs:
            v = [r["call_ms"] for r in rs]
            out.append("%-11s %s   median %.3f, spread (max - min) %.3f, %d regions" % (name, " ".join("%.3f" % x for x in v), float(np.median(v)), max(v) - min(v), rs[0]["regions"]))
    out += ["", "graf1 / graf6 (tests/golden, 800 x 640), mods_match_pair_dev: one view, homography, RANSAC seed pinned",
            "%-7s %-10s %-14s %-11s %-8s %-8s %-8s" % ("keep", "selection", "described", "tentatives", "unique", "inliers", "samples")]
    for r in spawn("graf", reps)["rows"]:
        out.append("%-7d %-10s %-14s %-11d %-8d %-8d %-8d" % (r["keep"], "on" if r["on"] else "off", "%d / %d" % tuple(r["described"]), r["tentatives"], r["unique"],
                                                        r["inliers"], r["samples"]))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "spatial_selection_timing.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
