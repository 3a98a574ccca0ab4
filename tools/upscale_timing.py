#!/usr/bin/env python3
"""The doubled first octave (mods_ctx_upscale_input; csrc/pyramid.hip) measured on an MI355X, device events throughout (the
context's stage events, and a pair of events around runs of calls that each end in a synchronise):
  - switch off: detect + describe of the 16 x 1080p batch, this build against another build of the library (the parent commit's,
    --against) in alternating fresh processes, with each build's run-to-run spread;
  - switch on: the scale space of that batch (stage `pyramid`: first blur launch to the end of the NMS), the whole detect + describe
    call and the device memory the context grows by, for mode 0, 1 (first level in one launch) and 2 (double, then blur); the sums
    of the stages the first level's launches are charged to (`blur`: the large-tile blur + response launches, `resize`: the
    doubling launch and the decimations) - every launch but the first level's is the same in modes 1 and 2, so the difference of
    the sums is the first level's;
  - does it pay: graf1 / graf6 at every second pixel (400 x 320) and at full size (800 x 640) through mods_match_pair_dev (one
    view, homography, default configuration, pinned RANSAC seed) with and without the switch.
  python tools/upscale_timing.py [reps] [--against PARENT.so]   the report (profiles/upscale_timing.txt)
  python tools/upscale_timing.py [reps] --one CASE              one run in this process: a JSON line"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, N_IMG, ROUNDS = 1920, 1080, 16, 3
STAGES = ("pyramid", "blur", "resize", "blur_small", "response", "nms")


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


def timed(torch, call, reps):
    """ms per call by a pair of device events around `reps` calls (each call ends in a synchronise of the context's stream)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def one_call(reps):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    t = torch.from_numpy(images()).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, W, H, N_IMG)
    call = lambda: ctx.detect_describe_dev(t.data_ptr(), N_IMG, W, H)
    call(); nd, nr = call()
    print(json.dumps({"call_ms": timed(torch, call, reps), "regions": int(sum(nr))}))
    ctx.close()


def one_modes(reps):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    t = torch.from_numpy(images()).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, W, H, N_IMG)
    call = lambda: ctx.detect_describe_dev(t.data_ptr(), N_IMG, W, H)
    rows = []
    for mode in (0, 1, 2, 1, 2):                 # (the second visit of a mode finds every pool grown)
        free0 = torch.cuda.mem_get_info()[0]
        ctx.upscale_input(mode)
        call(); nd, nr = call()
        grown = free0 - torch.cuda.mem_get_info()[0]
        ms = timed(torch, call, reps)
        ctx.timing_enable(STAGES); call(); ctx.timing_reset()
        for _ in range(reps):
            call()
        st = {s: ctx.timing_read(s)[0] / reps for s in STAGES}
        ctx.timing_enable([])
        rows.append({"mode": mode, "call_ms": ms, "grown_mb": grown / 2.0 ** 20, "detected": int(sum(nd)), "regions": int(sum(nr)), "stages": st})
    print(json.dumps({"rows": rows}))
    ctx.close()


def one_graf():
    import torch
    import __graft_entry__ as ge
    import orc
    from PIL import Image
    pkg = ge.load_package()
    rgb = [np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", fn)).convert("RGB")) for fn in ("graf1.png", "graf6.png")]
    rows = []
    for step in (2, 1):
        a, b = (orc.grey_of_rgb(np.ascontiguousarray(im[::step, ::step])) for im in rgb)   # (B + G + R) / 3.0 as the command line reads a colour image
        h, w = a.shape
        t = torch.from_numpy(np.stack([a, b])).cuda()
        torch.cuda.synchronize()
        ctx = pkg.Context(0, w, h, 2)
        for on in (0, 1):
            ctx.upscale_input(on)
            pkg.ransac_pin_seed(4242)
            res, _ = pkg.match_pair_dev(ctx, t.data_ptr(), w, h, pkg.PairParams.default())
            rows.append({"w": w, "h": h, "on": on, "detected": list(res.n_detected), "described": list(res.n_described), "tentatives": res.n_tentatives,
                         "unique": res.n_unique, "inliers": res.n_inliers, "samples": res.ransac_samples})
        ctx.close()
    print(json.dumps({"rows": rows}))


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
        return {"call": lambda: one_call(reps), "modes": lambda: one_modes(reps), "graf": one_graf}[case]()
    other = args[args.index("--against") + 1] if "--against" in args else None
    out = ["doubled first octave (mods_ctx_upscale_input), %d images of %d x %d, default HessianAffine + RootSIFT; device events, ms per call," % (N_IMG, W, H),
           "%d calls per figure" % reps, "",
           "1. switch off: detect + describe, %d rounds of fresh processes, alternating" % ROUNDS]
    runs = {"this build": [], "parent": []}
    for _ in range(ROUNDS):
        runs["this build"].append(spawn("call", reps))
        if other:
            runs["parent"].append(spawn("call", reps, other))
    for name, rs in runs.items():
        if rs:
            v = [r["call_ms"] for r in rs]
            out.append("%-11s %s   median %.3f, spread (max - min) %.3f, %d regions" % (name, " ".join("%.3f" % x for x in v), float(np.median(v)), max(v) - min(v), rs[0]["regions"]))
    rows = spawn("modes", reps)["rows"]
    out += ["", "2. switch on, one context walked through the modes (mode 1: the first level in one launch; mode 2: double, then blur);",
            "   `grown`: device memory taken since the row above (mode 0: what a context's first calls reserve on demand; mode 1: the pools",
            "   of the doubled octave; mode 2: the doubled batch; 0 once they exist)",
            "%-5s %-10s %-10s %-9s %-9s %-9s %-9s %-9s %-11s %-10s %-9s" % ("mode", "call", "PYRAMID", "blur", "resize", "small", "response", "nms", "grown MiB", "detected", "regions")]
    for r in rows:
        s = r["stages"]
        out.append("%-5d %-10.3f %-10.3f %-9.3f %-9.3f %-9.3f %-9.3f %-9.3f %-11.1f %-10d %-9d" % (r["mode"], r["call_ms"], s["pyramid"], s["blur"], s["resize"], s["blur_small"],
                                                                                           s["response"], s["nms"], r["grown_mb"], r["detected"], r["regions"]))
    m1 = [r for r in rows if r["mode"] == 1][-1]
    m2 = [r for r in rows if r["mode"] == 2][-1]
    f = lambda r: r["stages"]["blur"] + r["stages"]["resize"]
    out += ["first level, mode 2 - mode 1 (blur + resize stage sums, launches timed one by one): %.3f ms; PYRAMID scope: %.3f ms; call: %.3f ms"
            % (f(m2) - f(m1), m2["stages"]["pyramid"] - m1["stages"]["pyramid"], m2["call_ms"] - m1["call_ms"])]
    out += ["", "3. graf1 / graf6 (tests/golden) at every second pixel and at full size, mods_match_pair_dev: one view, homography, RANSAC seed pinned",
            "%-10s %-8s %-14s %-14s %-11s %-8s %-8s %-8s" % ("image", "switch", "detected", "described", "tentatives", "unique", "inliers", "samples")]
    for r in spawn("graf", reps)["rows"]:
        out.append("%-10s %-8s %-14s %-14s %-11d %-8d %-8d %-8d" % ("%dx%d" % (r["w"], r["h"]), "on" if r["on"] else "off", "%d / %d" % tuple(r["detected"]),
                                                                "%d / %d" % tuple(r["described"]), r["tentatives"], r["unique"], r["inliers"], r["samples"]))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "upscale_timing.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
