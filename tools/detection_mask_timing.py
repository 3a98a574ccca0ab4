#!/usr/bin/env python3
"""What the detection masks (mods_ctx_detection_mask*; the gate kernel of csrc/detect.hip) cost and save on a 16-image 1080p batch
through mods_detect_describe_dev, per call:
  - the whole call by the host clock (the call ends in a stream synchronise), mean of `reps` calls after two warm-up calls,
  - the stages by the context's HIP events in a second pass (per-stage events keep the scale space on one stream, so their sum is
    not the first figure): LOCALIZE - where the gate runs - alone, BAUMBERG, and ORIENT + DESCRIBE,
for no mask, an all-255 mask on every image (the gate's pure overhead) and a mask that allows the left half of every image.
Every case runs in a fresh process; the cases alternate `rounds` times and the spread of a case is what its rounds differ by.
  python tools/detection_mask_timing.py [reps] [--against PARENT.so]   the report (profiles/detection_mask_timing.txt); with
                                                                       --against, the no-mask case of another build of the library
                                                                       (the parent commit's) alternates with this build's
  python tools/detection_mask_timing.py [reps] --one CASE [--lib X.so] one such run: a JSON line"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, N_IMG, ROUNDS = 1920, 1080, 16, 3
CASES = ("none", "all255", "half")
STAGES = ("localize", "baumberg", "orient", "describe")


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


def one(case, reps):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    t = torch.from_numpy(images()).cuda()
    torch.cuda.synchronize()
    ctx = pkg.Context(0, W, H, N_IMG)
    if case != "none":
        m = np.full((H, W), 255, np.uint8)
        if case == "half":
            m[:, W // 2:] = 0
        for i in range(N_IMG):
            ctx.set_detection_mask(i, m)
    call = lambda: ctx.detect_describe_dev(t.data_ptr(), N_IMG, W, H)
    call(); nd, nr = call()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    wall = (time.perf_counter() - t0) / reps * 1e3
    ctx.timing_enable(STAGES); call(); ctx.timing_reset()
    for _ in range(reps):
        call()
    ms = {s: ctx.timing_read(s)[0] / reps for s in STAGES}
    counts = [ctx.detection_mask_counts(i) for i in range(N_IMG)] if case != "none" else []
    print(json.dumps({"case": case, "call_ms": wall, "stage_ms": ms, "regions": int(sum(nr)), "keys": int(sum(nd)),
                      "accepted": int(sum(c[0] for c in counts)), "kept": int(sum(c[1] for c in counts))}))
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
        return one(args[args.index("--one") + 1], reps)
    other = args[args.index("--against") + 1] if "--against" in args else None
    runs = {c: [] for c in CASES}
    if other:
        runs["parent none"] = []
    for _ in range(ROUNDS):
        for c in CASES:
            runs[c].append(spawn(c, reps))
            if c == "none" and other:
                runs["parent none"].append(spawn("none", reps, other))
    out = ["detection masks on a %d-image %d x %d batch, mods_detect_describe_dev, ms per call; %d rounds of fresh processes, %d calls each"
           % (N_IMG, W, H, ROUNDS, reps),
           "(call: host clock around the call, which ends in a synchronise; stages: HIP events of the context, a pass of their own)", "",
           "%-12s %-26s %-22s %-22s %-22s %9s %9s %9s" % ("case", "call (rounds)", "LOCALIZE", "BAUMBERG", "ORIENT + DESCRIBE", "regions", "accepted", "kept")]
    fmt = lambda v: " ".join("%.3f" % x for x in v)
    for c, rs in runs.items():
        out.append("%-12s %-26s %-22s %-22s %-22s %9d %9d %9d" % (
            c, fmt([r["call_ms"] for r in rs]), fmt([r["stage_ms"]["localize"] for r in rs]), fmt([r["stage_ms"]["baumberg"] for r in rs]),
            fmt([r["stage_ms"]["orient"] + r["stage_ms"]["describe"] for r in rs]), rs[0]["regions"], rs[0]["accepted"], rs[0]["kept"]))
    med = lambda c, f: float(np.median([f(r) for r in runs[c]]))
    spread = lambda c: max(r["call_ms"] for r in runs[c]) - min(r["call_ms"] for r in runs[c])
    call = lambda r: r["call_ms"]
    out += ["", "run-to-run spread of the call time (max - min over the rounds): " + ", ".join("%s %.3f" % (c, spread(c)) for c in runs)]
    if other:
        out.append("no mask, this build against the parent: median %.3f against %.3f ms (difference %+.3f, spreads %.3f / %.3f)"
                   % (med("none", call), med("parent none", call), med("none", call) - med("parent none", call), spread("none"), spread("parent none")))
    out.append("all-255 mask against no mask (the gate's overhead): %+.3f ms per call; LOCALIZE %+.4f ms"
               % (med("all255", call) - med("none", call), med("all255", lambda r: r["stage_ms"]["localize"]) - med("none", lambda r: r["stage_ms"]["localize"])))
    down = lambda r: r["stage_ms"]["baumberg"] + r["stage_ms"]["orient"] + r["stage_ms"]["describe"]
    out.append("half mask against no mask: call %+.3f ms (%.0f %%); BAUMBERG + ORIENT + DESCRIBE %.3f -> %.3f ms (%.0f %% saved)"
               % (med("half", call) - med("none", call), 100 * (med("half", call) / med("none", call) - 1), med("none", down), med("half", down),
                  100 * (1 - med("half", down) / med("none", down))))
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "detection_mask_timing.txt"), "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
