#!/usr/bin/env python3
"""The bf16 matrix-core mode of the built-in networks (csrc/nets_mfma.hip) beside the fp32 mode on the MI355X; writes
profiles/nets_bf16_timing.txt.

    python tools/bench_nets_bf16.py [--out FILE] [--n 6000] [--parent DIR]

Steps, each a process of its own under a time limit; the script stops at the first that fails:
  kernels   n patches through each network, an fp32 and a bf16 net alternating in one process: mods_net_forward_dev between device
            events, mean and range of 5 calls after 2 warm ones; then the time per layer (mods_test_net_stage_times: an event in
            front of every launch), mean of 5, and the FLOP/s of the matrix-core layers against the bf16 peak.
            Fails unless the bf16 net is faster than the fp32 net by more than both ranges, on every network.
  accuracy  the same patches: HardNet bytes that differ between the modes (share, largest), largest AffNet parameter difference,
            largest OriNet angle difference.  Reported, not judged.
  e2e       orient_describe of the 1920x1080 texture of tools/bench_nets.py with three fp32 nets against three bf16 nets
            (wall time of the call, alternating, mean and range of 5 after a warm one).
  deep      the command line's deep configuration (AffNet, OriNet, HardNet in-process) on graf1 / graf6 in both modes: described
            regions, unique tentatives, verified.
  default   with --parent DIR, a built checkout of the parent commit: `bench.py --gpus 1 --steps 10 --warmup 2` there and here in
            alternating fresh processes, three each; pairs/s, ms per step and the detect + describe time of a batch of 16 pairs of
            1920x1080 images (bench.py's stage_ms_per_pair.detect_describe x 16).  Fails unless the two series' ranges overlap:
            the default (fp32, no network) path must be what it was.
HardNet weights: the daemon's seeded model (seed 5) with random BatchNorm statistics for the kernels, as it is built for the
command line (no checkpoint ships with the reference); AffNet / OriNet: tests/golden/nets.npz."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "mods-light-zmq_amd"))
KINDS = ("affnet", "orinet", "hardnet")
MR = 3.0 * np.sqrt(3.0)
PEAK_BF16 = 2.5e15
N = int(os.environ.get("BENCH_NETS_N", "6000"))


def layer_macs(kind):
    """multiply-adds per patch of stages 1..7"""
    c = 32 if kind == "hardnet" else 16
    shapes = [(1, c, 32), (c, c, 32), (c, 2 * c, 16), (2 * c, 2 * c, 16), (2 * c, 4 * c, 8), (4 * c, 4 * c, 8)]
    m = [cin * cout * 9 * hw * hw for cin, cout, hw in shapes]
    if kind == "orinet":        # conv8x8 with padding 1: a 3 x 3 map of windows clipped by the border
        return m + [2 * 64 * sum((8 - abs(dy)) * (8 - abs(dx)) for dy in (-1, 0, 1) for dx in (-1, 0, 1))]
    return m + [128 * 128 * 64 if kind == "hardnet" else 3 * 64 * 64]


def _nets(pkg, precision):
    import test_gpu_nets as tg
    return {k: pkg.Net(k, tg._state(k), precision=precision) for k in KINDS}


def _patches():
    return np.random.default_rng(0).uniform(0, 255, (N, 32, 32)).astype(np.float32)


def step_kernels():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    nets = {"fp32": _nets(pkg, "fp32"), "bf16": _nets(pkg, "bf16")}
    t = torch.from_numpy(_patches()).cuda()
    s = torch.cuda.current_stream().cuda_stream
    print("# kernels: %d patches, mods_net_forward_dev between device events; fp32 and bf16 nets alternating, mean (min .. max) of 5 calls after 2" % N)
    ok = True
    for kind in KINDS:
        out = torch.zeros((N, nets["fp32"][kind].dim), dtype=torch.float32, device="cuda")
        ms = {"fp32": [], "bf16": []}
        for i in range(7):
            for mode in ("fp32", "bf16"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                nets[mode][kind].forward_dev(s, t.data_ptr(), N, out.data_ptr(), quantise=True)
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ms[mode].append(e0.elapsed_time(e1))
        f, b = ms["fp32"], ms["bf16"]
        faster = max(b) < min(f) and np.mean(f) - np.mean(b) > (max(f) - min(f)) + (max(b) - min(b))
        ok = ok and faster
        print("  %-8s fp32 %8.3f ms (%.3f .. %.3f)   bf16 %8.3f ms (%.3f .. %.3f)   fp32 / bf16 %5.2f x%s" % (
            kind, np.mean(f), min(f), max(f), np.mean(b), min(b), max(b), np.mean(f) / np.mean(b), "" if faster else "   NOT FASTER"))
    print("# per layer: milliseconds between the events around each launch, summed over the %d chunks, mean of 5 calls (2 warm);" % ((N + 511) // 512))
    print("# stage 0 = normalisation, 1..6 = convolution blocks, 7 = head; TFLOP/s = 2 x multiply-adds x n / time; the bf16 mode's")
    print("# stages 2..6 and HardNet's stage 7 run on the matrix cores: share of the %.1f PFLOP/s bf16 peak in brackets" % (PEAK_BF16 / 1e15))
    for kind in KINDS:
        out = torch.zeros((N, nets["fp32"][kind].dim), dtype=torch.float32, device="cuda")
        acc = {"fp32": [], "bf16": []}
        for i in range(7):
            for mode in ("fp32", "bf16"):
                r = nets[mode][kind].stage_times(s, t.data_ptr(), N, out.data_ptr(), quantise=True)
                if i >= 2:
                    acc[mode].append(r)
        macs = layer_macs(kind)
        for mode in ("fp32", "bf16"):
            m = np.mean(acc[mode], axis=0)
            sp = np.max(acc[mode], axis=0) - np.min(acc[mode], axis=0)
            print("  %-8s %s  ms     %s   sum %.3f" % (kind, mode, " ".join("%7.3f" % v for v in m), m.sum()))
            print("  %-8s %s  range  %s" % (kind, mode, " ".join("%7.3f" % v for v in sp)))
            tf = [2.0 * macs[i - 1] * N / (m[i] * 1e-3) / 1e12 for i in range(1, 8)]
            cells = []
            for i, v in enumerate(tf, 1):
                mfma = mode == "bf16" and (2 <= i <= 6 or (i == 7 and kind == "hardnet"))
                cells.append("%7.1f" % v + ("[%4.1f%%]" % (100 * v * 1e12 / PEAK_BF16) if mfma else ""))
            print("  %-8s %s  TFLOP/s        %s" % (kind, mode, " ".join(cells)))
    if not ok:
        print("  GATE FAILED: the bf16 mode is not faster than the fp32 mode by more than the two ranges on every network")
        sys.exit(1)


def step_accuracy():
    import __graft_entry__ as ge
    pkg = ge.load_package()
    p = _patches()
    f, b = _nets(pkg, "fp32"), _nets(pkg, "bf16")
    of = {k: f[k].forward(p, quantise=True) for k in KINDS}
    ob = {k: b[k].forward(p, quantise=True) for k in KINDS}
    d = np.abs(of["hardnet"] - ob["hardnet"])
    print("# accuracy: bf16 mode against fp32 mode on the same %d patches (uniform noise, rounded to 8 bits); trained AffNet / OriNet, seeded HardNet" % N)
    print("  hardnet  bytes that differ %.4f of %d, largest difference %d, mean %.4f (bytes' standard deviation %.1f)" % (
        float(np.mean(d > 0)), d.size, int(d.max()), float(d.mean()), float(of["hardnet"].std())))
    print("  affnet   largest parameter difference %.3g (parameters' range %.3g)" % (float(np.max(np.abs(of["affnet"] - ob["affnet"]))), float(np.ptp(of["affnet"]))))
    af, ab = (np.arctan2(o[:, 0], o[:, 1]) for o in (of["orinet"], ob["orinet"]))
    dd = np.degrees(np.abs(np.angle(np.exp(1j * (af - ab)))))
    print("  orinet   largest angle difference %.3f degrees, mean %.4f" % (float(dd.max()), float(dd.mean())))
    # atan2 of a short vector is ill-conditioned: the same figures over the patches whose fp32 output is not short
    nf, nb = np.hypot(of["orinet"][:, 0], of["orinet"][:, 1]), np.hypot(ob["orinet"][:, 0], ob["orinet"][:, 1])
    i = int(np.argmax(dd))
    print("  orinet   the largest is patch %d: |output| %.4f (fp32), %.4f (bf16); |output| over all patches: median %.3f, smallest %.4f;"
          % (i, nf[i], nb[i], float(np.median(nf)), float(nf.min())))
    print("  orinet   largest output difference %.3g; angle difference %s" % (float(np.max(np.abs(of["orinet"] - ob["orinet"]))),
          ", ".join("over the %d patches with |output| >= %.2f: largest %.3f degrees, mean %.4f" % (int((nf >= t).sum()), t, float(dd[nf >= t].max()), float(dd[nf >= t].mean()))
                    for t in (0.05, 0.2) if (nf >= t).any())))


def step_e2e():
    import time
    import __graft_entry__ as ge
    import synth
    pkg = ge.load_package()
    w, h = 1920, 1080
    img = synth.texture(w, h, seed=1)
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    ctx = pkg.Context(0, w, h, 1)
    keys = ctx.detect_hessian_affine(img, det)
    nets = {"fp32": _nets(pkg, "fp32"), "bf16": _nets(pkg, "bf16")}
    ms = {"fp32": [], "bf16": []}
    regs = {}
    for i in range(6):
        for mode in ("fp32", "bf16"):
            ctx.set_builtin_shape(nets[mode]["affnet"], MR, True)
            ctx.set_builtin_orientation(nets[mode]["orinet"], MR, True)
            ctx.set_builtin_descriptor(nets[mode]["hardnet"], MR, True)
            t0 = time.perf_counter()
            regs[mode] = ctx.orient_describe(img, keys)
            if i >= 1:
                ms[mode].append((time.perf_counter() - t0) * 1e3)
    print("# e2e: orient_describe of a %dx%d texture, %d keypoints; wall time of the call, alternating, mean (min .. max) of 5 after a warm one" % (w, h, len(keys)))
    for mode in ("fp32", "bf16"):
        print("  three %s networks  %8.2f ms (%.2f .. %.2f), %d regions" % (mode, np.mean(ms[mode]), min(ms[mode]), max(ms[mode]), len(regs[mode])))
    print("  fp32 / bf16          %8.2f x" % (np.mean(ms["fp32"]) / np.mean(ms["bf16"])))
    ctx.close()


def step_deep():
    import re
    import test_gpu_nets as tg
    from test_gpu_cli import CFG, G1, G6, MODS
    print("# deep: mods on graf1 / graf6, deep configuration (tests/configs/classic.ini with AffNet, OriNet, HardNet in-process, iters_zmq.ini),")
    print("# LO-RANSAC(homography), MODS_RANSAC_SEED=4242; AffNet / OriNet trained, HardNet the daemon's seeded model as built (untrained)")
    with tempfile.TemporaryDirectory() as tmp:
        import pathlib
        tmp = pathlib.Path(tmp)
        base = open(tg._deep_config(tmp, tg._weights_file(tmp / "w.npz"))).read()
        for mode in ("fp32", "bf16"):
            text = base
            for sec in ("AffNet", "OriNet", "zmqDescriptor"):
                text = text.replace("[%s]\nweights=" % sec, "[%s]\nprecision = %s\nweights=" % (sec, mode))
            (tmp / (mode + ".ini")).write_text(text)
            p = subprocess.run([MODS, G1, G6, "o1.png", "o2.png", "k1.npz", "k2.npz", "m.txt", "log.txt", "0", "0", "H.txt", str(tmp / (mode + ".ini")),
                                os.path.join(CFG, "iters_zmq.ini")], cwd=tmp, env=dict(os.environ, MODS_RANSAC_SEED="4242"), stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=300)
            if p.returncode:
                sys.stderr.write(p.stderr.decode()[-2000:])
                sys.exit(1)
            log = open(tmp / "log.txt").read().split()
            tent = re.search(r"(\d+) tentatives found", p.stderr.decode())
            print("  %s  described regions %d + %d, tentatives %s, unique tentatives %s, verified %s" % (
                mode, len(np.load(tmp / "k1.npz")["xy"]), len(np.load(tmp / "k2.npz")["xy"]), tent.group(1) if tent else "-", log[2], log[1]))


def step_default(parent):
    import json
    if not os.path.exists(os.path.join(parent, "bench.py")):
        print("# default: no bench.py under %s" % parent)
        sys.exit(1)
    runs = {"parent": [], "this": []}
    for i in range(3):
        for name, root in (("parent", parent), ("this", ROOT)):
            p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"], cwd=root,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if p.returncode:
                sys.stderr.write(p.stderr.decode()[-2000:])
                sys.exit(1)
            r = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])          # the result line
            runs[name].append((r["value"], r["ms_per_step"], 16.0 * r["config"]["stage_ms_per_pair"]["detect_describe"]))
    print("# default: bench.py --gpus 1 --steps 10 --warmup 2 of the parent commit and of this tree, alternating fresh processes, three each;")
    print("# detect + describe = 16 x stage_ms_per_pair.detect_describe (a batch of 16 pairs of 1920x1080 images); every run, then min .. max")
    ok = True
    for j, (label, fmt) in enumerate((("pairs/s", "%.1f"), ("ms per step", "%.2f"), ("detect + describe ms", "%.3f"))):
        v = {k: [r[j] for r in runs[k]] for k in runs}
        inside = max(min(v["parent"]), min(v["this"])) <= min(max(v["parent"]), max(v["this"]))
        ok = ok and inside
        for k in ("parent", "this"):
            print("  %-22s %-7s %s   (%s .. %s)" % (label, k, " ".join(fmt % x for x in v[k]), fmt % min(v[k]), fmt % max(v[k])))
        print("  %-22s the two ranges %s" % (label, "overlap" if inside else "DO NOT OVERLAP"))
    if not ok:
        print("  GATE FAILED: the default path is not inside the parent's run-to-run spread")
        sys.exit(1)


STEPS = {"kernels": step_kernels, "accuracy": step_accuracy, "e2e": step_e2e, "deep": step_deep}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nets_bf16_timing.txt"))
    ap.add_argument("--n", type=int, default=N, help="patches of the kernels and accuracy steps")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the step `default`")
    ap.add_argument("--step", default=None, choices=sorted(STEPS) + ["default"], help="run one step in this process (what the driver does for each of them)")
    args = ap.parse_args()
    if args.step:
        globals()["N"] = args.n
        if args.step == "default":
            step_default(os.path.abspath(args.parent or ""))
        else:
            STEPS[args.step]()
        return 0
    lines = ["# tools/bench_nets_bf16.py - the built-in networks in bf16 mode (csrc/nets_mfma.hip) beside the fp32 mode (csrc/nets.hip) on the MI355X"]
    rc = 0
    plan = [("kernels", 200), ("accuracy", 200), ("e2e", 200), ("deep", 300)] + ([("default", 900)] if args.parent else [])
    for step, limit in plan:
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n)]
                           + (["--parent", os.path.abspath(args.parent)] if args.parent else []),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        lines += p.stdout.decode().rstrip().splitlines()
        if p.returncode:
            lines.append("# step %s failed (exit status %d); stopped here" % (step, p.returncode))
            sys.stderr.write(p.stderr.decode()[-4000:])
            rc = 1
            break
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
