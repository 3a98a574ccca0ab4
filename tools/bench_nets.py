#!/usr/bin/env python3
"""Timing of the in-process networks (csrc/nets.hip) on the MI355X; writes profiles/nets_timing.txt.

    python tools/bench_nets.py [--out FILE] [--precision fp32|bf16]

--precision: the arithmetic of the built-in networks (pkg.Net(..., precision=...)); the comparison of the two modes with each
other is tools/bench_nets_bf16.py.

Three steps, each a process of its own under a time limit; the script stops at the first step that fails:
  kernels  per network and n in {512, 6000}: mods_net_forward_dev between device events (warm, median of 20), beside the same
           batch through the daemon's PyTorch model on the same GPU (device-resident input, requests of 512 as the daemon cuts
           them, warmed as the daemon warms it).  FLOP/s = 2 x the multiply-adds of the architecture x n / time.
  e2e      the gate: orient_describe of a 1920x1080 texture (doBaumberg = 0) with the three built-in networks against the same
           call with three daemons on the same GPU loaded from the same arrays.  Fails unless the built-in path takes less time.
  ladder   the two-step HessianAffine ladder with built-in networks, MODS_LADDER_WORKERS=1 against the default (recorded only).
HardNet weights: the daemon's seeded model (no checkpoint ships with the reference); AffNet / OriNet: tests/golden/nets.npz."""
import argparse
import ctypes as C
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "mods-light-zmq_amd"))
KINDS = ("affnet", "orinet", "hardnet")
MR = 3.0 * np.sqrt(3.0)
PEAK_FP32 = 157.3e12
PRECISION = "fp32"      # --precision


def macs(kind):
    """multiply-adds per patch, from the architecture"""
    c = 32 if kind == "hardnet" else 16
    shapes = [(1, c, 32), (c, c, 32), (c, 2 * c, 16), (2 * c, 2 * c, 16), (2 * c, 4 * c, 8), (4 * c, 4 * c, 8)]
    m = sum(cin * cout * 9 * hw * hw for cin, cout, hw in shapes)
    if kind == "hardnet":
        return m + 128 * 128 * 64
    if kind == "affnet":
        return m + 3 * 64 * 64
    return m + 2 * 64 * sum((8 - abs(dy)) * (8 - abs(dx)) for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def states():
    import test_gpu_nets as tg
    return {k: tg._state(k) for k in KINDS}


def step_kernels():
    import torch
    import __graft_entry__ as ge
    import test_gpu_nets as tg
    import zmq_daemon as zd
    pkg = ge.load_package()
    st = states()
    rng = np.random.default_rng(0)
    print("# kernels: time of one call for n patches, median of 20 warm calls between device events; FLOP/s against %.1f TF fp32" % (PEAK_FP32 / 1e12))
    print("# %-8s %6s %12s %10s %8s %14s %10s" % ("network", "n", "built-in ms", "TFLOP/s", "of peak", "PyTorch ms", "TFLOP/s"))
    for kind in KINDS:
        net = pkg.Net(kind, st[kind], precision=PRECISION)
        model = zd.build_model(kind, st[kind], 0, "cuda")
        model.warm_up()
        module = tg._module_of(model)
        for n in (512, 6000):
            p = rng.uniform(0, 255, (n, 32, 32)).astype(np.float32)
            t = torch.from_numpy(p).cuda()
            out = torch.zeros((n, net.dim), dtype=torch.float32, device="cuda")
            s = torch.cuda.current_stream().cuda_stream

            def ours():
                net.forward_dev(s, t.data_ptr(), n, out.data_ptr(), quantise=True)

            def theirs():
                with torch.no_grad():
                    for i in range(0, n, 512):
                        chunk = t[i:i + 512].unsqueeze(1)
                        if len(chunk) < 512:        # the daemon pads a request to its batch shape
                            chunk = torch.cat([chunk, torch.zeros((512 - len(chunk), 1, 32, 32), device="cuda")])
                        module(chunk)
            res = []
            for fn in (ours, theirs):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                ms = []
                for _ in range(20):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                res.append(float(np.median(ms)))
            fl = 2.0 * macs(kind) * n
            print("  %-8s %6d %12.3f %10.2f %7.1f%% %14.3f %10.2f" % (kind, n, res[0], fl / res[0] / 1e9, 100 * fl / (res[0] * 1e-3) / PEAK_FP32,
                                                                   res[1], fl / res[1] / 1e9))
        net.close()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def step_e2e():
    import __graft_entry__ as ge
    import synth
    pkg = ge.load_package()
    st = states()
    w, h = 1920, 1080
    img = synth.texture(w, h, seed=1)
    det = pkg.HessAffParams.default()
    det.doBaumberg = 0
    ctx = pkg.Context(0, w, h, 1)
    keys = ctx.detect_hessian_affine(img, det)
    nets = {k: pkg.Net(k, st[k], precision=PRECISION) for k in KINDS}

    def timed(reps=7):
        r = ctx.orient_describe(img, keys)         # warm
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = ctx.orient_describe(img, keys)     # returns after the regions are on the host
            ms.append((time.perf_counter() - t0) * 1e3)
        return r, float(np.median(ms)), float(np.min(ms))

    ctx.set_builtin_shape(nets["affnet"], MR, True)
    ctx.set_builtin_orientation(nets["orinet"], MR, True)
    ctx.set_builtin_descriptor(nets["hardnet"], MR, True)
    regs_b, ms_b, min_b = timed()
    ctx.set_builtin_shape(None); ctx.set_builtin_orientation(None); ctx.set_builtin_descriptor(None)

    wire = C.CDLL(os.path.join(ROOT, "mods-light-zmq_amd", "libmodszmq.so"))
    procs = []
    with tempfile.TemporaryDirectory() as tmp:
        wfile = os.path.join(tmp, "weights.npz")
        np.savez(wfile, **{k + "." + n: v for k in KINDS for n, v in st[k].items()})
        try:
            eps = {}
            for kind in KINDS:
                ep = "tcp://127.0.0.1:%d" % _free_port()
                d = subprocess.Popen([sys.executable, os.path.join(ROOT, "mods-light-zmq_amd", "zmq_daemon.py"), "--model", kind, "--bind", ep,
                                      "--device", "cuda", "--weights", wfile], stderr=subprocess.PIPE)
                procs.append(d)
                line = ""
                for _ in range(20):
                    line = d.stderr.readline().decode()
                    if "serving" in line or not line:
                        break
                if "serving" not in line:
                    raise RuntimeError("daemon %s did not start: %s" % (kind, line))
                eps[kind] = C.create_string_buffer(ep.encode())
            time.sleep(0.3)
            hook = C.cast(wire.mods_zmq_descriptor_hook, C.c_void_p).value
            ctx.set_external_shape(hook, C.addressof(eps["affnet"]), MR, 32)
            ctx.set_external_orientation(hook, C.addressof(eps["orinet"]), MR, 32)
            ctx.set_external_descriptor(hook, C.addressof(eps["hardnet"]), MR, 32)
            regs_d, ms_d, min_d = timed()
        finally:
            for d in procs:
                d.terminate()
            for d in procs:
                try:
                    d.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    d.kill()
    # (the daemons' convolutions come from a library and round differently: frames and descriptors agree closely, not bit for bit)
    note = "%d regions with the daemons" % len(regs_d)
    if len(regs_b) == len(regs_d):
        fr = max(float(np.max(np.abs(regs_b[f] - regs_d[f]))) for f in ("x", "y", "a11", "a12", "a21", "a22"))
        dd = np.abs(regs_b["desc"].astype(np.int16) - regs_d["desc"].astype(np.int16))
        note += "; largest frame difference %.3g; descriptor bytes that differ: %d of %d (largest difference %d)" % (fr, int((dd > 0).sum()), dd.size, int(dd.max()))
    print("# e2e: orient_describe of a %dx%d texture, %d keypoints -> %d regions; wall time of the call, median (min) of 7 warm calls" % (w, h, len(keys), len(regs_b)))
    print("  three built-in networks  %9.2f ms (%.2f)" % (ms_b, min_b))
    print("  three daemons, same GPU  %9.2f ms (%.2f)" % (ms_d, min_d))
    print("  daemons / built-in       %9.2f x" % (ms_d / ms_b))
    print("  " + note)
    ctx.close()
    if not ms_b < ms_d:
        print("  GATE FAILED: the built-in path is not faster")
        sys.exit(1)


def step_ladder():
    import torch
    import __graft_entry__ as ge
    import synth
    pkg = ge.load_package()
    st = states()
    w, h = 480, 360
    a, b, _ = synth.pair(w, h, seed=7)
    d = pkg.view_ctx_dims(w, h)
    steps = [pkg.LadderStep.make((1,), 360.0), pkg.LadderStep.make((1, 2, 4), 120.0)]
    par = pkg.PairParams.default()
    par.det.doBaumberg = 0
    t = torch.from_numpy(np.stack([a, b])).cuda()
    torch.cuda.synchronize()
    nets = {k: pkg.Net(k, st[k], precision=PRECISION) for k in KINDS}
    ctx = pkg.Context(0, d[0], d[1], 2)
    ctx.set_builtin_shape(nets["affnet"], MR, True)
    ctx.set_builtin_orientation(nets["orinet"], MR, True)
    ctx.set_builtin_descriptor(nets["hardnet"], MR, True)
    ms = []
    for i in range(8):
        rep1, rep2 = pkg.ImgRep(ctx, 1 << 18), pkg.ImgRep(ctx, 1 << 18)
        pkg.ransac_pin_seed(4242)
        t0 = time.perf_counter()
        res, _ = pkg.match_ladder_dev(ctx, t.data_ptr(), w, h, steps, rep1, rep2, par, min_matches=10 ** 6)
        ms.append((time.perf_counter() - t0) * 1e3)
        n1, n2 = len(rep1), len(rep2)
        rep1.close(); rep2.close()
    print("  MODS_LADDER_WORKERS=%-8s %8.2f ms (median of 6 after 2 warm runs; %d views, %d + %d regions, %d inliers)"
          % (os.environ.get("MODS_LADDER_WORKERS", "default"), float(np.median(ms[2:])), res.n_views, n1, n2, res.n_inliers))
    ctx.close()


def main():
    global PRECISION
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nets_timing.txt"))
    ap.add_argument("--precision", default=PRECISION, choices=["fp32", "bf16"], help="arithmetic of the built-in networks")
    ap.add_argument("--step", default=None, help="run one step in this process (what the driver does for each of them)")
    args = ap.parse_args()
    PRECISION = args.precision
    if args.step:
        {"kernels": step_kernels, "e2e": step_e2e, "ladder": step_ladder}[args.step]()
        return 0
    plan = [("kernels", {}, 300), ("e2e", {}, 300),
            ("ladder", {"MODS_LADDER_WORKERS": "1"}, 200), ("ladder", {}, 200)]
    lines = ["# tools/bench_nets.py - AffNet / OriNet / HardNet in-process (csrc/nets.hip) on the MI355X"]
    if args.precision != "fp32":
        lines.append("# built-in networks in %s mode (csrc/nets_mfma.hip)" % args.precision)
    rc = 0
    for step, env, limit in plan:
        if step == "ladder" and env:
            lines.append("# ladder: two-step HessianAffine ladder of a 480x360 pair, three built-in networks, wall time of mods_match_ladder_dev")
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--precision", args.precision],
                           env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
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
