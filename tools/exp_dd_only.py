#!/usr/bin/env python3
"""Development aid: detect + orient + describe only, N contexts on N host threads, 32 images per call (the pipeline's launch shape):
the rate the GPU stages in front of the matcher can reach without the matcher and the verifier behind them.
usage: exp_dd_only.py [contexts [calls per context]] [--u8] [--kernels=MASK]
  --u8: the batch as 8-bit grey through detect_describe_dev_u8; --kernels: the mask of Context.set_u8_kernels (240: all four sampling
  kernels on the strip copy of the 8-bit images, 15: on the row-major 8-bit images, default: the library's choice)"""
import os, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import __graft_entry__ as ge
import synth

pkg = ge.load_package()
W, H, B = 1920, 1080, 32
U8 = "--u8" in sys.argv
MASK = [int(a.split("=")[1], 0) for a in sys.argv[1:] if a.startswith("--kernels=")]
argv = [a for a in sys.argv[1:] if a != "--u8" and not a.startswith("--kernels=")]
NW = int(argv[0]) if len(argv) > 0 else 4
REP = int(argv[1]) if len(argv) > 1 else 12
imgs = []
for i in range(B // 2):
    a, b, _ = synth.pair(W, H, seed=2000 + (i % 2))
    imgs += [a, b]
t = torch.from_numpy(np.stack(imgs).astype(np.uint8) if U8 else np.stack(imgs)).cuda()
ctxs = [pkg.Context(0, W, H, B) for _ in range(NW)]
for c in ctxs:
    if MASK:
        c.set_u8_kernels(MASK[0])
call = (lambda c: c.detect_describe_dev_u8(t.data_ptr(), B, W, H)) if U8 else (lambda c: c.detect_describe_dev(t.data_ptr(), B, W, H))
for c in ctxs:
    call(c); c.sync()
def work(c):
    for _ in range(REP):
        call(c)
    c.sync()
torch.cuda.synchronize()
t0 = time.perf_counter()
th = [threading.Thread(target=work, args=(c,)) for c in ctxs]
for x in th: x.start()
for x in th: x.join()
dt = time.perf_counter() - t0
print(("8-bit source, " if U8 else "") + ("kernels mask %d, " % MASK[0] if MASK else "") + "contexts %d: %.1f pairs/s (%.3f ms per 32-image call per context)" % (NW, NW * REP * B / 2 / dt, dt / REP * 1e3))
