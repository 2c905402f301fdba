"""The skinning-weight offset network at 200k points: the fused kernels (csrc/mlp.hip, both instructions) vs the same module in torch
ops -- the error of each forward against float64, then forward and forward + backward times.
python tools/mlp_bench.py [--bones {24,55}] [--points P]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mygauhuman_amd import nets  # noqa: E402
from mygauhuman_amd.nets import FusedLBSOffsetDecoder  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bones", type=int, default=24, choices=nets.FUSED_BONE_COUNTS)
ap.add_argument("--points", type=int, default=200_000)
args = ap.parse_args()
NB, P = args.bones, args.points
FLOP = 2 * (63 * 128 + 2 * 128 * 128 + 191 * 128 + 128 * NB)   # forward, per point

torch.manual_seed(0)
dec = FusedLBSOffsetDecoder(NB).cuda()
dec.use_fused = True
pts = torch.rand(1, P, 3, device="cuda") - 0.5
w = torch.randn(1, NB, P, device="cuda")
d64 = FusedLBSOffsetDecoder(NB).cuda().double()
d64.load_state_dict({k: v.double() for k, v in dec.state_dict().items()})
with torch.no_grad():
    want = d64.forward_torch(pts.double())


def timed(fn, n=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def step(fn):
    for p in dec.parameters():
        p.grad = None
    (fn() * w).sum().backward()


variants = (("fused f32", "f32", lambda: dec(pts)), ("fused bf16x3", "bf16x3", lambda: dec(pts)),
            ("torch ops", None, lambda: dec.forward_torch(pts)))
try:
    for name, mode, fn in variants:
        if mode:
            nets.set_precision(mode)
        with torch.no_grad():
            err = float((fn().double() - want).abs().max() / want.abs().max())
            t_fwd = timed(fn)
        t_both = timed(lambda: step(fn))
        print(f"bones={NB} P={P:7d} {name:12s} error vs float64 / max |out| = {err:.2e}   forward {t_fwd * 1e3:7.3f} ms "
              f"({FLOP * P / t_fwd / 1e12:5.1f} TFLOP/s)   forward + backward {t_both * 1e3:7.3f} ms", flush=True)
finally:
    nets.set_precision("bf16x3")
