"""Event-timed optimizer update of train.py:401-423 alone (no render): the densification statistics + the Adam step at 200k
Gaussians, SH degree 3, the nine per-Gaussian groups, with and without the two decoder groups of --motion_offset_flag:

    python tools/optim_bench.py [--P 200000] [--reps 50] [--rounds 5]

  "torch"  torch.optim.Adam(fused=True) + densify.update_max_radii + densify.add_densification_stats (what training_setup builds
           by default)
  "fused"  optim.FusedAdam.step(stats=...): two launches (csrc/adam.hip)

Per round and variant one JSON line: GPU milliseconds per call (median of HIP-event pairs over --reps calls, at a settled clock),
wall microseconds per call (host time of a loop of --reps calls that ends with one synchronisation), and the achieved bytes per
second against the traffic model of the update: Adam reads p, g, m, v and writes p, m, v = 28 B per parameter float.  The kernel
launches of one call are counted with the torch profiler (tools/ssim_crop_bench.py does the same); `rocprofv3 --kernel-trace
--stats -- python tools/optim_bench.py --reps 5 --rounds 1` gives the same count from the runtime's side."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = dict(xyz=(3,), f_dc=(1, 3), f_rest=(15, 3), opacity=(1,), scaling=(3,), rotation=(4,), normal=(3,), albedo=(3,), roughness=(1,))
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=0.05, scaling=5e-3, rotation=1e-3, normal=1e-3, albedo=0.05, roughness=0.05)


def timed(fn, reps):
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return host / reps * 1e6, (time.perf_counter() - t0) / reps * 1e6


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            out[e.name] = out.get(e.name, 0) + 1
    return out


def build(P, decoders, fused, gen):
    from mygauhuman_amd import nets, nets_pose, optim
    groups = [{"params": [torch.nn.Parameter(torch.randn((P,) + shp, device="cuda", generator=gen))], "lr": LRS[n], "name": n}
              for n, shp in ROWS.items()]
    if decoders:
        torch.manual_seed(0)
        groups.append({"params": list(nets_pose.FusedBodyPoseRefiner(total_bones=24, embedding_size=69, mlp_width=128,
                                                                     mlp_depth=2).cuda().parameters()), "lr": 5e-4, "name": "pose_decoder"})
        groups.append({"params": list(nets.FusedLBSOffsetDecoder(total_bones=24).cuda().parameters()), "lr": 5e-5,
                       "name": "lweight_offset_decoder"})
    cls = optim.FusedAdam if fused else torch.optim.Adam
    opt = cls(groups, lr=0.0, eps=1e-15, **({} if fused else {"fused": True}))
    params = [p for g in opt.param_groups for p in g["params"]]
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
    model = types.SimpleNamespace(xyz_gradient_accum=torch.zeros((P, 1), device="cuda"), denom=torch.zeros((P, 1), device="cuda"),
                                  max_radii2D=torch.zeros((P,), device="cuda"))
    return opt, params, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from mygauhuman_amd import _lib, densify
    ghz = _lib.settle_clock()[-1][1]
    P = args.P
    gen = torch.Generator(device="cuda").manual_seed(0)
    vpt = torch.zeros((P, 3), device="cuda", requires_grad=True)
    vpt.grad = torch.randn((P, 3), device="cuda", generator=gen) * 1e-3
    radii = torch.randint(0, 40, (P,), device="cuda", generator=gen, dtype=torch.int32)
    vis = radii > 8
    for decoders in (False, True):
        variants = []
        for name in ("torch", "fused"):
            opt, params, model = build(P, decoders, name == "fused", gen)
            if name == "fused":
                fn = (lambda opt=opt, model=model: opt.step(stats=(vpt, vis, radii, model)))
            else:
                def fn(opt=opt, model=model):
                    densify.update_max_radii(model, radii, vis)
                    densify.add_densification_stats(model, vpt, vis)
                    opt.step()
            floats = sum(p.numel() for p in params)
            variants.append((name, fn, floats, len(params)))
            for _ in range(5):
                fn()
        for rnd in range(args.rounds):
            for name, fn, floats, n_tensors in variants:
                _lib.settle_clock()
                ms = timed(fn, args.reps)
                host_us, wall_us = wall(fn, args.reps)
                print(json.dumps({"what": "optimizer_update", "P": P, "decoders": decoders, "tensors": n_tensors, "floats": floats,
                                  "variant": name, "round": rnd, "gpu_ms": round(ms, 4), "host_us_per_call": round(host_us, 1),
                                  "wall_us_per_call": round(wall_us, 1), "model_bytes": 28 * floats,
                                  "tb_per_s": round(28 * floats / (ms * 1e-3) / 1e12, 3), "clock_ghz": ghz}), flush=True)
        for name, fn, _, _ in variants:
            k = launches(fn)
            print(json.dumps({"what": "kernel_launches", "decoders": decoders, "variant": name, "total": sum(k.values()), "kernels": k}),
                  flush=True)


if __name__ == "__main__":
    main()
