"""Event-timed occlusion bake (mygauhuman_amd.baking, csrc/bake.hip): one JSON line per measurement.

    python tools/bake_bench.py [--sizes 13000,200000] [--reps 3] [--no-reference]

  * bake ms, fused bake_set against the reference's algorithm (bake_set(fused=False): 6 rasterizer calls per occupied cell), on
    the synthetic human (human_synth) with random unit normals; cell count, instances, batches and peak workspace of the fused bake
  * the per-frame reduction (env_occlusion, one HIP kernel) against its torch expression at 200k Gaussians, with the bytes it reads
"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="13000,200000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    from mygauhuman_amd import baking, human_synth
    for P in [int(s) for s in args.sizes.split(",")]:
        model, _ = human_synth.build(P, seed=0)
        means = model.get_xyz.detach()
        g = torch.Generator().manual_seed(0)
        n = torch.nn.functional.normalize(torch.randn((P, 3), generator=g), dim=1).cuda()
        view = types.SimpleNamespace(occlusion=None)
        fused = lambda: baking.bake_set(view, model, means, n, 16, 32)  # noqa: E731
        fused()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = _time(fused, args.reps)
        peak = torch.cuda.max_memory_allocated() - base
        rec = dict(what="bake", P=P, fused_ms=round(ms, 3), **baking.LAST_STATS, peak_alloc_bytes=int(peak))
        if not args.no_reference:
            ref = lambda: baking.bake_set(view, model, means, n, 16, 32, fused=False)  # noqa: E731
            rms = _time(ref, 1)
            rec.update(reference_ms=round(rms, 1), speedup=round(rms / ms, 1))
        print(json.dumps(rec), flush=True)
        del model, means
        torch.cuda.empty_cache()
    P = 200000
    occ = torch.rand((P, 16, 32, 1), device="cuda")
    env = torch.rand((1, 16, 32), device="cuda") * 0.01
    k = lambda: baking.env_occlusion(occ, env)  # noqa: E731
    t = lambda: (torch.clamp(occ, min=0, max=1) * env.permute(1, 2, 0)).sum(dim=(1, 2)).repeat(1, 3).clamp(min=0.0, max=1.0)  # noqa: E731
    k(), t()
    kms, tms = _time(k, 20), _time(t, 20)
    nbytes = occ.numel() * 4
    print(json.dumps(dict(what="env_reduce", P=P, kernel_ms=round(kms, 4), torch_ms=round(tms, 4), bytes_read=nbytes,
                          kernel_GBps=round(nbytes / kms / 1e6, 1))), flush=True)


if __name__ == "__main__":
    main()
