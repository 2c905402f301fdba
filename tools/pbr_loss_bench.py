"""Event-timed PBR-phase training loss (csrc/pbr_loss.hip, PbrPhaseLoss) against the torch composition of train.py:316-344.

    python tools/pbr_loss_bench.py [--reps 50] [--P 200000]

Prints one JSON line per measurement (milliseconds per call, median of --reps after warm-up): forward + backward of the five
terms (masked L1, masked TV of [albedo; roughness], the two histogram entropies, the material smoothness over knn, the roughness
prior) at 512^2 and 1024^2 pixels with P Gaussians, for the fused path ("hip") and the torch composition ("torch_fp32", whose
boolean indexing and entropy branches read the device).  The shader clock is settled and reported as in tools/pbr_bench.py."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
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


def _entropy(x):
    """train.py:47-71 as torch ops."""
    v = x.view(-1, x.shape[-1])
    sigma = v.var(dim=0)
    centers = (torch.arange(15, device=x.device, dtype=x.dtype) + 0.5) / 15
    h = ((-0.5 * ((v[None] - centers[:, None, None]) / sigma).pow(2)).exp() / (sigma * np.sqrt(np.pi * 2)) * (1.0 / 15)).sum(1)
    e = 0
    for i in range(3):
        hi = h[..., i]
        hi = hi / hi.sum() + 1e-6 if hi.sum() > 1e-6 else torch.ones_like(hi)
        e = e + torch.sum(-hi * torch.log(hi))
    return e


def composition(rgb, gt, bound, alpha, albedo, rough, ga, gr, knn):
    sel = bound[0] == 1
    l1 = (rgb.permute(1, 2, 0)[sel] - gt.permute(1, 2, 0)[sel]).abs().mean()
    pred = torch.cat([albedo, rough], 0)
    m = alpha.float()
    tv = ((pred[:, 1:] - pred[:, :-1]) ** 2 * (m[:, 1:] * m[:, :-1])).mean() + \
        ((pred[:, :, 1:] - pred[:, :, :-1]) ** 2 * (m[:, :, 1:] * m[:, :, :-1])).mean()

    def sm(g):
        a, b = g[knn][:, 1], g[knn][:, 2]
        return (torch.abs(a - b) / (b + 1e-6)).mean()
    lamb = (1.0 - rough[alpha > 0]).mean()
    return l1 + tv + 5e-5 * (_entropy(albedo) + _entropy(rough)) + 0.1 * (sm(ga) + sm(gr)) + 0.001 * lamb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--P", type=int, default=200_000)
    args = ap.parse_args()
    from mygauhuman_amd import _lib
    from mygauhuman_amd.pbr import PbrPhaseLoss
    ghz = _lib.settle_clock()[-1][1]
    gen = torch.Generator(device="cuda").manual_seed(0)
    P = args.P
    knn = torch.randint(0, P, (P, 3), device="cuda", generator=gen)
    knn[:, 0] = torch.arange(P, device="cuda")
    ga = (torch.rand(P, 3, device="cuda", generator=gen) * 0.98 + 0.02).requires_grad_(True)
    gr = (torch.rand(P, 3, device="cuda", generator=gen) * 0.98 + 0.02).requires_grad_(True)
    for S in (512, 1024):
        hwc = torch.rand(S, S, 3, device="cuda", generator=gen).requires_grad_(True)
        rgb = hwc.permute(2, 0, 1)
        gt = torch.rand(3, S, S, device="cuda", generator=gen)
        bound = (torch.rand(1, S, S, device="cuda", generator=gen) > 0.3).float()
        alpha = torch.rand(1, S, S, device="cuda", generator=gen).requires_grad_(True)
        albedo = torch.rand(3, S, S, device="cuda", generator=gen).requires_grad_(True)
        rough = (torch.rand(1, S, S, device="cuda", generator=gen) * 0.96 + 0.04).requires_grad_(True)
        fused = PbrPhaseLoss(gt, bound, knn)
        leaves = (hwc, alpha, albedo, rough, ga, gr)

        def run_fused():
            torch.autograd.backward(fused(rgb, alpha, albedo, rough, ga, gr)[0], inputs=leaves)

        def run_torch():
            torch.autograd.backward(composition(rgb, gt, bound, alpha, albedo, rough, ga, gr, knn), inputs=leaves)
        for impl, fn in (("hip", run_fused), ("torch_fp32", run_torch)):
            print(json.dumps({"what": "pbr_loss_fwd_bwd", "impl": impl, "pixels": f"{S}x{S}", "P": P,
                              "ms": round(timed(fn, args.reps), 4), "clock_ghz": ghz}), flush=True)
        for leaf in leaves:
            leaf.grad = None


if __name__ == "__main__":
    main()
