"""Event-timed SSIM term of train.py:269-281 (image and normal on the bound-mask crop), forward + backward, three ways:

    python tools/ssim_crop_bench.py [--reps 30] [--rounds 5] [--size 1024]

  (a) "host_rect"   as train.py writes it: the box read on the host (mask -> CPU -> numpy min / max, standing in for cv2.boundingRect),
                    the four slices, two loss_utils.ssim() calls and their backward
  (b) "known_rect"  the same with the box already known on the host: the best case of the composition
  (c) "ssim_crop"   loss_utils.bounding_rect + the two-group loss_utils.ssim_crop: no host read (csrc/ssim_crop.hip)

at a standing-human box (about 400 x 800 of 1024^2) and at the full frame.  The variants alternate within a round and every round
prints its own median (milliseconds per call over --reps calls), so the spread between rounds is visible next to the difference
between variants; the kernel launches of one call of each variant are counted with the torch profiler.  One JSON line each."""
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


def launches(fn):
    """{kernel name: count} of one call."""
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


def human_mask(S, x, y, w, h):
    m = torch.zeros(S, S)
    m[y:y + h // 6, x + w // 3:x + 2 * w // 3] = 1
    m[y + h // 6:y + h // 2, x:x + w] = 1
    m[y + h // 2:y + h, x + w // 8:x + 3 * w // 8] = 1
    m[y + h // 2:y + h, x + 5 * w // 8:x + 7 * w // 8] = 1
    return m


def host_rect(bound):
    ys, xs = np.nonzero(bound[0].cpu().numpy().astype(np.uint8))
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    from mygauhuman_amd import _lib, loss_utils
    ghz = _lib.settle_clock()[-1][1]
    S = args.size
    gen = torch.Generator(device="cuda").manual_seed(0)
    gt, gt_normal = (torch.rand(3, S, S, device="cuda", generator=gen) for _ in range(2))
    image = (gt + 0.1 * torch.randn(3, S, S, device="cuda", generator=gen)).clamp(0, 1).requires_grad_(True)
    normal = (gt_normal + 0.1 * torch.randn(3, S, S, device="cuda", generator=gen)).clamp(0, 1).requires_grad_(True)
    leaves = (image, normal)
    boxes = {"human": (S * 5 // 16, S // 10, S * 25 // 64, S * 25 // 32), "full_frame": (0, 0, S, S)}
    for box_name, box in boxes.items():
        bound = human_mask(S, *box).cuda()[None].contiguous()
        assert host_rect(bound) == box
        rect = torch.zeros(4, dtype=torch.int32, device="cuda")

        def composition(x, y, w, h):
            crop = lambda t: t[:, y:y + h, x:x + w].unsqueeze(0)  # noqa: E731
            s = loss_utils.ssim(crop(image), crop(gt)) + loss_utils.ssim(crop(normal), crop(gt_normal))
            torch.autograd.backward(0.01 * (2.0 - s), inputs=leaves)

        def run_a():
            composition(*host_rect(bound))

        def run_b():
            composition(*box)

        def run_c():
            loss_utils.bounding_rect(bound, out=rect)
            s_img, s_nrm = loss_utils.ssim_crop((image, normal), (gt, gt_normal), rect)
            torch.autograd.backward(0.01 * (2.0 - (s_img + s_nrm)), inputs=leaves)

        variants = (("host_rect", run_a), ("known_rect", run_b), ("ssim_crop", run_c))
        grads = {}
        for name, fn in variants:   # warm-up, and the three must agree
            for _ in range(5):
                image.grad = normal.grad = None
                fn()
            grads[name] = (image.grad.clone(), normal.grad.clone())
        for name in ("host_rect", "ssim_crop"):
            for got, want in zip(grads[name], grads["known_rect"]):
                assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()), name
        assert tuple(rect.tolist()) == box
        for rnd in range(args.rounds):
            for name, fn in variants:
                print(json.dumps({"what": "ssim_term_fwd_bwd", "box": box_name, "rect": box, "pixels": f"{S}x{S}", "variant": name,
                                  "round": rnd, "ms": round(timed(fn, args.reps), 4), "clock_ghz": ghz}), flush=True)
        for name, fn in variants:
            k = launches(fn)
            print(json.dumps({"what": "kernel_launches", "box": box_name, "variant": name, "total": sum(k.values()), "kernels": k}),
                  flush=True)


if __name__ == "__main__":
    main()
