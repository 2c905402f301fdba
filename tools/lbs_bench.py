"""LBS kernels at SMPL (24 joints) or SMPL-X (55 joints) size: forward and forward + backward at 200k points, with and without
learned skinning-weight offsets, and the pose-blend-shape GEMV (forward and transposed) with its achieved HBM rate.

    python tools/lbs_bench.py --joints 24            # V = 6890, posedirs K = 207
    python tools/lbs_bench.py --joints 55            # V = 10475, K = 486
    python tools/lbs_bench.py --joints 55 --verts 6890 --points 100000

Prints one line per measurement and a final JSON line.  Times are per call (median of --reps timed batches of --iters calls)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mygauhuman_amd import human_synth, lbs  # noqa: E402

DEFAULT_VERTS = {24: 6890, 55: 10475}


def timed(fn, iters, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / iters * 1e6)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--joints", type=int, choices=(24, 55), default=24)
    ap.add_argument("--verts", type=int, default=None)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    J, V, P = a.joints, a.verts or DEFAULT_VERTS[a.joints], a.points
    body = human_synth.body_arrays(V, 0, "smpl" if J == 24 else "smplx")
    rng = np.random.default_rng(0)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()  # noqa: E731
    verts, w = d(body["v_template"]), d(body["weights"])
    q = (verts[torch.from_numpy(rng.integers(0, V, P)).cuda()] + 0.01 * torch.randn(P, 3, device="cuda")).requires_grad_(True)
    n = torch.randn(P, 3, device="cuda", requires_grad=True)
    A_big = torch.eye(4, device="cuda").repeat(J, 1, 1) + 0.01 * torch.randn(J, 4, 4, device="cuda")
    A_big[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda")
    A_pose = (A_big + 0.01).clone().requires_grad_(True)
    z = torch.zeros(V, 3, device="cuda")
    off_pose = z.clone().requires_grad_(True)
    loff = (0.1 * torch.randn(P, J, device="cuda")).requires_grad_(True)
    R, Th = torch.eye(3, device="cuda"), torch.zeros(3, device="cuda")
    res = dict(joints=J, verts=V, points=P)

    for with_off in (False, True):
        lo = loff if with_off else None
        tag = "offsets" if with_off else "plain"

        def fwd():
            with torch.no_grad():
                lbs.lbs_deform(q, n, lo, A_big, A_pose, z, z, off_pose, R, Th, verts, w, lean=True)

        def fwd_bwd():
            for t in (q, n, A_pose, off_pose, loff):
                t.grad = None
            o = lbs.lbs_deform(q, n, lo, A_big, A_pose, z, z, off_pose, R, Th, verts, w, lean=True)
            (o["world_pts"].sum() + o["transforms"].sum() + o["world_normals"].sum()).backward()
        res[f"fwd_{tag}_us"] = round(timed(fwd, a.iters, a.reps), 1)
        res[f"fwd_bwd_{tag}_us"] = round(timed(fwd_bwd, a.iters, a.reps), 1)
        print(f"LBS J={J} V={V} P={P} {tag:8s} forward {res[f'fwd_{tag}_us']:8.1f} us   forward+backward "
              f"{res[f'fwd_bwd_{tag}_us']:8.1f} us", flush=True)

    pd = d(body["posedirs"]).reshape(V * 3, -1)
    K = pd.shape[1]
    vec = torch.randn(K, device="cuda")
    g = torch.randn(V * 3, device="cuda")
    out, dv = torch.empty(V * 3, device="cuda"), torch.empty(K, device="cuda")
    from mygauhuman_amd._lib import check, lib, ptr
    s = torch.cuda.current_stream().cuda_stream
    gemv = lambda: check(lib.gsr_gemv_rows(V * 3, K, ptr(pd), ptr(vec), ptr(out), s), "gsr_gemv_rows")  # noqa: E731
    gemv_t = lambda: check(lib.gsr_gemv_rows_t(V * 3, K, ptr(pd), ptr(g), ptr(dv), s), "gsr_gemv_rows_t")  # noqa: E731
    mb = pd.numel() * 4 / 1e6
    for name, fn in (("gemv", gemv), ("gemv_t", gemv_t)):
        us = timed(fn, 100, a.reps)
        res[f"{name}_us"], res[f"{name}_GBps"] = round(us, 2), round(mb * 1e6 / us / 1e3, 0)
        print(f"pose-blend {name:7s} [{V * 3} x {K}] {mb:.1f} MB: {us:7.2f} us = {res[f'{name}_GBps']:.0f} GB/s", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
