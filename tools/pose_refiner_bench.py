"""The pose-correction network (csrc/pose_refiner.hip, nets_pose.FusedBodyPoseRefiner) against the same module in torch ops, at
B = 1 pose row and J = 24 / 55: forward and forward + backward, eager (host launches included) and captured as one graph; then the
render() motion step with both reference-sized networks (decoder="reference_size", pose_decoder="reference_size" vs
"reference_size_torch") recorded by graph.GraphedFrame, A/B interleaved.  Prints the shader clock it ran at.
python tools/pose_refiner_bench.py [--reps N] [--points P] [--size S]"""
import argparse
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mygauhuman_amd import _lib, human_synth, nets_pose  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--points", type=int, default=200_000)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()


def timed(fn, n):
    """mean ms per call over n calls (CUDA events around the whole loop: host launch cost included when fn launches eagerly)"""
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def micro(J):
    torch.manual_seed(0)
    m = nets_pose.FusedBodyPoseRefiner(total_bones=J, embedding_size=3 * (J - 1), mlp_width=128, mlp_depth=2).cuda()
    with torch.no_grad():
        m.block_mlps[4].weight.mul_(2e3)
    poses = torch.randn(1, 3 * J, device="cuda") * 0.3
    x = poses[:, 3:]                                   # the strided view render() passes
    gR = torch.randn(1, J - 1, 3, 3, device="cuda")
    params = list(m.parameters())
    out = {}
    for fused in (True, False):
        m.use_fused = fused

        def fwd():
            with torch.no_grad():
                return m(x)["Rs"]

        def both():
            return torch.autograd.grad((m(x)["Rs"] * gR).sum(), params)

        out[fused] = (timed(fwd, args.reps), timed(both, args.reps), timed(graphed(fwd), args.reps), timed(graphed(both), args.reps))
    for fused, name in ((True, "fused    "), (False, "torch ops")):
        f, fb, gf, gfb = out[fused]
        print(f"J={J} B=1 {name}  forward eager {f * 1e3:7.1f} us   fwd+bwd eager {fb * 1e3:7.1f} us   "
              f"forward graph {gf * 1e3:6.1f} us   fwd+bwd graph {gfb * 1e3:6.1f} us", flush=True)


def render_step(pose_decoder):
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.graph import GraphedFrame
    model, body = human_synth.build(args.points, None, "cuda", seed=0, motion=True, decoder="reference_size",
                                    pose_decoder=pose_decoder)
    cam = human_synth.view_camera(body, args.size, args.size, 0, n_views=8, device="cuda")
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = torch.zeros(3, device="cuda")
    params = list(model.parameters()) + list(model.pose_decoder.parameters()) + list(model.lweight_offset_decoder.parameters())

    def step():
        o = render(1, cam, model, pipe, bg)
        (o["render"].mean() + o["render_alpha"].mean() + o["normal"].mean()).backward()
        return o["render"]

    return GraphedFrame(step, warmup=3, zero_grads=params)


print(f"shader clock (settled): {_lib.settle_clock()[-1][1]:.3f} GHz", flush=True)
for J in (24, 55):
    micro(J)
frames = {k: render_step(k) for k in ("reference_size", "reference_size_torch")}
res = {k: [] for k in frames}
for _ in range(args.rounds):
    for k, f in frames.items():
        res[k].append(timed(f.replay, 50))
for k, v in res.items():
    v = sorted(v)
    print(f"render() motion step, {args.points} Gaussians, {args.size}², one graph, pose_decoder={k:22s} "
          f"median {v[len(v) // 2]:.3f} ms per frame (min {v[0]:.3f}, max {v[-1]:.3f}, {args.rounds} rounds x 50 replays)", flush=True)
print(f"shader clock after: {_lib.clock_probe()[0]:.3f} GHz", flush=True)
