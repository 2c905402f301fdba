"""Event-timed environment-light side of a PBR step (csrc/pbr.hip) against the same arithmetic as it stood before
the fused calls existed, each eager and replayed as one captured graph:

    python tools/env_light_bench.py [--reps 20] [--inner 20] [--rounds 5] [--out profiles/env_light_bench.txt]

  grey_envmap   CubemapLight.grey_envmap(res [16, 32], out=)  vs  export_envmap(return_img=True) + clamp + the grey weights
  env_tv        env_tv_loss(base, dirs [256, 512]) forward + backward, with both gradient reductions (window / whole)
                vs  nvdiffrast.torch.texture + the two torch squared-difference means, forward + backward
  view_dirs     pbr.view_dirs(out=) at 512^2 and 1024^2  vs  evaluate.view_dirs_of (torch.inverse reads its status on the host,
                so it cannot be captured: its graph figure is the composition with the inverse formed outside the graph)

N = 32 everywhere (the only light size the reference uses).  The variants of one measurement alternate within a round and every
round prints its own median (milliseconds per call: --inner calls between two events, the median over --reps such windows), so
the spread between rounds stands next to the difference between variants; the shader clock the run settled at is in every line.
Kernel launches of one call are counted with the torch profiler.  One JSON line each."""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GREY = (0.2989, 0.587, 0.114)
OUT = None


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


def timed(fn, reps, inner):
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
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


def graphed(fn, warmup=3):
    """fn captured into one graph (after `warmup` eager calls on the capture stream); returns the replay callable."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    torch.cuda.synchronize()
    return g.replay


def measure(what, variants, args, ghz, graph_variants=None, **tags):
    """variants: [(name, fn)].  Eager rounds, then the same as graphs (graph_variants replaces the list where a variant cannot be
    captured), then launch counts."""
    for name, fn in variants:
        for _ in range(5):
            fn()
    for mode, vs in (("eager", variants), ("graph", [(n, graphed(f)) for n, f in (graph_variants or variants)])):
        for rnd in range(args.rounds):
            for name, fn in vs:
                emit(what=what, mode=mode, variant=name, round=rnd, ms=round(timed(fn, args.reps, args.inner), 5), clock_ghz=ghz,
                     **tags)
    for name, fn in variants:
        k = launches(fn)
        emit(what=what + "_launches", variant=name, total=sum(k.values()), kernels=k, **tags)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        OUT = open(args.out, "w")
    import mygauhuman_amd.nvdiffrast.torch as dr
    from mygauhuman_amd import _lib, baking, evaluate
    from mygauhuman_amd.pbr import CubemapLight, env_tv_loss, view_dirs
    from tests import pbr_reference as PR
    ghz = _lib.settle_clock()[-1][1]
    torch.manual_seed(0)
    light = CubemapLight(base_res=32).cuda()
    base = light.base

    # ---- grey map ------------------------------------------------------------------------------------------------------------
    env = torch.empty(1, 16, 32, device="cuda")

    def grey_fused():
        light.grey_envmap([16, 32], out=env)

    def grey_composition():
        with torch.no_grad():
            img = light.export_envmap(return_img=True, res=[16, 32]).permute(2, 0, 1).clamp(0.0, 1.0)
            return (GREY[0] * img[0] + GREY[1] * img[1] + GREY[2] * img[2])[None]

    assert float((grey_composition() - light.grey_envmap([16, 32])).abs().max()) <= 1e-6
    measure("grey_envmap", [("fused", grey_fused), ("composition", grey_composition)], args, ghz, res=[16, 32], N=32)

    # ---- environment-map TV ------------------------------------------------------------------------------------------------------
    dirs = torch.from_numpy(PR.envmap_dirs([256, 512]).astype(np.float32)).cuda().contiguous()

    def tv(reduce):
        def run():
            base.grad = None
            env_tv_loss(base, dirs, reduce=reduce).backward()
        return run

    def tv_composition():
        base.grad = None
        em = dr.texture(base[None], dirs[None], filter_mode="linear", boundary_mode="cube")[0]
        (((em[1:] - em[:-1]) ** 2).mean() + ((em[:, 1:] - em[:, :-1]) ** 2).mean()).backward()

    tv_composition()
    want = base.grad.clone()
    for r in (_lib.ENV_TV_WINDOW, _lib.ENV_TV_WHOLE):
        tv(r)()
        assert float((base.grad - want).abs().max()) <= 1e-4 * float(want.abs().max()), r
    measure("env_tv_fwd_bwd", [("fused_window", tv(_lib.ENV_TV_WINDOW)), ("fused_whole", tv(_lib.ENV_TV_WHOLE)),
                               ("fused_auto", tv(_lib.ENV_TV_AUTO)), ("composition", tv_composition)], args, ghz, dirs=[256, 512], N=32)

    # ---- view directions -----------------------------------------------------------------------------------------------------------
    from mygauhuman_amd import cameras
    for S in (512, 1024):
        cam = cameras.look_at_camera(S, S, [0.3, -0.1, -2.6], [0.0, -0.1, 0.0])
        view = types.SimpleNamespace(world_view_transform=torch.from_numpy(np.asarray(cam["viewmatrix"], np.float32)).cuda())
        rays = baking.get_canonical_rays(S, S, cam["tanfovx"], cam["tanfovy"], device="cuda").float().contiguous()
        vd = torch.empty(S, S, 3, device="cuda")
        c2w = torch.inverse(view.world_view_transform.T)

        def vd_fused():
            view_dirs(rays, view.world_view_transform, S, S, out=vd)

        def vd_composition():
            return evaluate.view_dirs_of(view, rays, S, S)

        def vd_known_inverse():
            r = torch.nn.functional.normalize(rays[:, None, :], p=2, dim=-1)
            return -((r * c2w[None, :3, :3]).sum(dim=-1).reshape(S, S, 3))

        vd_fused()
        assert float((vd - vd_composition()).abs().max()) <= 1e-5
        measure("view_dirs", [("fused", vd_fused), ("composition", vd_composition), ("composition_known_inverse", vd_known_inverse)],
                args, ghz, graph_variants=[("fused", vd_fused), ("composition_known_inverse", vd_known_inverse)], pixels=f"{S}x{S}")


if __name__ == "__main__":
    main()
