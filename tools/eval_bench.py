"""Event-timed evaluation view (render.py:186-350), PBR branch on, three ways:

    python tools/eval_bench.py [--size 1024] [--points 200000] [--views 8] [--repeats 3] [--out profiles/eval_bench.json]

  "baseline"      what the package offered before evaluate.py: our render() + pbr_shading, then the reference's post-processing and
                  metrics as torch ops (tests/eval_reference.finish_torch: eleven masked fills with .item(), thirteen clamps;
                  save_image's quantisation chain per image; psnr; loss_utils.ssim(...).mean())
  "fused"         evaluate.finish_view (csrc/eval.hip), eager
  "fused_graph"   the whole frame recorded once into graph.GraphedFrame and replayed (whole view only)

Two figures per variant, milliseconds per view from device events around work that ends in a synchronise: the post-render part alone
(on copies of one view's thirteen images, the copies outside the timed region) and the whole view over --views ring cameras.  The
variants alternate within a repeat; every repeat is reported, so the spread is visible next to the difference.  Kernel launches and
device-to-host copies of one view are counted with the torch profiler.  One JSON line each; --out also writes them to a file."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def census(fn):
    """(kernel launches, device-to-host copies) of one call."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    k = d2h = 0
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA:
            continue
        name = e.name.lower()
        if "memcpy" in name:
            d2h += "dtoh" in name or "device -> host" in name or "devicetohost" in name
        elif "memset" not in name:
            k += 1
    return k, d2h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mygauhuman_amd import _lib, evaluate, human_synth, loss_utils
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.graph import GraphedFrame
    from mygauhuman_amd.pbr import CubemapLight, get_brdf_lut, pbr_shading
    from tests import eval_reference as R
    S, it = args.size, 3001
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    ghz = _lib.settle_clock()[-1][1]
    model, body = human_synth.build(args.points, device="cuda", seed=0)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True, sync_free_raster=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    views = []
    for k in range(args.views):
        cam = human_synth.view_camera(body, S, S, k, n_views=args.views)
        cam.original_image = torch.rand(3, S, S, device="cuda", generator=gen)
        cam.original_normal = torch.rand(3, S, S, device="cuda", generator=gen)
        m = torch.zeros(1, S, S, device="cuda")
        m[:, S // 10:S * 9 // 10, S * 5 // 16:S * 11 // 16] = 1
        cam.bound_mask = m
        views.append(cam)
    bg = torch.zeros(3, device="cuda")
    light = CubemapLight(base_res=32).cuda()
    with torch.no_grad():
        light.base.copy_(torch.rand(light.base.shape, device="cuda", generator=gen))
        light.build_mips()
    lut = get_brdf_lut(os.path.join(ROOT, "tests", "golden", "pbr_brdf_256_256.bin")).cuda()
    rays = torch.randn(S * S, 3, device="cuda", generator=gen)
    view_dirs = evaluate.view_dirs_of(views[0], rays, S, S)

    def frame_images(view):
        """render() + pbr_shading: the thirteen images of one view, unfinished (the part every variant shares)."""
        out = render(it, view, model, pipe, bg)
        images = {n: out[k] for n, k in evaluate._RENDER_KEYS}
        occ = out["occlusion"]
        r = pbr_shading(light=light, normals=out["world_normal"].permute(1, 2, 0).detach(), view_dirs=view_dirs,
                        mask=out["render_alpha"].permute(1, 2, 0), albedo=out["albedo"].permute(1, 2, 0),
                        roughness=out["roughness"][0, ...].unsqueeze(0).permute(1, 2, 0), metallic=None, tone=False, gamma=False,
                        occlusion=occ.permute(1, 2, 0)[..., 0][..., None], brdf_lut=lut)
        images.update(render_pbr=r["render_rgb"].permute(2, 0, 1), render_diffuse=r["diffuse_rgb"].permute(2, 0, 1),
                      render_specular=r["specular_rgb"].permute(2, 0, 1), render_ao=occ)
        return images

    acc = torch.zeros(2, device="cuda", dtype=torch.float64)

    def post_baseline(images, view):
        images = dict(images, gt=view.original_image.clone(), gt_normal=view.original_normal.clone())
        fin = R.finish_torch(images, view.bound_mask, bg)
        u8 = [R.quantise_torch(t) for t in fin.values()]
        acc[0] += evaluate.psnr(fin["render_pbr"], fin["gt"]).mean().double()
        acc[1] += loss_utils.ssim(fin["render_pbr"], fin["gt"]).mean().double()
        return u8

    table = evaluate.EvalMetrics(1 << 16)

    def post_fused(images, view):
        images = dict(images, gt=view.original_image, gt_normal=view.original_normal)
        out = {"gt": torch.empty_like(view.original_image), "gt_normal": torch.empty_like(view.original_normal)}
        return evaluate.finish_view(images, view.bound_mask, bg, metrics=table, metric=("render_pbr", "gt"), to_uint8=list(images),
                                    out=out)

    with torch.no_grad():
        base_images = frame_images(views[0])
        torch.cuda.synchronize()

        def post_timed(post):
            ts = []
            for _ in range(args.reps):
                imgs = {n: t.clone(memory_format=torch.preserve_format) for n, t in base_images.items()}
                ts.append(events(lambda: post(imgs, views[0])))
            return float(np.median(ts))

        def whole(post):
            def run():
                for v in views:
                    post(frame_images(v), v)
            return run

        sv = evaluate._static_view(views[0], "cuda")
        graph = GraphedFrame(lambda: post_fused(frame_images(sv), sv))

        def whole_graph():
            for v in views:
                evaluate._static_update(sv, v)
                graph.replay()

        for fn in (whole(post_baseline), whole(post_fused), whole_graph):  # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        for rep in range(args.repeats):
            for name, post in (("baseline", post_baseline), ("fused", post_fused)):
                emit({"what": "post_render_ms_per_view", "variant": name, "repeat": rep, "ms": round(post_timed(post), 4),
                      "size": S, "clock_ghz": ghz})
            for name, fn in (("baseline", whole(post_baseline)), ("fused", whole(post_fused)), ("fused_graph", whole_graph)):
                table.reset()
                emit({"what": "whole_view_ms_per_view", "variant": name, "repeat": rep, "ms": round(events(fn) / len(views), 4),
                      "size": S, "points": args.points, "views": len(views), "clock_ghz": ghz})
        for name, post in (("baseline", post_baseline), ("fused", post_fused)):
            imgs = {n: t.clone(memory_format=torch.preserve_format) for n, t in base_images.items()}
            k, d2h = census(lambda: post(dict(imgs), views[0]))
            emit({"what": "post_render_census", "variant": name, "kernel_launches": k, "device_to_host_copies": d2h,
                  "counted_with": "torch.profiler"})
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "lines": lines}, f, indent=1)


if __name__ == "__main__":
    main()
