"""Event-timed WHOLE PBR training step with the geometry frozen as the reference freezes it after pbr_iteration
(scene/gaussian_model.py:296-306): render() -> build_mips -> pbr_shading -> PbrPhaseLoss + ssim_crop + env_tv_loss -> backward ->
FusedAdam step for the materials and the light, on the bench scene (200k articulated Gaussians, 1024^2, a baked camera).

    python tools/pbr_step_bench.py [--modes full,materials] [--repeats 7] [--steps 20] [--P 200000] [--size 1024] [--lut FILE]

  full        render() as it is by default: the full rasterizer backward (21-channel blend backward + backward preprocess), the
              attribute, activation and LBS backward.  This mode uses nothing newer than the frozen-geometry phase itself, so the
              same file run on an older checkout gives the baseline.
  materials   render(..., geometry_grad=False): the colour-only blend backward (csrc/blend_colors_bwd.hip).

Each mode is timed eagerly and as ONE graph (graph.GraphedFrame(verify=False), the optimizer steps inside).  A repeat is --steps steps
between two device events; the modes alternate inside every repeat; the lines give the median, the minimum and the maximum over the
repeats in ms per step.  The shader clock is settled first and printed, as bench.py does.  Afterwards, with the stage events on,
the per-frame time of stages 3 (blend forward), 4 (blend backward), 5 (backward preprocess) and 6 (blend backward, colours only)
of gsr_profile_read.
One JSON line per figure."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import types

# GraphedFrame(verify=False) stands on this (mygauhuman_amd/graph.py); read when the HIP runtime starts
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GEOMETRY = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
MATERIALS = ("_albedo", "_roughness", "_normal")


def build_scene(P, S, lut_path, dev):
    import mygauhuman_amd
    from mygauhuman_amd import baking, human_synth
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.pbr import CubemapLight, get_brdf_lut
    s = types.SimpleNamespace(H=S, W=S)
    s.model, body = human_synth.build(P, 6890, dev, seed=0)
    s.cam = human_synth.view_camera(body, S, S, 0, n_views=8, device=dev)
    s.pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    s.bg = torch.zeros(3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    s.env = torch.rand((1, 16, 32), device=dev, generator=gen) * 0.01
    torch.manual_seed(0)
    s.cubemap = CubemapLight(base_res=32).to(dev)   # train.py:150
    s.lut = get_brdf_lut(lut_path).to(dev)
    s.envmap_dirs = baking.get_envmap_dirs([256, 512], device=dev)[1].contiguous()
    s.cam.occlusion = None
    mygauhuman_amd.install_dropin(bake=True)
    with torch.no_grad():   # bakes the camera once (a bake cannot run inside a capture)
        out = gr.render(30001, s.cam, s.model, s.pipe, s.bg, envmap=s.env)
    assert s.cam.occlusion is not None
    s.view_dirs = torch.nn.functional.normalize(torch.randn(S, S, 3, device=dev, generator=gen), dim=-1)
    s.gt = torch.rand(3, S, S, device=dev, generator=gen)
    bound = torch.zeros((1, S, S), device=dev)
    bound[:, S // 8: S - S // 8, S // 4: S - S // 4] = 1.0   # a box around the subject, ~38 % of the pixels
    s.bound = bound
    s.rect = torch.zeros(4, dtype=torch.int32, device=dev)
    s.knn = torch.randint(0, P, (P, 3), device=dev, generator=gen)
    s.knn[:, 0] = torch.arange(P, device=dev)
    s.coverage = float((out["render_alpha"] > 0.05).float().mean())
    # the freeze of update_learning_rate after pbr_iteration (the bench scene has its motion decoders off)
    for n in GEOMETRY:
        getattr(s.model, n).requires_grad_(False)
    return s


def make_step(s, mode, opts):
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss, bounding_rect, env_tv_loss, pbr_shading, ssim_crop
    fused = PbrPhaseLoss(s.gt, s.bound, MaterialSmoothness(s.knn))
    kw = {} if mode == "full" else {"geometry_grad": False}

    def step():
        o = gr.render(30001, s.cam, s.model, s.pipe, s.bg, envmap=s.env, **kw)
        s.cubemap.build_mips()
        alpha = o["render_alpha"]
        rough = o["roughness"][0:1] * (1.0 - 0.04) + 0.04
        res = pbr_shading(light=s.cubemap, normals=o["world_normal"].permute(1, 2, 0).detach(), view_dirs=s.view_dirs,
                          mask=alpha.permute(1, 2, 0), albedo=o["albedo"].permute(1, 2, 0), roughness=rough.permute(1, 2, 0),
                          metallic=None, tone=False, gamma=False, occlusion=o["occlusion"][0:1].permute(1, 2, 0), brdf_lut=s.lut)
        rgb = res["render_rgb"].permute(2, 0, 1)
        loss, _terms = fused(rgb, alpha, o["albedo"], rough, s.model.get_albedo, s.model.get_roughness)
        bounding_rect(s.bound, out=s.rect)
        loss = loss + 0.01 * (1.0 - ssim_crop(rgb, s.gt, s.rect)) + 0.01 * env_tv_loss(s.cubemap, s.envmap_dirs)
        loss.backward()
        for o_ in opts:
            o_.step()
        return loss.detach()
    return step


def drop_light_graph(s):
    """CubemapLight.build_mips keeps its mip chain -- and with it the autograd graph down to the gradient-accumulation node of
    `base` -- on the module until the next call, and the next call's graph picks that same node up again.  A node made by an eager
    step on the default stream would pull a later CAPTURED backward onto the default stream (not allowed inside a capture); dropped
    here, the node dies and the next step makes its own on the stream it runs on."""
    s.cubemap.specular = s.cubemap.diffuse = None


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def stage_ms(lib, stage):
    ms, n = C.c_double(0), C.c_long(0)
    if lib.gsr_profile_read(stage, C.byref(ms), C.byref(n)) != 0:
        return None   # a library without that stage
    return (round(ms.value / n.value, 4) if n.value else 0.0), n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="full,materials")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--P", type=int, default=200_000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--lut", default=os.path.join(ROOT, "tests", "golden", "pbr_brdf_256_256.bin"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least 5 (the figure is a median with its spread)")
    modes = [m for m in args.modes.split(",") if m]
    assert all(m in ("full", "materials") for m in modes), modes
    from mygauhuman_amd import _lib
    from mygauhuman_amd.graph import GraphedFrame
    from mygauhuman_amd.optim import FusedAdam
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    s = build_scene(args.P, args.size, args.lut, dev)
    params = [getattr(s.model, n) for n in GEOMETRY + MATERIALS]
    opt = FusedAdam([{"params": [p], "lr": 1e-4} for p in params], eps=1e-15)
    light_opt = FusedAdam([{"params": [s.cubemap.base], "lr": 1e-4, "clamp_min": 0.0}], eps=1e-15)
    opts = (opt, light_opt)
    every = params + [s.cubemap.base]
    clock = _lib.settle_clock(dev)
    print(json.dumps({"what": "scene", "P": args.P, "pixels": f"{args.size}x{args.size}", "alpha_coverage": round(s.coverage, 3),
                      "frozen": list(GEOMETRY), "modes": modes, "steps_per_repeat": args.steps, "repeats": args.repeats,
                      "clock_ghz_settled": clock[-1][1], "settle_ms": clock[-1][0]}), flush=True)

    steps = {m: make_step(s, m, opts) for m in modes}
    drop_light_graph(s)

    def eager(m):
        def run():
            for p in every:
                p.grad = None
            steps[m]()
        return run
    runs = {(m, "eager"): eager(m) for m in modes}
    for m in modes:
        for _ in range(args.warmup):
            runs[(m, "eager")]()
    torch.cuda.synchronize()
    for o_ in opts:
        o_.sync_lr()
    frames = {}
    for m in modes:
        drop_light_graph(s)
        for p in every:
            p.grad = None
        frames[m] = GraphedFrame(steps[m], warmup=3, zero_grads=every, verify=False)

        def replay(f=frames[m]):
            for o_ in opts:
                o_.sync_lr()
            f.replay()
        runs[(m, "one_graph")] = replay
        for _ in range(args.warmup):
            replay()
    torch.cuda.synchronize()
    for f in frames.values():
        f.check()
    drop_light_graph(s)
    for m in modes:   # (eager again: its autograd nodes are made on this stream)
        runs[(m, "eager")]()
    _lib.settle_clock(dev)
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):   # the modes alternate inside every repeat
        for k, fn in runs.items():
            ms[k].append(timed(fn, args.steps))
    for (m, how), v in ms.items():
        print(json.dumps({"what": "pbr_step", "backward": m, "how": how, "ms_per_step_median": round(statistics.median(v), 4),
                          "min": round(min(v), 4), "max": round(max(v), 4), "spread": round(max(v) - min(v), 4),
                          "repeats": [round(x, 4) for x in v]}), flush=True)
    print(json.dumps({"what": "clock_after", "clock_ghz": round(_lib.clock_probe(1024, 1 << 19, dev)[0], 4)}), flush=True)
    # ---- the rasterizer's backward stages on that frame (stage events on: a pass of its own, eager)
    for m in modes:
        _lib.check(_lib.lib.gsr_profile_enable(0b1111000), "gsr_profile_enable")
        _lib.check(_lib.lib.gsr_profile_reset(), "gsr_profile_reset")
        for _ in range(10):
            runs[(m, "eager")]()
        torch.cuda.synchronize()
        rec = {"what": "backward_stages_ms_per_frame", "backward": m}
        for name, stage in (("blend_fwd", 3), ("blend_bwd", 4), ("preprocess_bwd", 5), ("blend_bwd_colors", 6)):
            r = stage_ms(_lib.lib, stage)
            rec[name] = None if r is None else r[0]
            rec[name + "_launches"] = None if r is None else r[1]
        _lib.check(_lib.lib.gsr_profile_enable(0), "gsr_profile_enable")
        print(json.dumps(rec), flush=True)
    final = {n: float(getattr(s.model, n).detach().abs().sum()) for n in GEOMETRY}
    print(json.dumps({"what": "frozen_parameter_checksums", **{k: round(v, 3) for k, v in final.items()}}), flush=True)


if __name__ == "__main__":
    main()
