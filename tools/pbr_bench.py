"""Event-timed image-based-lighting stage (csrc/pbr.hip) against the same math as fp32 torch ops on the GPU.

    python tools/pbr_bench.py [--reps 50]

Prints one JSON line per measurement (milliseconds per call, median of --reps after warm-up):
  build_mips   CubemapLight(base_res=32).build_mips() forward + backward of a sum over every level;
  shade        pbr_shading forward, and forward + backward, at 512^2 and 1024^2 pixels (diffuse + 3 specular levels + LUT).
The torch baseline ("torch_fp32") runs the same composition with torch ops: cube taps by torch.where / gathers (the seam rule
of tests/pbr_reference.py), the prefilter as matrix products with the weight matrices built once outside the timed region
(so the baseline is not charged for them)."""
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

from tests import pbr_reference as R  # noqa: E402


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


# ---- torch fp32 baseline ---------------------------------------------------------------------------------------------------
def _sel(f, vals):
    out = vals[-1]
    for i in range(len(vals) - 2, -1, -1):
        out = torch.where(f == i, vals[i], out)
    return out


def _face_of(x, y, z):
    ax, ay, az = x.abs(), y.abs(), z.abs()
    return torch.where(az > torch.maximum(ax, ay), torch.where(z < 0, 5, 4),
                       torch.where(ay > ax, torch.where(y < 0, 3, 2), torch.where(x < 0, 1, 0)))


def _coords(f, x, y, z):
    return _sel(f, [-z, z, x, x, x, -x]), _sel(f, [-y, -y, z, -z, -y, -y]), _sel(f, [x, -x, y, -y, z, -z])


def _tap(f, x, y, N):
    ox, oy = (x < 0) | (x >= N), (y < 0) | (y >= N)
    a, b = 2 * x + 1 - N, 2 * y + 1 - N
    m = torch.full_like(a, N)
    dx, dy, dz = _sel(f, [m, -m, a, a, a, -a]), _sel(f, [-b, -b, m, -m, -b, -b]), _sel(f, [-a, a, b, -b, m, -m])
    g = _face_of(dx, dy, dz)
    a2, b2, m2 = _coords(g, dx, dy, dz)
    m2 = m2.clamp(min=1)
    nx = torch.div((a2 + m2) * N, 2 * m2, rounding_mode="floor").clamp(0, N - 1)
    ny = torch.div((b2 + m2) * N, 2 * m2, rounding_mode="floor").clamp(0, N - 1)
    return torch.where(~ox & ~oy, (f * N + y) * N + x, torch.where(ox & oy, -2, (g * N + ny) * N + nx))


def cube_lookup(tex, d):
    N, C = tex.shape[1], tex.shape[-1]
    f = _face_of(d[:, 0], d[:, 1], d[:, 2])
    a, b, m = _coords(f, d[:, 0], d[:, 1], d[:, 2])
    valid = m > 0
    ms = torch.where(valid, m, torch.ones_like(m))
    u, v = ((a / ms + 1) * 0.5).clamp(0, 1), ((b / ms + 1) * 0.5).clamp(0, 1)
    sx, sy = u * N - 0.5, v * N - 0.5
    x0, y0 = torch.floor(sx), torch.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.long(), y0.long()
    w = torch.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
    idx = torch.stack([_tap(f, x0, y0, N), _tap(f, x0 + 1, y0, N), _tap(f, x0, y0 + 1, N), _tap(f, x0 + 1, y0 + 1, N)], 1)
    corner = idx == -2
    w = torch.where(corner, torch.zeros_like(w), w + (w * corner).sum(1, keepdim=True) / 3.0)
    w = w * valid[:, None]
    flat = tex.reshape(-1, C)
    idx = idx.clamp(min=0)
    return sum(w[:, k:k + 1] * flat[idx[:, k]] for k in range(4))


def torch_shade(diffuse, specular, lut, n, v, albedo, rough, occ, mask):
    nv = (n * v).sum(-1, keepdim=True)
    ref = 2.0 * nv.clamp(min=0.0) * n - v
    dl = cube_lookup(diffuse.pow(1.0 / 2.2).clamp(0, 1), n) * occ
    nov = nv.clamp(1e-4, 1.0)
    fg = R.flat_sample(lut, torch.cat([nov, rough], -1))[:, 0:1]
    L = len(specular)
    lvl = torch.where(rough < 0.5, (rough.clamp(0.08, 0.5) - 0.08) / 0.42 * (L - 2), (rough.clamp(0.5, 1.0) - 0.5) / 0.5 + L - 2)
    lv = lvl[:, 0].clamp(0, L - 1)
    l0 = torch.floor(lv).detach()
    l1 = (l0 + 1).clamp(max=L - 1)
    t = (lv - l0)[:, None]
    spec = 0
    for i, s in enumerate(specular):
        spec = spec + ((1 - t) * (l0 == i)[:, None] + t * (l1 == i)[:, None]) * cube_lookup(s, ref)
    diffuse_rgb = dl * albedo
    specular_rgb = spec * (0.04 * fg)
    rgb = (diffuse_rgb + specular_rgb).clamp(0, 1)
    return torch.where(mask > 0, rgb, torch.zeros_like(rgb)), diffuse_rgb, specular_rgb, dl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from mygauhuman_amd import _lib
    from mygauhuman_amd.pbr import CubemapLight, pbr_shading
    torch.manual_seed(0)
    ghz = _lib.settle_clock()[-1][1]
    light = CubemapLight(base_res=32)

    def mips():
        light.base.grad = None
        light.build_mips()
        (light.diffuse.sum() + sum(s.sum() for s in light.specular)).backward()

    print(json.dumps({"what": "build_mips_fwd_bwd", "impl": "hip", "base": 32, "ms": round(timed(mips, args.reps), 4),
                      "clock_ghz": ghz}), flush=True)
    # baseline prefilter: mip by avg_pool2d, diffuse / specular as products with the prebuilt weight matrices
    mats = {}
    for n, r in ((32, 0.08), (16, 0.5), (8, 1.0)):
        M, wsum = R._specular_matrix(n, r, R.ndf_cutoff(r))
        mats[n] = (M.to_dense().float().cuda(), wsum.float().cuda())
    Md = torch.from_numpy(np.concatenate([R._diffuse_rows(32, i, min(6144, i + 512)) for i in range(0, 6144, 512)])).float().cuda()
    base = light.base.detach().clone().requires_grad_(True)

    def mips_torch():
        base.grad = None
        lv = [base]
        while lv[-1].shape[1] > 8:
            lv.append(torch.nn.functional.avg_pool2d(lv[-1].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
        dif = (Md @ base.reshape(-1, 3)).reshape(base.shape)
        spec = [(mats[x.shape[1]][0] @ x.reshape(-1, 3) / mats[x.shape[1]][1][:, None]) for x in lv]
        (dif.sum() + sum(s.sum() for s in spec)).backward()

    print(json.dumps({"what": "build_mips_fwd_bwd", "impl": "torch_fp32", "base": 32, "ms": round(timed(mips_torch, args.reps), 4),
                      "clock_ghz": ghz}), flush=True)

    with torch.no_grad():
        light.build_mips()
    lut = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (1, 256, 256, 2)).astype(np.float32)).cuda()
    for S in (512, 1024):
        rng = np.random.default_rng(S)
        n = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(S, S, 3)).astype(np.float32)).cuda(), dim=-1)
        v = torch.nn.functional.normalize(n + 0.5 * torch.randn_like(n), dim=-1)
        alb = torch.rand(S, S, 3, device="cuda", requires_grad=True)
        rough = torch.rand(S, S, 1, device="cuda", requires_grad=True)
        occ = torch.rand(S, S, 1, device="cuda", requires_grad=True)
        mask = (torch.rand(S, S, 1, device="cuda") > 0.2).float()
        dif = light.diffuse.detach().requires_grad_(True)
        spec = [s.detach().requires_grad_(True) for s in light.specular]
        import types
        lt = types.SimpleNamespace(diffuse=dif, specular=spec)

        def fwd():
            with torch.no_grad():
                pbr_shading(lt, n, v, alb, rough, mask, occlusion=occ, brdf_lut=lut)

        def fwd_bwd():
            r = pbr_shading(lt, n, v, alb, rough, mask, occlusion=occ, brdf_lut=lut)
            sum(x.sum() for x in r.values()).backward()

        args_t = (dif, spec, lut[0], n.reshape(-1, 3), v.reshape(-1, 3), alb.reshape(-1, 3), rough.reshape(-1, 1),
                  occ.reshape(-1, 1), mask.reshape(-1, 1))

        def tfwd():
            with torch.no_grad():
                torch_shade(*args_t)

        def tfwd_bwd():
            sum(x.sum() for x in torch_shade(*args_t)).backward()

        # the backward kernel alone (the light-gradient zero fill included), outside autograd
        import ctypes as C
        from mygauhuman_amd.pbr import _ops
        tt = {"normals": n.reshape(-1, 3), "view_dirs": v.reshape(-1, 3), "mask": mask.reshape(-1), "background": None,
              "lut": lut[0].contiguous(), "albedo": alb.detach().reshape(-1, 3), "roughness": rough.detach().reshape(-1),
              "occlusion": occ.detach().reshape(-1), "metallic": None, "diffuse": dif.detach()}
        sp = [x.detach() for x in spec]
        st = _ops.ShadeFn._struct(tt, sp, False, False)
        gin = torch.ones(S * S, 3, device="cuda")
        gout = [torch.empty(S * S, 3, device="cuda"), torch.empty(S * S, device="cuda"), torch.empty(S * S, device="cuda")]
        dgr = [torch.zeros_like(dif)] + [torch.zeros_like(x) for x in sp]
        st.d_render_rgb = st.d_diffuse_rgb = st.d_specular_rgb = st.d_diffuse_light = gin.data_ptr()
        st.d_albedo, st.d_roughness, st.d_occlusion = (x.data_ptr() for x in gout)
        st.diffuse.grad[0] = dgr[0].data_ptr()
        for i, x in enumerate(dgr[1:]):
            st.specular.grad[i] = x.data_ptr()

        def bwd_kernel():
            for x in dgr:
                x.zero_()
            _lib.check(_lib.lib.gsr_pbr_shade_backward(C.byref(st), torch.cuda.current_stream().cuda_stream), "shade_backward")

        for what, fn, impl in (("shade_bwd_kernel", bwd_kernel, "hip"), ("shade_fwd", fwd, "hip"), ("shade_fwd_bwd", fwd_bwd, "hip"), ("shade_fwd", tfwd, "torch_fp32"),
                               ("shade_fwd_bwd", tfwd_bwd, "torch_fp32")):
            print(json.dumps({"what": what, "impl": impl, "pixels": f"{S}x{S}", "ms": round(timed(fn, args.reps), 4),
                              "clock_ghz": ghz}), flush=True)


if __name__ == "__main__":
    main()
