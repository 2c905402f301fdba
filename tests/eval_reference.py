"""Inputs and host-side restatements for the evaluation view finish (mygauhuman_amd.evaluate, csrc/eval.hip).

    case_inputs(name) / inputs_at(H, W, salt)   seeded images, mask and background rebuilt bit for bit from an index hash
                                                (tests/golden/make_golden_eval.py stores only the reference's outputs)
    finish_np, quantise_np, psnr_np, ssim_np    float64 numpy restatement of render.py:264-311,337-338 and save_image's rounding
    finish_torch, quantise_torch, metrics_torch the reference's torch statements (any device, any float dtype)
    reference_loop(...)                         the loop of render.py:186-350 in those statements over our render() / pbr_shading"""
import zlib

import numpy as np
import torch

from tests.pbr_reference import _u01
from tests.torch_reference import _window_2d, ssim_torch

FILL_NAMES = ("render", "render_alpha", "normal", "world_normal", "albedo", "roughness", "render_depth", "render_pbr",
              "render_diffuse", "render_specular", "render_ao")
NAMES = ("render", "render_alpha", "albedo", "gt", "gt_normal")   # the images of a fixture case, in slot order
CHANNELS = {"render": 3, "render_alpha": 1, "albedo": 3, "gt": 3, "gt_normal": 3}

# name: (H, W, mask kind, background, variant)
CASES = {
    "rect_black_70x90": (70, 90, "rect", (0.0, 0.0, 0.0), None),
    "rect_white_70x90": (70, 90, "rect", (1.0, 1.0, 1.0), None),
    "rect_black_256": (256, 256, "rect", (0.0, 0.0, 0.0), None),
    "ones_white_256": (256, 256, "ones", (1.0, 1.0, 1.0), None),
    "zeros_black_70x90_inf": (70, 90, "zeros", (0.0, 0.0, 0.0), "gt0_zero"),      # channel 0: mse == 0 -> psnr = +inf
    "strip_white_1x200": (1, 200, "rect", (1.0, 1.0, 1.0), None),
    "inside_equal_256": (256, 256, "rect", (0.0, 0.0, 0.0), "inside_equal"),      # render == gt inside: a tiny mse
}


def _mask(kind, H, W):
    if kind == "ones":
        return np.ones((H, W), np.float32)
    m = np.zeros((H, W), np.float32)
    if kind == "rect":
        m[H // 5:max(H // 5 + 1, (4 * H) // 5), W // 7:(6 * W) // 7] = 1.0
    return m


def inputs_at(H, W, salt, variant=None, kind="rect", background=(0.0, 0.0, 0.0)):
    """dict(images: name -> float32 [C, H, W] drawn from [-0.2, 1.2] (both clamp sides act), with exact 0, 1 and (k + 0.5) / 255
    boundary values planted; mask float32 [H, W] of 0 / 1; background float32 [3])."""
    images = {}
    for i, n in enumerate(NAMES):
        images[n] = (_u01((CHANNELS[n], H, W), salt + i) * 1.4 - 0.2).astype(np.float32)
    mask = _mask(kind, H, W)
    # gt is the rendering plus noise where both are inside [0, 1]: a psnr in the range a run reports
    images["gt"] = (np.clip(images["render"], 0.0, 1.0) + 0.1 * (_u01((3, H, W), salt + 50) - 0.5)).astype(np.float32)
    planted = [0.0, 1.0, -0.0, 0.5 / 255, 1.5 / 255, 127.5 / 255, 254.5 / 255, 253.5 / 255, 0.49999 / 255, 0.50001 / 255, 1.0 + 1e-7,
               -1e-9, 100.5 / 255, 200.5 / 255]
    flat = images["render"].reshape(-1)
    for k, val in enumerate(planted):
        flat[(k * 37 + 5) % flat.size] = np.float32(val)
    if variant == "gt0_zero":
        images["gt"][0] = 0.0
    elif variant == "inside_equal":
        inside = mask > 0
        images["gt"][:, inside] = np.clip(images["render"][:, inside], 0.0, 1.0)
        images["gt"][1][~inside] = (1e-3 * _u01((H, W), salt + 60)).astype(np.float32)[~inside]
    return dict(images=images, mask=mask, background=np.asarray(background, np.float32))


def case_inputs(name):
    H, W, kind, bg, variant = CASES[name]
    return inputs_at(H, W, 1000 * (1 + list(CASES).index(name)), variant, kind, bg)


# ---- float64 numpy restatement ----------------------------------------------------------------------------------------------------
def flip_normal_np(n):
    """render.py:191-193 in the array's dtype."""
    n = n * n.dtype.type(2) - n.dtype.type(1)
    n[2] = -n[2]
    return (n + n.dtype.type(1)) / n.dtype.type(2)


def finish_np(images, mask, background):
    """Fill (render.py:264-270, the names of FILL_NAMES) then clamp (:303-311): exact operations, float32 in and out."""
    fill = np.float32(0.0 if float(np.sum(background)) == 0 else 1.0)
    out = {}
    for n, a in images.items():
        a = a.copy()
        if n in FILL_NAMES:
            a[:, mask == 0] = fill
        out[n] = np.clip(a, np.float32(0), np.float32(1))
    return out


def quantise_np(img):
    """torchvision.utils.save_image: img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8), in float32."""
    q = img.astype(np.float32) * np.float32(255) + np.float32(0.5)
    return np.ascontiguousarray(np.clip(q, 0, 255).astype(np.uint8).transpose(1, 2, 0))


def psnr_np(a, b):
    """utils/image_utils.py:19-21 followed by .mean(), float64."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    mse = ((a - b) ** 2).reshape(a.shape[0], -1).mean(1)
    with np.errstate(divide="ignore"):
        return float(np.mean(20.0 * np.log10(1.0 / np.sqrt(mse))))


def window_2d():
    """utils/loss_utils.py:26-33: float32 taps normalised by their float32 sum (torch's summation order, hence torch here), outer
    product in float32."""
    return _window_2d(11).numpy().astype(np.float32)


def _blur(x, w2):
    C, H, W = x.shape
    p = np.zeros((C, H + 10, W + 10), np.float64)
    p[:, 5:5 + H, 5:5 + W] = x
    out = np.zeros((C, H, W), np.float64)
    for i in range(11):
        for j in range(11):
            out += w2[i, j] * p[:, i:i + H, j:j + W]
    return out


def ssim_np(a, b):
    """utils/loss_utils.py:36-66 (.mean()), float64, zero padding."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    w2 = window_2d().astype(np.float64)
    m1, m2 = _blur(a, w2), _blur(b, w2)
    s1, s2, s12 = _blur(a * a, w2) - m1 * m1, _blur(b * b, w2) - m2 * m2, _blur(a * b, w2) - m1 * m2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return float((((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2))).mean())


def crc_of(u8s):
    c = 0
    for a in u8s:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


# ---- the reference's torch statements ---------------------------------------------------------------------------------------------
def flip_normal_torch(gt_normal):
    gt_normal = (gt_normal * 2) - 1.
    gt_normal[2, ...] = -gt_normal[2, ...]
    return (gt_normal + 1) / 2.


def finish_torch(images, bound_mask, background):
    """render.py:264-270 then :303-311 as written there; images: name -> [C, H, W] (mutated, like there); bound_mask [1, H, W]."""
    out = {}
    for n, img in images.items():
        if n in FILL_NAMES:
            img.permute(1, 2, 0)[bound_mask[0] == 0] = 0 if background.sum().item() == 0 else 1
        out[n] = torch.clamp(img, 0.0, 1.0)
    return out


def quantise_torch(img):
    return img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def psnr_torch(img1, img2):
    mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def metrics_torch(img, gt, ssim=ssim_torch, psnr=psnr_torch):
    """render.py:337-338 / :341-342: (psnr(...).mean().double(), ssim(...).mean().double()) as Python floats."""
    return float(psnr(img, gt).mean().double()), float(ssim(img, gt).mean().double())


def reference_loop(render, pbr_shading, views, gaussians, pipe, background, iteration, cubemap=None, brdf_lut=None, view_dirs=None):
    """render.py:186-350 over our render() / pbr_shading with the reference's statements for everything after them.  Returns the
    per-view finished images (name -> [C, H, W]) and (psnr, ssim) in float32 as render.py computes them."""
    per_view, metrics = [], []
    with torch.no_grad():
        for view in views:
            gt = view.original_image[0:3, :, :].cuda().clone()
            gt_normal = view.original_normal[0:3, :, :].cuda().clone()
            out = render(iteration, view, gaussians, pipe, background)
            images = {"render": out["render"], "normal": out["normal"], "world_normal": out["world_normal"], "albedo": out["albedo"],
                      "roughness": out["roughness"], "render_depth": out["render_depth"], "render_alpha": out["render_alpha"]}
            if iteration > 3000:
                occ = out["occlusion"]
                r = pbr_shading(light=cubemap, normals=out["world_normal"].permute(1, 2, 0).detach(), view_dirs=view_dirs,
                                mask=out["render_alpha"].permute(1, 2, 0), albedo=out["albedo"].permute(1, 2, 0),
                                roughness=out["roughness"][0, ...].unsqueeze(0).permute(1, 2, 0), metallic=None, tone=False, gamma=False,
                                occlusion=occ.permute(1, 2, 0)[..., 0][..., None], brdf_lut=brdf_lut)
                images["render_pbr"] = r["render_rgb"].clamp(min=0.0, max=1.0).permute(2, 0, 1)
                images["render_diffuse"] = r["diffuse_rgb"].clamp(min=0.0, max=1.0).permute(2, 0, 1)
                images["render_specular"] = r["specular_rgb"].clamp(min=0.0, max=1.0).permute(2, 0, 1)
                images["render_ao"] = occ.clamp(min=0.0, max=1.0)
            images["gt"], images["gt_normal"] = gt, gt_normal
            fin = finish_torch(images, view.bound_mask, background)
            metrics.append(metrics_torch(fin["render_pbr" if iteration > 3000 else "render"], fin["gt"]))
            per_view.append(fin)
    return per_view, metrics
