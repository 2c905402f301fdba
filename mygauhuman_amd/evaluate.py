"""Evaluation of a trained model without a host read per view (render.py:186-350; the same block in training_report, train.py:480-540).

    EvalMetrics(n_views, device)   the (psnr, ssim) table, its row counter and the overflow word, all on the device; .result()
                                   synchronises once
    finish_view(images, bound_mask, background, ...)
                                   everything the reference does to a view's images after render() / pbr_shading return -- the fill
                                   under the bound mask (render.py:250-253, :264-270), the clamps (:303-311, :327-330), save_image's
                                   8-bit quantisation, psnr and ssim of the finished pair (:336-343) -- in three launches
                                   (csrc/eval.hip) that read nothing back: it records into graph.GraphedFrame
    psnr(img1, img2)               utils/image_utils.py:19-21 (a plain tensor expression, identical to the reference)
    save_png(path, u8)             the PNG torchvision.utils.save_image writes, from a finished uint8 [H, W, C] buffer
    render_set(views, gaussians, pipe, background, iteration, ...)
                                   the loop of render.py:186-350 over the above
No CPU path and no torch fallback: a missing library or a CPU tensor raises."""
import copy
import ctypes as C
import math
import os
import time

import torch

from ._lib import EVAL_FILL, EVAL_FLIP_Z, EVAL_MAX_SLOTS, MASK_F32, MASK_U8, EvalView, call, lib

# the eleven images render.py fills under the bound mask (:250-253, :264-270); the ground truths are not filled
FILL_NAMES = ("render", "render_alpha", "normal", "world_normal", "albedo", "roughness", "render_depth", "render_pbr",
              "render_diffuse", "render_specular", "render_ao")
PBR_ITERATION = 3000  # render.py:211,322,336: the PBR branch of the evaluation loop


class EvalMetrics:
    """table [n_views, 2] float64 (psnr, ssim), the row counter and the sticky overflow word, on `device`.  Every finish_view(...,
    metrics=self) fills the row the counter names and advances it ON THE DEVICE, so one captured graph fills one row per replay."""

    def __init__(self, n_views, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("EvalMetrics: the table lives on a HIP device (no CPU path)")
        if int(n_views) < 1:
            raise ValueError("EvalMetrics: n_views must be positive")
        self.n_views = int(n_views)
        self.table = torch.zeros((self.n_views, 2), device=device, dtype=torch.float64)
        self.state = torch.zeros(2, device=device, dtype=torch.int32)  # [counter, overflow]

    @property
    def device(self):
        return self.table.device

    def reset(self):
        self.table.zero_()
        self.state.zero_()

    def result(self):
        """ONE device-to-host copy.  {"psnr", "ssim": numpy float64 arrays of the rows filled so far, "psnr_mean", "ssim_mean": Python
        floats (the reference's psnrs /= len(views))}; raises if more views were finished than the table has rows."""
        host = torch.cat([self.table.reshape(-1), self.state.to(torch.float64)]).cpu().numpy()
        n, overflow = int(host[-2]), int(host[-1])
        if overflow or n > self.n_views:
            raise RuntimeError(f"EvalMetrics: {n} views were finished into a table of {self.n_views} rows; the extra ones were dropped")
        rows = host[:-2].reshape(self.n_views, 2)[:n]
        ps, ss = rows[:, 0].copy(), rows[:, 1].copy()
        return {"psnr": ps, "ssim": ss, "psnr_mean": float(ps.sum() / n) if n else float("nan"),
                "ssim_mean": float(ss.sum() / n) if n else float("nan")}


def _check_image(name, t, what="image"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"finish_view: {what} {name!r} must live on a HIP device (no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 3:
        raise ValueError(f"finish_view: {what} {name!r} must be a float32 [C, H, W] tensor (or a permuted [H, W, C] view), got "
                         f"{t.dtype} {tuple(t.shape)}")
    if t.shape[0] not in (1, 3):
        raise ValueError(f"finish_view: {what} {name!r} has {t.shape[0]} channels; 1 or 3 are supported")
    order = sorted(range(3), key=lambda d: -t.stride(d))
    if t.numel() == 0 or not t.permute(order).is_contiguous():
        raise ValueError(f"finish_view: {what} {name!r} is not a dense permutation of a contiguous tensor (strides {t.stride()}); it is "
                         "finished in place, so no copy is made for you: pass a dense tensor")


def _mask_of(bound_mask, H, W, dev):
    if not isinstance(bound_mask, torch.Tensor) or not bound_mask.is_cuda:
        raise RuntimeError("finish_view: bound_mask must live on a HIP device (no CPU path)")
    m = bound_mask.detach()
    if m.dim() == 3 and m.shape[0] == 1:
        m = m[0]
    if tuple(m.shape) != (H, W) or m.device != dev:
        raise ValueError(f"finish_view: bound_mask must be [H, W] or [1, H, W] = {(H, W)} on {dev}, got {tuple(bound_mask.shape)} on {m.device}")
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype not in (torch.float32, torch.uint8):
        m = (m != 0).view(torch.uint8)
    return m.contiguous()


def finish_view(images, bound_mask, background, metrics=None, metric=("render", "gt"), to_uint8=(), flip_gt_normal=False, out=None):
    """Finish one view's images as render.py does after render() / pbr_shading return.

    images       dict name -> float32 GPU tensor [C, H, W], C = 1 or 3; a permuted view of an [H, W, C] tensor (pbr_shading's
                 results) is read in place.  Names in FILL_NAMES get the fill value (0 for a black background, else 1, decided on the
                 device from `background`) where bound_mask == 0; every image is clamped to [0, 1].  THE TENSORS ARE FINISHED IN
                 PLACE (the reference mutates render()'s outputs too) unless `out` names another destination.
    bound_mask   [H, W] or [1, H, W]: float32, uint8 or bool (other dtypes are compared with 0 first)
    background   float32 [3] on the device
    metrics      an EvalMetrics: psnr / ssim of the finished pair `metric` = (image name, ground-truth name) go into its next row
    to_uint8     names (or a dict name -> uint8 [H, W, C] buffer to reuse): save_image's 8-bit image of the finished values
    flip_gt_normal  the 'zju' branch of render.py:190-193 on images["gt_normal"]
    out          dict name -> tensor with the image's shape and strides: the finished floats go there and the input is left alone

    Returns (finished, u8): dicts name -> tensor.  At most 16 images per call.  Nothing reads the device: the call records under
    torch.cuda.graph.  No CPU path."""
    if not isinstance(images, dict) or not images:
        raise ValueError("finish_view: images must be a non-empty dict name -> tensor")
    if len(images) > EVAL_MAX_SLOTS:
        raise ValueError(f"finish_view: at most {EVAL_MAX_SLOTS} images per call, got {len(images)}")
    names = list(images)
    if metrics is not None and (len(metric) != 2 or metric[0] not in images or metric[1] not in images or metric[0] == metric[1]):
        raise ValueError(f"finish_view: metric = {tuple(metric)!r} must name two different images of {names}")
    for n in names:
        _check_image(n, images[n])
    first = images[names[0]]
    dev, (H, W) = first.device, first.shape[1:]
    for n in names:
        if images[n].shape[1:] != first.shape[1:] or images[n].device != dev:
            raise ValueError(f"finish_view: image {n!r} is {tuple(images[n].shape)} on {images[n].device}; every image must be "
                             f"[C, {H}, {W}] on {dev}")
    out = dict(out) if out else {}
    for n, o in out.items():
        if n not in images:
            raise ValueError(f"finish_view: out names an unknown image {n!r}")
        _check_image(n, o, "destination")
        if o.shape != images[n].shape or o.stride() != images[n].stride() or o.device != dev:
            raise ValueError(f"finish_view: destination {n!r} must have the image's shape and strides "
                             f"({tuple(images[n].shape)}, {images[n].stride()}), e.g. torch.empty_like(image)")
    if metrics is not None:
        if not isinstance(metrics, EvalMetrics) or metrics.device != dev:
            raise ValueError("finish_view: metrics must be an EvalMetrics on the images' device")
        for n in metric:
            if images[n].shape[0] != 3:
                raise ValueError(f"finish_view: metric image {n!r} must have 3 channels")
    if flip_gt_normal and ("gt_normal" not in images or images["gt_normal"].shape[0] != 3):
        raise ValueError("finish_view: flip_gt_normal needs a 3-channel image named 'gt_normal'")
    u8 = {}
    for n in (to_uint8 if isinstance(to_uint8, dict) else list(to_uint8)):
        if n not in images:
            raise ValueError(f"finish_view: to_uint8 names an unknown image {n!r}")
        shape = (H, W, images[n].shape[0])
        buf = to_uint8[n] if isinstance(to_uint8, dict) else None
        if buf is None:
            buf = torch.empty(shape, device=dev, dtype=torch.uint8)
        elif not isinstance(buf, torch.Tensor) or buf.device != dev or buf.dtype != torch.uint8 or tuple(buf.shape) != shape or \
                not buf.is_contiguous():
            raise ValueError(f"finish_view: the uint8 buffer of {n!r} must be a contiguous uint8 {shape} tensor on {dev}")
        u8[n] = buf
    if not isinstance(background, torch.Tensor) or not background.is_cuda:
        raise RuntimeError("finish_view: background must live on a HIP device (no CPU path): it is read there, not with .item()")
    if background.device != dev or background.dtype != torch.float32 or background.numel() != 3 or not background.is_contiguous():
        raise ValueError("finish_view: background must be a contiguous float32 [3] tensor on the images' device")
    mask = _mask_of(bound_mask, H, W, dev)

    v = EvalView()
    v.slots, v.height, v.width = len(names), H, W
    for k, n in enumerate(names):
        t, s = images[n].detach(), v.slot[k]
        s.src = t.data_ptr()
        s.dst = out[n].data_ptr() if n in out else None
        s.u8 = u8[n].data_ptr() if n in u8 else None
        s.stride[:] = list(t.stride())
        s.channels = t.shape[0]
        s.flags = (EVAL_FILL if n in FILL_NAMES else 0) | (EVAL_FLIP_Z if flip_gt_normal and n == "gt_normal" else 0)
    v.mask, v.mask_dtype = mask.data_ptr(), MASK_F32 if mask.dtype == torch.float32 else MASK_U8
    v.background = background.data_ptr()
    ws = None
    if metrics is not None:
        v.metric_image, v.metric_gt = names.index(metric[0]), names.index(metric[1])
        v.counter, v.overflow = metrics.state.data_ptr(), metrics.state.data_ptr() + 4
        v.table, v.capacity = metrics.table.data_ptr(), metrics.n_views
        ws = torch.empty(int(lib.gsr_eval_workspace_floats(H, W)), device=dev, dtype=torch.float32)
    else:
        v.metric_image = v.metric_gt = -1
    call("gsr_eval_view_finish", dev, C.byref(v), ws.data_ptr() if ws is not None else None)
    return {n: out.get(n, images[n]) for n in names}, u8


def psnr(img1, img2):
    """utils/image_utils.py:19-21: [B, ...] -> [B, 1] (for a [3, H, W] image: one value per channel; render.py takes .mean())."""
    mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def save_png(path, u8):
    """Write a finished uint8 [H, W, C] buffer (finish_view's to_uint8) as the PNG torchvision.utils.save_image gives: a 1-channel
    image becomes RGB with the channel repeated (make_grid does that)."""
    from PIL import Image
    a = u8.detach().cpu().numpy() if isinstance(u8, torch.Tensor) else u8
    if a.ndim != 3 or a.shape[2] not in (1, 3) or a.dtype.name != "uint8":
        raise ValueError(f"save_png: expected a uint8 [H, W, 1 or 3] image, got {a.dtype} {a.shape}")
    if a.shape[2] == 1:
        a = a.repeat(3, axis=2)
    Image.fromarray(a, "RGB").save(path, format="PNG")


# ---- the evaluation loop ---------------------------------------------------------------------------------------------------------
# output name -> render()'s key, in the order render.py saves them
_RENDER_KEYS = (("render", "render"), ("normal", "normal"), ("world_normal", "world_normal"), ("albedo", "albedo"),
                ("roughness", "roughness"), ("render_depth", "render_depth"), ("render_alpha", "render_alpha"))
_PBR_NAMES = ("render_pbr", "render_diffuse", "render_specular", "render_ao")


def view_dirs_of(ref_view, canonical_rays, H, W):
    """render.py:214-222: the view directions of the reference view for pbr_shading, [H, W, 3]."""
    c2w = torch.inverse(ref_view.world_view_transform.T)
    rays = torch.nn.functional.normalize(canonical_rays[:, None, :], p=2, dim=-1)
    return -((rays * c2w[None, :3, :3]).sum(dim=-1).reshape(H, W, 3))


def _frame(iteration, view, gaussians, pipe, background, smpl, light, brdf_lut, view_dirs, gt, gt_normal, metrics, want_u8, flip,
           envmap):
    """One evaluation frame: render -> shade -> finish -> metrics.  Returns (finished, u8)."""
    from .gaussian_renderer import render
    kw = {} if smpl is None else {"transforms": smpl["transforms"], "translation": smpl["translation"]}
    res = render(iteration, view, gaussians, pipe, background, envmap=envmap, **kw)
    images = {n: res[k] for n, k in _RENDER_KEYS}
    pair = ("render", "gt")
    if iteration > PBR_ITERATION:
        from .pbr import pbr_shading
        occ = res["occlusion"]
        shaded = pbr_shading(light=light, normals=res["world_normal"].permute(1, 2, 0).detach(), view_dirs=view_dirs,
                             mask=res["render_alpha"].permute(1, 2, 0), albedo=res["albedo"].permute(1, 2, 0),
                             roughness=res["roughness"][0, ...].unsqueeze(0).permute(1, 2, 0), metallic=None, tone=False, gamma=False,
                             occlusion=occ.permute(1, 2, 0)[..., 0][..., None], brdf_lut=brdf_lut)
        # (:240-243 clamp before the fill and :327-329 after it: with a fill value of 0 or 1 the second clamp alone gives the same)
        images["render_pbr"] = shaded["render_rgb"].permute(2, 0, 1)
        images["render_diffuse"] = shaded["diffuse_rgb"].permute(2, 0, 1)
        images["render_specular"] = shaded["specular_rgb"].permute(2, 0, 1)
        images["render_ao"] = occ
        pair = ("render_pbr", "gt")
    images["gt"], images["gt_normal"] = gt, gt_normal
    # the ground truths belong to the dataset: finished into buffers of their own (torch.clamp is out of place there too)
    out = {"gt": torch.empty_like(gt), "gt_normal": torch.empty_like(gt_normal)}
    return finish_view(images, view.bound_mask, background, metrics=metrics, metric=pair,
                       to_uint8=list(images) if want_u8 else (), flip_gt_normal=flip, out=out)


def _static_view(view, dev):
    """A copy of `view` whose tensors (and dicts of tensors) are private device tensors: the static inputs of a captured frame."""
    s = copy.copy(view)
    for k, a in vars(view).items():
        if isinstance(a, torch.Tensor):
            setattr(s, k, a.detach().to(dev, copy=True))
        elif isinstance(a, dict):
            setattr(s, k, {q: (b.detach().to(dev, copy=True) if isinstance(b, torch.Tensor) else b) for q, b in a.items()})
    return s


def _static_update(s, view):
    for k, a in vars(view).items():
        if isinstance(a, torch.Tensor):
            getattr(s, k).copy_(a, non_blocking=True)
        elif isinstance(a, dict):
            for q, b in a.items():
                if isinstance(b, torch.Tensor):
                    getattr(s, k)[q].copy_(b, non_blocking=True)


def render_set(views, gaussians, pipe, background, iteration, cubemap=None, brdf_lut=None, canonical_rays=None, smpl_rot=None,
               out_dir=None, lpips_fn=None, graphed=False, flip_gt_normal=False, envmap=None, return_images=False):
    """The loop of render.py:186-350 under torch.no_grad(): per view render() (with the cached transforms / translation of
    smpl_rot[view.pose_id] when smpl_rot is given), pbr_shading and the PBR metric pair when iteration > 3000 (render.py's own
    threshold), finish_view, and the metrics into one device table.  Nothing inside the loop reads the device; it ends in one
    synchronise.  Afterwards: PNGs of the thirteen (nine below the threshold) images per view under out_dir/<name>/00000.png from
    the uint8 buffers, and lpips_fn(finished image, finished gt) per view if given.

    views: objects with the fields render() reads plus original_image, original_normal ([>=3, H, W]), bound_mask and, with
    smpl_rot, pose_id.  cubemap (a pbr.CubemapLight with its mips built), brdf_lut and canonical_rays ([H*W, 3]) are needed above
    the threshold.  flip_gt_normal: the 'zju' branch of :190-193.  return_images: also return "images", per view a dict name ->
    finished float tensor (render.py's thirteen lists), kept on the device.
    graphed=True records one frame per distinct (H, W, FoVx, FoVy) into a graph.GraphedFrame (forward only; the per-view inputs are
    copied in place into static tensors) and replays it per view.
    Returns {"psnr", "ssim", "lpips" (None without lpips_fn), "fps": len(views) / seconds of the loop, "per_view": {"psnr", "ssim"}}."""
    views = list(views)
    if not views:
        raise ValueError("render_set: no views")
    dev = background.device
    pbr = iteration > PBR_ITERATION
    if pbr and (cubemap is None or brdf_lut is None or canonical_rays is None):
        raise ValueError(f"render_set: iteration > {PBR_ITERATION} needs cubemap, brdf_lut and canonical_rays")
    want_u8 = out_dir is not None
    with torch.no_grad():
        metrics = EvalMetrics(len(views), dev)
        H0, W0 = int(views[0].image_height), int(views[0].image_width)
        view_dirs = view_dirs_of(views[0], canonical_rays, H0, W0) if pbr else None
        lut = brdf_lut.to(dev) if pbr else None
        smpl_of = (lambda v: smpl_rot[v.pose_id]) if smpl_rot is not None else (lambda v: None)
        gts = [(v.original_image[0:3, :, :].to(dev), v.original_normal[0:3, :, :].to(dev)) for v in views]
        frames, kept, images_out = {}, [], []

        def run(view, smpl, gt, gt_normal):
            return _frame(iteration, view, gaussians, pipe, background, smpl, cubemap, lut, view_dirs, gt, gt_normal, metrics,
                          want_u8, flip_gt_normal, envmap)

        if graphed:
            from .graph import GraphedFrame
            for v, (gt, gtn) in zip(views, gts):
                key = (int(v.image_height), int(v.image_width), float(v.FoVx), float(v.FoVy))
                if key not in frames:
                    sv = _static_view(v, dev)
                    sm = smpl_of(v)
                    sm = None if sm is None else {k: sm[k].detach().to(dev, copy=True) for k in ("transforms", "translation")}
                    sgt, sgtn = gt.contiguous().clone(), gtn.contiguous().clone()
                    frames[key] = (GraphedFrame(lambda sv=sv, sm=sm, sgt=sgt, sgtn=sgtn: run(sv, sm, sgt, sgtn)), sv, sm, sgt, sgtn)
            metrics.reset()  # the warm-up and self-check runs of the captures advanced the counter
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for v, (gt, gtn) in zip(views, gts):
            if graphed:
                frame, sv, sm, sgt, sgtn = frames[(int(v.image_height), int(v.image_width), float(v.FoVx), float(v.FoVy))]
                _static_update(sv, v)
                if sm is not None:
                    for k in sm:
                        sm[k].copy_(smpl_of(v)[k], non_blocking=True)
                sgt.copy_(gt, non_blocking=True)
                sgtn.copy_(gtn, non_blocking=True)
                finished, u8 = frame.replay()
                if want_u8:
                    u8 = {k: b.clone() for k, b in u8.items()}  # the graph's buffers are rewritten by the next replay
            else:
                finished, u8 = run(v, smpl_of(v), gt, gtn)
            pair = None
            if lpips_fn is not None:
                pair = (finished["render_pbr" if pbr else "render"], finished["gt"])
                pair = tuple(t.clone() for t in pair) if graphed else pair
            if return_images:
                images_out.append({k: t.clone() for k, t in finished.items()} if graphed else finished)
            kept.append((u8, pair))
        torch.cuda.synchronize(dev)
        seconds = time.perf_counter() - t0
        for f in frames.values():
            f[0].check()
        r = metrics.result()
        lp = None
        if lpips_fn is not None:
            lp = float(sum(lpips_fn(a, b).mean().double() for _, (a, b) in kept) / len(views))
        if want_u8:
            for i, (u8, _) in enumerate(kept):
                for name, buf in u8.items():
                    d = os.path.join(out_dir, name)
                    os.makedirs(d, exist_ok=True)
                    save_png(os.path.join(d, "{0:05d}.png".format(i)), buf)
    res = {"psnr": r["psnr_mean"], "ssim": r["ssim_mean"], "lpips": lp, "fps": len(views) / seconds if seconds > 0 else math.inf,
           "per_view": {"psnr": r["psnr"], "ssim": r["ssim"]}}
    if return_images:
        res["images"] = images_out
    return res
