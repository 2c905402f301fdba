"""Image losses of the reference training loop (utils/loss_utils.py:20-66, used at train.py:261-287).

    l1_loss, l2_loss       plain tensor expressions (identical to the reference)
    ssim(img1, img2)       fused HIP forward + backward (csrc/ssim.hip) behind the reference's signature; gradient flows to
                           img1 (the rendering), img2 is treated as ground truth
                           (the grouped-conv2d formulation it replaces is kept with the tests: tests/torch_reference.py)
    bounding_rect(mask)    cv2.boundingRect of the bound mask (train.py:269, :318) into an int32 [4] DEVICE tensor (x, y, w, h)
    ssim_crop(img1, img2, rect)   ssim(img1[:, y:y+h, x:x+w][None], img2[:, y:y+h, x:x+w][None]) with the rectangle read on the
                           device (csrc/ssim_crop.hip): no host read, no shape that depends on the rectangle, so a training step
                           with the reference's SSIM term records into graph.GraphedFrame and one graph serves every camera
"""
import ctypes as C

import torch

from ._lib import MASK_F32, MASK_U8, SSIM_CROP_MAX_GROUPS, SsimCrop, call, lib, ptr


def l1_loss(network_output, gt):
    return torch.abs((network_output - gt)).mean()


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()


class _SsimMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        dev = img1.device
        a, b = img1.detach().contiguous().float(), img2.detach().contiguous().float()
        H, W = a.shape[-2], a.shape[-1]
        planes = a.numel() // (H * W) if H * W else 0
        out = torch.empty_like(a)
        need = ctx.needs_input_grad[0]
        dA, dB, dC = (torch.empty_like(a) for _ in range(3)) if need else (None, None, None)
        call("gsr_ssim_forward", dev, planes, H, W, ptr(a), ptr(b), ptr(out), ptr(dA), ptr(dB), ptr(dC))
        if need:
            ctx.save_for_backward(a, b, dA, dB, dC)
        ctx.dims = (planes, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, dA, dB, dC = ctx.saved_tensors
        planes, H, W = ctx.dims
        g = g.contiguous().float()
        out = torch.empty_like(a)
        call("gsr_ssim_backward", a.device, planes, H, W, ptr(a), ptr(b), ptr(g), 0.0, ptr(dA), ptr(dB), ptr(dC), ptr(out))
        return out, None


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss_utils.py:36-66.  img1, img2: [..., C, H, W] on the GPU; the kernel is built for the reference's 11 x 11
    window (its only call sites, train.py:264,287).  No CPU / torch fallback."""
    if not img1.is_cuda:
        raise RuntimeError("ssim: tensors must live on a HIP device (no CPU path)")
    if window_size != 11:
        raise RuntimeError("ssim: only the reference's window_size = 11 is built")
    ssim_map = _SsimMap.apply(img1, img2)
    if size_average:
        return ssim_map.mean()
    return ssim_map.mean(1).mean(1).mean(1)


def bounding_rect(mask, out=None):
    """cv2.boundingRect(mask) on the device: mask [H, W] or [1, H, W] (float32, uint8 or bool; nonzero = inside; other dtypes are
    compared with 0 first) -> int32 [4] = (x, y, w, h) on the mask's device, (0, 0, 0, 0) for an all-zero mask.  `out` reuses a
    buffer (int32 [4], contiguous, same device): what a captured graph needs.  Nothing is read to the host."""
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise RuntimeError("bounding_rect: tensors must live on a HIP device (no CPU path)")
    if mask.dim() == 3 and mask.shape[0] == 1:
        mask = mask[0]
    if mask.dim() != 2 or mask.numel() == 0:
        raise ValueError(f"bounding_rect: mask must be [H, W] or [1, H, W], got {tuple(mask.shape)}")
    m = mask.detach()
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype not in (torch.float32, torch.uint8):
        m = m != 0
        m = m.view(torch.uint8)
    m = m.contiguous()
    dev = m.device
    if out is None:
        out = torch.empty(4, device=dev, dtype=torch.int32)
    elif not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.int32 or out.numel() != 4 or \
            not out.is_contiguous():
        raise ValueError("bounding_rect: out must be a contiguous int32 [4] tensor on the mask's device")
    ws = torch.empty(int(lib.gsr_bounding_rect_workspace_ints()), device=dev, dtype=torch.int32)
    H, W = m.shape
    call("gsr_bounding_rect", dev, H, W, m.data_ptr(), MASK_F32 if m.dtype == torch.float32 else MASK_U8, out.data_ptr(),
         ws.data_ptr())
    return out


def _dense_view(t):
    """img1 as the kernels read it: float32 at its own (plane, row, pixel) strides when it is a dense permutation of a contiguous
    tensor (train.py's render_rgb.permute(2, 0, 1) is read in place), a contiguous float32 copy otherwise."""
    t = t.detach()
    order = sorted(range(t.dim()), key=lambda d: -t.stride(d))
    if t.dtype != torch.float32 or not t.permute(order).is_contiguous():
        t = t.contiguous().float()
    return t


class _SsimCrop(torch.autograd.Function):
    """(value_0, ..) of n groups: apply(rect, n, img1_0, .., img1_{n-1}, img2_0, .., img2_{n-1}), every image [planes, H, W]."""
    @staticmethod
    def forward(ctx, rect, n, *imgs):
        a = [_dense_view(t) for t in imgs[:n]]
        b = [t.detach().contiguous().float() for t in imgs[n:]]
        dev = a[0].device
        H, W = a[0].shape[-2:]
        need = [bool(f) for f in ctx.needs_input_grad[2:2 + n]]
        maps = [tuple(torch.empty(t.shape, device=dev, dtype=torch.float32) for _ in range(3)) if f else None
                for t, f in zip(a, need)]
        values = [torch.empty((), device=dev, dtype=torch.float32) for _ in range(n)]
        ws = torch.empty(int(lib.gsr_ssim_crop_workspace_floats(sum(t.shape[0] for t in a), H, W)), device=dev, dtype=torch.float32)
        s = _crop_struct(rect, a, b, maps)
        for g in range(n):
            s.value[g] = values[g].data_ptr()
        call("gsr_ssim_crop_forward", dev, C.byref(s), ws.data_ptr())
        ctx.n, ctx.need = n, need
        ctx.save_for_backward(rect, *a, *b, *[m for t in maps if t is not None for m in t])
        return tuple(values)

    @staticmethod
    def backward(ctx, *grads):
        n, need = ctx.n, ctx.need
        rect, *saved = ctx.saved_tensors
        a, b = saved[:n], saved[n:2 * n]
        it = iter(saved[2 * n:])
        maps = [(next(it), next(it), next(it)) if f else None for f in need]
        dev = rect.device
        outs = [torch.empty(t.shape, device=dev, dtype=torch.float32) if f else None for t, f in zip(a, need)]
        if any(need):
            s = _crop_struct(rect, a, b, maps)
            ups = [g.detach().contiguous().float() for g in grads]  # (kept alive until the launch is queued)
            for g in range(n):
                s.upstream[g] = ups[g].data_ptr()
                s.d_img1[g] = ptr(outs[g])
            call("gsr_ssim_crop_backward", dev, C.byref(s))
        return (None, None, *outs, *([None] * n))


def _crop_struct(rect, a, b, maps):
    s = SsimCrop()
    s.groups, s.height, s.width = len(a), a[0].shape[-2], a[0].shape[-1]
    s.rect = rect.data_ptr()
    for g, (x, y, m) in enumerate(zip(a, b, maps)):
        s.planes[g] = x.shape[0]
        s.img1[g], s.img2[g] = x.data_ptr(), y.data_ptr()
        s.img1_stride[g][:] = list(x.stride())
        if m is not None:
            s.dA[g], s.dB[g], s.dC[g] = (t.data_ptr() for t in m)
    return s


def ssim_crop(img1, img2, rect, window_size=11):
    """ssim(img1[:, y:y+h, x:x+w][None], img2[:, y:y+h, x:x+w][None]) of train.py:270-281 and :319-321 with (x, y, w, h) = rect, an
    int32 [4] DEVICE tensor (bounding_rect()): a 0-dim tensor whose gradient reaches img1 only, as in ssim().  img1, img2: [C, H, W]
    on the GPU, or tuples of up to four such pairs that share H and W -- (image, normal), (gt_image, gt_normal) -- which are served
    by one launch each way and give a tuple of values.  img1 may be a permuted view of an [H, W, C] tensor (read in place).
    Nothing in a call reads the device and no tensor's shape depends on the rectangle.  One divergence from the reference: an
    empty rectangle (w == 0 or h == 0, an all-zero mask) gives the value 0 and a zero gradient; the reference raises there (conv2d
    refuses an empty crop), which cannot be done without reading the device.  No CPU / torch fallback."""
    single = isinstance(img1, torch.Tensor)
    a, b = ((img1,), (img2,)) if single else (tuple(img1), tuple(img2))
    if isinstance(img2, torch.Tensor) != single or len(a) != len(b) or not 1 <= len(a) <= SSIM_CROP_MAX_GROUPS:
        raise ValueError(f"ssim_crop: img1 and img2 must be two tensors or two tuples of 1..{SSIM_CROP_MAX_GROUPS} tensors each")
    for t in a + b + (rect,):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("ssim_crop: tensors must live on a HIP device (no CPU path)")
    if window_size != 11:
        raise RuntimeError("ssim_crop: only the reference's window_size = 11 is built")
    dev = a[0].device
    if rect.device != dev or any(t.device != dev for t in a + b):
        raise RuntimeError(f"ssim_crop: rect and the images must live on one device, got {rect.device} and {dev}")
    if rect.dtype != torch.int32 or rect.numel() != 4 or not rect.is_contiguous():
        raise ValueError("ssim_crop: rect must be a contiguous int32 [4] tensor (x, y, w, h)")
    for x, y in zip(a, b):
        if x.dim() != 3 or x.shape != y.shape or x.shape[1:] != a[0].shape[1:] or x.numel() == 0:
            raise ValueError(f"ssim_crop: every pair must be [C, H, W] with one H and W, got {tuple(x.shape)} and {tuple(y.shape)}")
    if sum(x.shape[0] for x in a) > 65535:
        raise ValueError("ssim_crop: at most 65535 planes")
    out = _SsimCrop.apply(rect, len(a), *a, *b)
    return out[0] if single else tuple(out)
