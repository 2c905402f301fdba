"""The PBR-phase training loss of train.py:296-363 (iterations > 30,000) on csrc/pbr_loss.hip, without host synchronisation:

    get_masked_tv_loss(mask, prediction)          train.py:81-95 (mask takes a gradient, as in the reference)
    gaussian_entropy(x, bins=15, min=0, max=1)     train.py:47-71 (columns 0..2 of x.view(-1, W); see the sigma = 0 rule below)
    MaterialSmoothness(knn)(albedo_g, roughness_g) the bracket at train.py:341 (utils/loss_utils.py:102-124), without its 0.1
    PbrPhaseLoss(gt_image, bound_mask, knn)(render_rgb, alpha, albedo, roughness, albedo_g, roughness_g) -> (loss, terms)
        loss = w_l1 * L1 + w_tv * TV + w_entropy * entropy + w_smooth * smoothness + w_lamb * roughness prior (0-dim), terms = the
        five unweighted values in that order (a device tensor: logging it needs no synchronisation here)

Every branch of the reference (the masked means, `if hi.sum() > eps`) is decided on the device: a call makes no host read, and a PBR
step that uses these records into graph.GraphedFrame.  One deliberate divergence: an entropy column whose branch is
not taken (a constant column, sigma = 0) gets a zero gradient; the reference's autograd gives NaN there (0 * inf) whenever another
column takes its branch.  Tensors must live on the GPU (no CPU path); they are read as float32."""
import ctypes as C

import torch

from .._lib import PbrLoss, call, lib, ptr

N_TERMS = 5  # l1, tv, entropy, smooth, prior


def _on_dev(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: tensors must live on a HIP device (no CPU path)")
    return t


def _dev(t, what):
    return _on_dev(t, what).detach().contiguous().float()


def _rgb(t):
    """render_rgb as the kernels read it: any dense layout (train.py passes an [H, W, 3] tensor permuted to [3, H, W]) is kept."""
    t = t.detach()
    if not t.is_cuda:
        raise RuntimeError("PbrPhaseLoss: tensors must live on a HIP device (no CPU path)")
    order = sorted(range(t.dim()), key=lambda d: -t.stride(d))
    if t.dtype != torch.float32 or not t.permute(order).is_contiguous():  # (a dense permutation of a contiguous tensor is kept)
        t = t.contiguous().float()
    return t


class _Spec:
    """What stays fixed between calls: targets, knn tables, term flags and weights."""
    def __init__(self, H, W, gt=None, bound=None, tv=False, entropy=(False, False), prior=False, bins=15, lo=0.0, hi=1.0,
                 smooth=None, w=(1.0, 1.0, 1.0, 1.0, 1.0)):
        self.H, self.W, self.gt, self.bound = H, W, gt, bound
        self.tv, self.entropy, self.prior = tv, entropy, prior
        self.bins, self.lo, self.hi = bins, lo, hi
        self.smooth, self.w = smooth, w

    def struct(self, rgb, mask, a, b, g0, g1):
        s = PbrLoss()
        s.width, s.height = self.W, self.H
        if rgb is not None:
            s.rgb, s.gt, s.bound = ptr(rgb), ptr(self.gt), ptr(self.bound)
            s.rgb_stride[:] = list(rgb.stride())
        s.a, s.b, s.mask = ptr(a), ptr(b), ptr(mask)
        s.ca = a.shape[0] if a is not None else 0
        s.cb = b.shape[0] if b is not None else 0
        s.tv, s.prior = int(self.tv), int(self.prior)
        s.entropy[0], s.entropy[1] = int(self.entropy[0]), int(self.entropy[1])
        s.bins, s.lo, s.hi = self.bins, self.lo, self.hi
        if self.smooth is not None and (g0 is not None or g1 is not None):
            sm = self.smooth
            s.P, s.k1, s.k2 = sm.P, ptr(sm.k1), ptr(sm.k2)
            s.inv_off[0], s.inv_off[1], s.inv_idx[0], s.inv_idx[1] = ptr(sm.off1), ptr(sm.off2), ptr(sm.idx1), ptr(sm.idx2)
            for i, g in enumerate((g0, g1)):
                s.g[i], s.gc[i] = ptr(g), (g.shape[1] if g is not None else 0)
        s.w_l1, s.w_tv, s.w_entropy, s.w_smooth, s.w_prior = self.w
        return s


class _PbrLossFn(torch.autograd.Function):
    """(loss 0-dim, terms [5]) of the terms spec enables over rgb [3,H,W], mask [H,W], a [Ca,H,W], b [Cb,H,W], g0 / g1 [P,C]."""
    @staticmethod
    def forward(ctx, spec, rgb, mask, a, b, g0, g1):
        rgb = _rgb(rgb) if rgb is not None else None
        mask, a, b, g0, g1 = (_dev(t, "pbr loss") if t is not None else None for t in (mask, a, b, g0, g1))
        dev = next(t.device for t in (rgb, mask, a, b, g0, g1) if t is not None)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        terms = torch.empty(N_TERMS, device=dev, dtype=torch.float32)
        ws = torch.empty(int(lib.gsr_pbr_loss_workspace_floats()), device=dev, dtype=torch.float32)
        s = spec.struct(rgb, mask, a, b, g0, g1)
        s.loss, s.terms = loss.data_ptr(), terms.data_ptr()
        call("gsr_pbr_loss_forward", dev, C.byref(s), ws.data_ptr())
        ctx.spec = spec
        ctx.present = [t is not None for t in (rgb, mask, a, b, g0, g1)]
        ctx.save_for_backward(ws, *[t for t in (rgb, mask, a, b, g0, g1) if t is not None])
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, g_terms):
        ws, *saved = ctx.saved_tensors
        it = iter(saved)
        rgb, mask, a, b, g0, g1 = (next(it) if p else None for p in ctx.present)
        need = ctx.needs_input_grad[1:]
        outs = [torch.empty_like(t) if (t is not None and n) else None for t, n in zip((rgb, mask, a, b, g0, g1), need)]
        s = ctx.spec.struct(rgb, mask, a, b, g0, g1)
        dummy = torch.empty(N_TERMS + 1, device=ws.device, dtype=torch.float32)  # (the forward's outputs are not rewritten)
        s.loss, s.terms = dummy.data_ptr(), dummy.data_ptr() + 4
        up = g_loss.detach().contiguous().float() if g_loss is not None else torch.zeros((), device=ws.device)
        s.upstream = up.data_ptr()
        s.d_rgb, s.d_mask, s.d_a, s.d_b = (ptr(o) for o in outs[:4])
        s.d_g[0], s.d_g[1] = ptr(outs[4]), ptr(outs[5])
        if any(o is not None for o in outs):
            call("gsr_pbr_loss_backward", ws.device, C.byref(s), ws.data_ptr())
        return (None, *outs)


def _mask2d(mask, H, W, what):
    m = _on_dev(mask, what)
    if m.numel() != H * W:
        raise ValueError(f"{what}: mask must be [1, {H}, {W}], got {tuple(mask.shape)}")
    return mask.reshape(H, W)


def get_masked_tv_loss(mask, prediction):
    """train.py:81-95: mask [1,H,W], prediction [C,H,W]; (Delta pred)^2 times the product of the two masks, averaged with the
    masked-out entries in the denominators.  Gradients reach prediction and mask."""
    if prediction.dim() != 3:
        raise ValueError(f"get_masked_tv_loss: prediction must be [C, H, W], got {tuple(prediction.shape)}")
    _on_dev(prediction, "get_masked_tv_loss")
    Cc, H, W = prediction.shape
    m = _mask2d(mask, H, W, "get_masked_tv_loss")
    spec = _Spec(H, W, tv=True, w=(0.0, 1.0, 0.0, 0.0, 0.0))
    return _PbrLossFn.apply(spec, None, _as_f32(m), _as_f32(prediction), None, None, None)[0]


def gaussian_entropy(x, bins=15, min=0.0, max=1.0):
    """train.py:47-71: the summed entropy of the Gaussian-kernel histograms of columns 0..2 of x.view(-1, x.shape[-1]) (sigma is the
    column's unbiased variance).  A column whose histogram sums to <= 1e-6 (NaN included) adds 0 and gets a zero gradient."""
    _on_dev(x, "gaussian_entropy")
    W = x.shape[-1] if x.dim() else 1
    if W < 3:
        raise ValueError(f"gaussian_entropy: the last dimension must be at least 3 (columns 0..2 enter the loss), got {W}")
    if not 1 <= int(bins) <= 32:
        raise ValueError("gaussian_entropy: 1..32 bins are built")
    x2 = x.reshape(1, -1, W)
    spec = _Spec(x2.shape[1], W, entropy=(True, False), bins=int(bins), lo=float(min), hi=float(max), w=(0.0, 0.0, 1.0, 0.0, 0.0))
    return _PbrLossFn.apply(spec, None, None, _as_f32(x2), None, None, None)[0]


def _as_f32(t):
    return t if t.dtype == torch.float32 else t.float()


class MaterialSmoothness:
    """The per-Gaussian material smoothness of train.py:341 over knn [P, 3] (gaussians.get_knn_3[0]; column 0, the point itself,
    is unused): sum over the given tensors g [P, C] of mean |g[k1] - g[k2]| / (g[k2] + 1e-6), k1 = knn[:, 1], k2 = knn[:, 2].
    The set-up checks the indices on the host (one synchronisation) and builds the inverse tables the gathering backward reads;
    calls do neither."""
    def __init__(self, knn):
        if not isinstance(knn, torch.Tensor) or not knn.is_cuda:
            raise RuntimeError("MaterialSmoothness: knn must live on a HIP device (no CPU path)")
        if knn.dim() != 2 or knn.shape[1] < 3 or knn.shape[0] < 1 or knn.dtype.is_floating_point:
            raise ValueError(f"MaterialSmoothness: knn must be integer [P, 3], got {tuple(knn.shape)} {knn.dtype}")
        P = knn.shape[0]
        if P >= 2 ** 31 - 1:
            raise ValueError("MaterialSmoothness: P must fit in int32")
        kk = knn[:, 1:3]
        if bool(((kk < 0) | (kk >= P)).any()):
            raise ValueError(f"MaterialSmoothness: knn indices must lie in [0, {P})")
        self.P = P
        self.k1, self.k2 = (kk[:, i].to(torch.int32).contiguous() for i in range(2))
        self.off1, self.idx1 = self._inverse(self.k1)
        self.off2, self.idx2 = self._inverse(self.k2)

    def _inverse(self, k):
        idx = torch.argsort(k, stable=True).to(torch.int32)
        counts = torch.bincount(k.long(), minlength=self.P)
        off = torch.zeros(self.P + 1, device=k.device, dtype=torch.int64)
        off[1:] = torch.cumsum(counts, 0)
        return off.to(torch.int32).contiguous(), idx.contiguous()

    def check(self, g, what):
        if g is None:
            return None
        _on_dev(g, what)
        if g.dim() != 2 or g.shape[0] != self.P:
            raise ValueError(f"{what}: expected [{self.P}, C] (the P knn was built for), got {tuple(g.shape)}")
        return _as_f32(g)

    def __call__(self, albedo_g, roughness_g=None):
        a, r = self.check(albedo_g, "albedo_g"), self.check(roughness_g, "roughness_g")
        if a is None and r is None:
            raise ValueError("MaterialSmoothness: at least one tensor is needed")
        spec = _Spec(1, 1, smooth=self, w=(0.0, 0.0, 0.0, 1.0, 0.0))
        return _PbrLossFn.apply(spec, None, None, None, None, a, r)[0]


class PbrPhaseLoss:
    """The PBR-phase loss of train.py:316-344 without SSIM and LPIPS, fused:
        w_l1 * masked L1(render_rgb, gt_image | bound_mask == 1)     train.py:316
      + w_tv * get_masked_tv_loss(alpha, [albedo; roughness])        :326
      + w_entropy * (gaussian_entropy(albedo) + gaussian_entropy(roughness))   :333
      + w_smooth * MaterialSmoothness(knn)(albedo_g, roughness_g)    :341 (off when knn or both tensors are None)
      + w_lamb * (1 - roughness[alpha > 0]).mean()                    :344
    gt_image [3,H,W] and bound_mask [1,H,W] are the camera's targets.  Float32 contiguous targets are used in place: an in-place
    update of the caller's tensor is seen by the next call (what a captured graph needs).  Any other dtype or layout (a bool
    bound_mask, say) is copied here once, later updates of the caller's tensor are NOT seen, and targets_in_place is False.
    knn: [P, 3] integer indices, or a MaterialSmoothness built once from them.  Building one checks the indices on the host (one
    synchronisation) and sorts them, so a loop that makes a PbrPhaseLoss per camera passes the same MaterialSmoothness each time.
    Returns (loss, terms): a 0-dim tensor and the five unweighted terms on the device."""
    def __init__(self, gt_image, bound_mask, knn=None, w_l1=1.0, w_tv=1.0, w_entropy=5e-5, w_smooth=0.1, w_lamb=0.001):
        gt = _dev(gt_image, "PbrPhaseLoss")
        if gt.dim() != 3 or gt.shape[0] != 3:
            raise ValueError(f"PbrPhaseLoss: gt_image must be [3, H, W], got {tuple(gt_image.shape)}")
        self.H, self.W = gt.shape[1:]
        if self.W < 3:
            raise ValueError("PbrPhaseLoss: the entropy term needs W >= 3")
        bound = _dev(bound_mask, "PbrPhaseLoss")
        self.targets_in_place = all(t.dtype == torch.float32 and t.is_contiguous() for t in (gt_image, bound_mask))
        self.gt = gt
        self.bound = _mask2d(bound, self.H, self.W, "PbrPhaseLoss")
        self.smooth = knn if isinstance(knn, MaterialSmoothness) else (MaterialSmoothness(knn) if knn is not None else None)
        self.weights = tuple(float(v) for v in (w_l1, w_tv, w_entropy, w_smooth, w_lamb))

    def __call__(self, render_rgb, alpha, albedo, roughness, albedo_g=None, roughness_g=None):
        H, W = self.H, self.W
        for name, t, c in (("render_rgb", render_rgb, 3), ("albedo", albedo, 3), ("roughness", roughness, 1)):
            _on_dev(t, "PbrPhaseLoss")
            if tuple(t.shape) != (c, H, W):
                raise ValueError(f"PbrPhaseLoss: {name} must be [{c}, {H}, {W}], got {tuple(t.shape)}")
        m = _mask2d(alpha, H, W, "PbrPhaseLoss")
        g0 = g1 = None
        if albedo_g is not None or roughness_g is not None:
            if self.smooth is None:
                raise ValueError("PbrPhaseLoss: per-Gaussian materials were given but no knn")
            g0, g1 = self.smooth.check(albedo_g, "albedo_g"), self.smooth.check(roughness_g, "roughness_g")
        spec = _Spec(H, W, gt=self.gt, bound=self.bound, tv=True, entropy=(True, True), prior=True, smooth=self.smooth,
                     w=self.weights)
        return _PbrLossFn.apply(spec, render_rgb, _as_f32(m), _as_f32(albedo), _as_f32(roughness), g0, g1)
