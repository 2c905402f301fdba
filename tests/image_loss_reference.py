"""Host restatements of the image-loss kernels (csrc/ssim.hip, csrc/ssim_crop.hip, csrc/loss.hip and the SSIM tile of
csrc/eval.hip) in numpy.  Nothing of the library is imported: the host tests that use this module run without a build.

Two evaluations of every SSIM quantity:

    float64   the reference's formulation (utils/loss_utils.py:25-66): the 11 x 11 window is the float32 outer product of the
              float32 1-D window, as create_window() builds it, applied as 121 taps in float64 with zero padding; every other
              operation in float64.  This is what the kernels are held to.
    float32   the "twin": the arithmetic the kernels spell out, in float32 with one rounding per operation (no FMA): the window
              applied separably, x then y, taps in the order 0..10, each accumulator starting at 0, products formed as
              w * (u * u), zero padding; then the map and the A / B / C planes by the expressions of ssim.hip in their order.
              Its distance from float64 is the rounding error of a CORRECT float32 evaluation, which is what local_bound() turns
              into the bound a kernel must keep.

    ssim_planes(img1, img2, dtype)                 -> map, A, B, C          [P, H, W] each
    ssim_backward(img1, img2, g, A, B, C, dtype)   -> dL/dimg1              general per-pixel g = dL/dmap
    ssim_crop(img1, img2, rect, upstream, dtype)   -> value, gradient       (and the planes, see there)
    phase1_loss(...)                               -> stats[8]
    alpha_mask_grad(...)                           -> dL_dcolor, dL_dalpha  float32, bit for bit
    local_bound(twin, ref)                         -> 2 E(p) + 4 ulp32 M(p), E(p) / M(p) the largest |twin - ref| / |ref| within 10 pixels"""
from math import exp

import numpy as np

F32, F64 = np.float32, np.float64
ULP32 = float(np.finfo(np.float32).eps)   # 2^-23
TILE = 16                                 # the SSIM kernels' tile (ssim_window.h)
BOUND_FACTOR, BOUND_ULPS, BOUND_RADIUS = 2.0, 4.0, 10
WINDOW_BITS = (0x3a86cab6, 0x3bf8ff01, 0x3d13758c, 0x3ddff87f, 0x3e5a1e1f, 0x3e8832b0)   # taps 0..5; 6..10 mirror them


def window():
    """gaussian(11, 1.5) of utils/loss_utils.py:26-28 as float32: the unnormalised values are Python floats rounded to float32 and
    divided by their float32 sum, which torch returns as the exact sum rounded once (adding them one after the other in float32
    gives one ulp less).  WINDOW_BITS pins the result; csrc/ssim_window.h forms the same eleven values."""
    g = np.array([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], F32)
    return (g / F32(g.astype(F64).sum())).astype(F32)


def window_2d():
    """create_window(): the float32 product of the 1-D window with itself (one rounding per entry), [11, 11] float32."""
    w = window()
    return (w[:, None] * w[None, :]).astype(F32)


def _conv_2d(x, w2):
    """121 taps, zero padding, in x's dtype.  x [P, H, W]."""
    P, H, W = x.shape
    xp = np.zeros((P, H + 10, W + 10), x.dtype)
    xp[:, 5:5 + H, 5:5 + W] = x
    out = np.zeros_like(x)
    for i in range(11):
        for j in range(11):
            out += w2[i, j] * xp[:, i:i + H, j:j + W]
    return out


def _conv_separable(x, w, fused=False):
    """11 taps along x into a zero-padded intermediate, then 11 along y; every accumulator starts at 0 and takes tap 0 first.
    fused: each tap is one fused multiply-add (the product exact, one rounding), what FMA contraction makes of the two loops."""
    if fused:
        tap = lambda acc, wk, v: (F64(wk) * v.astype(F64) + acc.astype(F64)).astype(F32)  # noqa: E731
    else:
        tap = lambda acc, wk, v: acc + wk * v  # noqa: E731
    P, H, W = x.shape
    xp = np.zeros((P, H, W + 10), x.dtype)
    xp[:, :, 5:5 + W] = x
    h = np.zeros((P, H, W), x.dtype)
    for k in range(11):
        h = tap(h, w[k], xp[:, :, k:k + W])
    hp = np.zeros((P, H + 10, W), x.dtype)
    hp[:, 5:5 + H, :] = h
    out = np.zeros((P, H, W), x.dtype)
    for k in range(11):
        out = tap(out, w[k], hp[:, k:k + H, :])
    return out


def _conv(x, dtype, fused=False):
    if dtype == F64:
        return _conv_2d(x, window_2d().astype(F64))
    return _conv_separable(x, window(), fused)


def _planes(a, dtype):
    a = np.asarray(a)
    assert a.ndim == 3, "images are [planes, H, W]"
    return np.ascontiguousarray(a, dtype=dtype)


def _constants(dtype):
    if dtype == F64:
        return 0.01 ** 2, 0.03 ** 2
    return F32(0.01) * F32(0.01), F32(0.03) * F32(0.03)


def ssim_planes(img1, img2, dtype=F64, fused_taps=False):
    """map, A, B, C as the header of csrc/ssim.hip defines them:
        f = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),
        A = df/dmu1 - 2 mu1 df/ds1 - mu2 df/ds12,   B = df/ds1,   C = df/ds12.
    fused_taps (float32 only): the window taps as fused multiply-adds, everything else unchanged -- another correct float32 evaluation,
    kept to show how far one strays from the twin by rounding alone (tests/test_image_loss_reference_host.py)."""
    dtype = np.dtype(dtype).type
    u, v = _planes(img1, dtype), _planes(img2, dtype)
    two = dtype(2.0)
    C1, C2 = _constants(dtype)
    with np.errstate(all="ignore"):
        mu1, mu2 = _conv(u, dtype, fused_taps), _conv(v, dtype, fused_taps)
        e11, e22, e12 = _conv(u * u, dtype, fused_taps), _conv(v * v, dtype, fused_taps), _conv(u * v, dtype, fused_taps)
        mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        sg1, sg2, sg12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
        a, b, c, d = two * mu12 + C1, two * sg12 + C2, mu1_sq + mu2_sq + C1, sg1 + sg2 + C2
        f = (a * b) / (c * d)
        df_dmu1 = (two * mu2 * b) / (c * d) - f * (two * mu1) / c
        df_ds1 = -f / d
        df_ds12 = (two * a) / (c * d)
        A = df_dmu1 - two * mu1 * df_ds1 - mu2 * df_ds12
    return f, A, df_ds1, df_ds12


def ssim_backward(img1, img2, g, A, B, C, dtype=F64, fused_taps=False):
    """dL/dimg1(p) = conv(g A)(p) + 2 img1(p) conv(g B)(p) + img2(p) conv(g C)(p): g = dL/dmap is applied UNDER the window (at the
    pixel whose map value it weights), not at the output pixel.  g: [P, H, W] or a scalar."""
    dtype = np.dtype(dtype).type
    u, v = _planes(img1, dtype), _planes(img2, dtype)
    g = np.broadcast_to(np.asarray(g, dtype), u.shape)
    with np.errstate(all="ignore"):
        a = _conv(g * _planes(A, dtype), dtype, fused_taps)
        b = _conv(g * _planes(B, dtype), dtype, fused_taps)
        c = _conv(g * _planes(C, dtype), dtype, fused_taps)
        return a + dtype(2.0) * u * b + v * c


def clip_rect(rect, H, W):
    """(x0, y0, x1, y1) of the (x, y, w, h) rectangle inside the frame; x1 <= x0 or y1 <= y0: empty."""
    x, y, w, h = (int(t) for t in rect)
    return max(x, 0), max(y, 0), min(x + max(w, 0), W), min(y + max(h, 0), H)


def ssim_crop(img1, img2, rect, upstream=1.0, dtype=F64):
    """SSIM of img[:, y:y+h, x:x+w] (train.py:269-281) as csrc/ssim_crop.hip states it: the rectangle is clipped to the frame, both
    images are zero outside it, the value is the sum of the map over the clipped rectangle / (planes w h), the gradient is the SSIM
    backward under g = upstream / (planes w h) inside the rectangle, and 0 outside it.  An empty rectangle gives 0 and zeros.
    Returns dict(value, grad, map, A, B, C, box): value a scalar of `dtype`; the planes are full frames, meaningful inside box =
    (x0, y0, x1, y1) only.  The float32 twin adds the map per 16 x 16 tile of the frame in float32 and the tiles in float64, and
    forms g in float32 as upstream / ((float) planes * (float) w * (float) h)."""
    dtype = np.dtype(dtype).type
    u, v = _planes(img1, dtype), _planes(img2, dtype)
    P, H, W = u.shape
    x0, y0, x1, y1 = box = clip_rect(rect, H, W)
    zero = np.zeros_like(u)
    if x1 <= x0 or y1 <= y0:
        return dict(value=dtype(0.0), grad=zero, map=zero, A=zero, B=zero, C=zero, box=box)
    inside = np.zeros((H, W), bool)
    inside[y0:y1, x0:x1] = True
    u, v = np.where(inside, u, dtype(0.0)), np.where(inside, v, dtype(0.0))
    f, A, B, C = ssim_planes(u, v, dtype)
    fm = np.where(inside, f, dtype(0.0))
    if dtype == F64:
        n = float(P) * float(x1 - x0) * float(y1 - y0)
        value = F64(fm.sum() / n)
        g = float(upstream) / n
    else:
        th, tw = -(-H // TILE), -(-W // TILE)
        padded = np.zeros((P, th * TILE, tw * TILE), F32)
        padded[:, :H, :W] = fm
        tiles = padded.reshape(P, th, TILE, tw, TILE).transpose(0, 1, 3, 2, 4).reshape(P, th, tw, TILE * TILE)
        partial = tiles.sum(axis=-1, dtype=F32)
        n = float(P) * float(x1 - x0) * float(y1 - y0)
        value = F32(partial.astype(F64).sum() / n)
        g = F32(upstream) / (F32(P) * F32(x1 - x0) * F32(y1 - y0))
    gmap = np.where(inside, dtype(g), dtype(0.0))[None]
    grad = ssim_backward(u, v, gmap, np.where(inside, A, 0), np.where(inside, B, 0), np.where(inside, C, 0), dtype)
    grad = np.where(inside, grad, dtype(0.0))
    return dict(value=value, grad=grad, map=fm, A=A, B=B, C=C, box=box)


# ---- csrc/loss.hip ------------------------------------------------------------------------------------------------------------------
STATS = ("loss", "n_bound", "1/(3 n_bound)", "1/n_bound", "image", "alpha", "normal", "axis")


def phase1_loss(color, alpha, extra, gt_image, gt_normal, alpha_target, bound, weights, normal_triple, axis_triple, dtype=F64):
    """The eight stats of gsr_phase1_loss_forward (include/gsr.h; train.py:261-265 with utils/loss_utils.py:20-24):
        (loss, n_bound, 1 / (3 n_bound), 1 / n_bound, L1(image), L2(alpha), L1(normal), L1(axis))
    with the means taken over the pixels whose bound != 0 (so -0.0 is outside, 0.5, 255 and NaN are inside) and n_bound replaced by 1
    in the divisors when the mask is empty.  color / gt_image / gt_normal [3, n], extra [18, n], alpha / alpha_target / bound [n].
    float64: everything in float64.  float32 twin: the per-pixel terms in float32, added over 256 consecutive pixels in float32, the
    256-pixel sums added in float64 and finished in float64 like the kernel's last workgroup.  Returns float64[8] (dtype float64) or
    float32[8]."""
    dtype = np.dtype(dtype).type
    n = np.asarray(bound).size
    inside = ~(np.asarray(bound, F32).reshape(n) == 0)   # != 0, NaN included
    col, gti, gtn = (np.asarray(t, dtype).reshape(3, n) for t in (color, gt_image, gt_normal))
    ex = np.asarray(extra, dtype).reshape(18, n)
    nrm, axs = ex[3 * normal_triple:3 * normal_triple + 3], ex[3 * axis_triple:3 * axis_triple + 3]
    da = np.asarray(alpha, dtype).reshape(n) - np.asarray(alpha_target, dtype).reshape(n)

    def l1(a, b):
        t = np.abs(a - b)
        return (t[0] + t[1]) + t[2] if dtype == F64 else ((dtype(0) + t[0]) + t[1]) + t[2]
    terms = np.stack([l1(col, gti), da * da, l1(nrm, gtn), l1(axs, gtn), np.ones(n, dtype)])
    with np.errstate(invalid="ignore"):
        terms = np.where(inside[None], terms, dtype(0.0))
    if dtype == F64:
        tot = terms.sum(axis=1)
    else:
        pad = (-n) % 256
        chunks = np.concatenate([terms, np.zeros((5, pad), F32)], axis=1).reshape(5, -1, 256)
        tot = chunks.sum(axis=2, dtype=F32).astype(F64).sum(axis=1)
    nb = tot[4] if tot[4] > 0 else 1.0
    li, la, ln, lx = tot[0] / (3.0 * nb), tot[1] / nb, tot[2] / (3.0 * nb), tot[3] / (3.0 * nb)
    w = [float(F32(t)) for t in weights]
    out = np.array([w[0] * li + w[1] * la + w[2] * ln + w[3] * lx, tot[4], 1.0 / (3.0 * nb), 1.0 / nb, li, la, ln, lx], F64)
    return out if dtype == F64 else out.astype(F32)


def alpha_mask_grad(color, alpha, gt, mask, lam):
    """gsr_alpha_mask_loss_backward in float32, operation for operation: dL_dcolor = sign3(color - gt) / (3 n) with the three-way
    sign (+1, -1, and 0 on an exact tie, on -0.0 and on NaN), dL_dalpha = (2 lambda / n) (alpha - mask).  color / gt [3, n]."""
    color, gt = np.asarray(color, F32), np.asarray(gt, F32)
    alpha, mask = np.asarray(alpha, F32), np.asarray(mask, F32)
    n = alpha.size
    sc = F32(1.0) / (F32(3.0) * F32(n))
    sa = F32(2.0) * F32(lam) / F32(n)
    with np.errstate(invalid="ignore"):
        d = color - gt
        dcolor = np.where(d > 0, sc, np.where(d < 0, -sc, F32(0.0))).astype(F32)
        dalpha = (sa * (alpha - mask)).astype(F32)
    return dcolor, dalpha


# ---- the bound ----------------------------------------------------------------------------------------------------------------------
def _local_max(e, radius=BOUND_RADIUS):
    """The largest value over the (2 radius + 1)^2 neighbourhood of each element within its plane.  [..., H, W], values >= 0."""
    H, W = e.shape[-2:]
    pad = [(0, 0)] * (e.ndim - 2)
    ex = np.pad(e, pad + [(0, 0), (radius, radius)])
    e = np.max([ex[..., k:k + W] for k in range(2 * radius + 1)], axis=0)
    ey = np.pad(e, pad + [(radius, radius), (0, 0)])
    return np.max([ey[..., k:k + H, :] for k in range(2 * radius + 1)], axis=0)


def local_error(twin, ref, radius=BOUND_RADIUS):
    """E(p): the largest |twin - ref| over the (2 radius + 1)^2 neighbourhood of p within its plane.  [..., H, W]."""
    return _local_max(np.abs(np.asarray(twin, F64) - np.asarray(ref, F64)), radius)


def local_bound(twin, ref, factor=BOUND_FACTOR):
    """What a float32 kernel may be off by at each element: factor x E(p) + 4 float32 ulps of the largest |ref| in the SAME
    neighbourhood.  The floor is local like E(p): with 4 ulps of the whole tensor's maximum (never smaller than this, so a kernel
    within this bound is within that one) the flat half of half_and_half, where |B| and |C| reach 1 / C2, would loosen the textured
    half's bound for B and C about twentyfold."""
    ref = np.asarray(ref, F64)
    return factor * local_error(twin, ref) + BOUND_ULPS * ULP32 * _local_max(np.abs(ref))


def global_floor_bound(twin, ref, factor=BOUND_FACTOR):
    """The same with the floor taken from the whole tensor, factor x E(p) + 4 ulp32 max|ref|: never below local_bound()."""
    ref = np.asarray(ref, F64)
    return factor * local_error(twin, ref) + BOUND_ULPS * ULP32 * float(np.abs(ref).max(initial=0.0))


def scalar_bound(twin, ref, factor=BOUND_FACTOR):
    """The same form for a scalar: factor x |twin - ref| + 4 float32 ulps of |ref|."""
    return factor * abs(float(twin) - float(ref)) + BOUND_ULPS * ULP32 * abs(float(ref))
