"""The host restatements the GPU image-loss tests compare against (tests/image_loss_reference.py), checked without a GPU and
without the library: the float64 reference against autograd of the reference's conv2d formulation in float64 (value and gradient
under a NON-uniform dL/dmap, full frame and crop), against the fixture the reference's own ssim() made on rendering-like crops, the
float32 twin against float64 per input family (the e32 table, printed), the two conditions the measured bound has to meet, and the
phase-1 / alpha-mask restatements against the torch statements of train.py:261-265."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import image_loss_cases as K
from tests import image_loss_reference as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_crop.npz")
TENSORS = ("map", "A", "B", "C", "grad")


def conv2d_ssim_map(img1, img2):
    """utils/loss_utils.py:25-61 for [1, C, H, W] tensors: the map, before any mean."""
    gauss = torch.Tensor([np.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    w1 = (gauss / gauss.sum()).unsqueeze(1)
    C = img1.size(-3)
    window = w1.mm(w1.t()).float()[None, None].expand(C, 1, 11, 11).contiguous().type_as(img1)
    mu1, mu2 = F.conv2d(img1, window, padding=5, groups=C), F.conv2d(img2, window, padding=5, groups=C)
    s1 = F.conv2d(img1 * img1, window, padding=5, groups=C) - mu1.pow(2)
    s2 = F.conv2d(img2 * img2, window, padding=5, groups=C) - mu2.pow(2)
    s12 = F.conv2d(img1 * img2, window, padding=5, groups=C) - mu1 * mu2
    return ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1.pow(2) + mu2.pow(2) + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))


def _autograd(a, b, g):
    """map and d sum(g map) / d img1 of the conv2d formulation in float64 (numpy in, numpy out; [P, H, W])."""
    x = torch.from_numpy(np.asarray(a, np.float64))[None].requires_grad_(True)
    m = conv2d_ssim_map(x, torch.from_numpy(np.asarray(b, np.float64))[None])
    (m * torch.from_numpy(np.asarray(g, np.float64))[None]).sum().backward()
    return m.detach()[0].numpy(), x.grad[0].numpy()


def _close64(got, want, what, rel=1e-11):
    scale = float(np.abs(want).max()) or 1.0
    err = float(np.abs(np.asarray(got) - want).max())
    assert err <= rel * scale, f"{what}: {err:.3e} against a magnitude of {scale:.3e}"


def test_the_window_is_the_references_bit_for_bit():
    gauss = torch.Tensor([np.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    w1 = (gauss / gauss.sum())
    assert np.array_equal(R.window(), w1.numpy())
    assert tuple(int(v) for v in R.window().view(np.uint32)) == R.WINDOW_BITS + R.WINDOW_BITS[4::-1]
    assert np.array_equal(R.window_2d(), w1.unsqueeze(1).mm(w1.unsqueeze(0)).numpy())


@pytest.mark.parametrize("family", K.FAMILIES)
def test_float64_reference_against_autograd_of_the_conv2d_formulation(family):
    for shape in ((6, 11), (17, 33), (47, 33), (1, 17)):
        H, W = shape
        P = K.planes_of(shape)
        a, b = K.make(family, H, W, P)
        g = K.upstream_map(H, W, P)
        want_map, want_grad = _autograd(a, b, g)
        m, A, B, C = R.ssim_planes(a, b, np.float64)
        _close64(m, want_map, f"{family} {shape} map")
        # against the sum of the magnitudes of the gradient's three terms: they cancel to nothing where the images are identical
        terms = float(np.abs(g).max()) * float(np.abs(A).max() + 2 * np.abs(a).max() * np.abs(B).max() + np.abs(b).max() * np.abs(C).max())
        err = float(np.abs(R.ssim_backward(a, b, g, A, B, C, np.float64) - want_grad).max())
        assert err <= 1e-12 * terms, f"{family} {shape} gradient: {err:.3e} against terms of {terms:.3e}"


def test_the_gradient_weights_the_map_under_the_window_not_at_the_output_pixel():
    """What a uniform dL/dmap cannot tell apart: with g nonzero at one pixel, the gradient covers that pixel's 11 x 11 footprint."""
    a, b = K.make("noise", 17, 33, 1)
    g = np.zeros((1, 17, 33))
    g[0, 8, 20] = 1.0
    m, A, B, C = R.ssim_planes(a, b)
    grad = R.ssim_backward(a, b, g, A, B, C)
    ys, xs = np.nonzero(grad[0])
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (3, 13, 15, 25)
    _close64(grad, _autograd(a, b, g)[1], "one-pixel g", rel=1e-9)


RECTS = {"interior": (9, 5, 20, 14), "overhang": (30, 22, 1000, 1000), "negative": (-5, -3, 20, 15), "one_pixel": (7, 9, 1, 1),
         "empty": (20, 30, 0, 15), "outside": (500, 500, 10, 10)}


@pytest.mark.parametrize("name", list(RECTS))
def test_float64_crop_against_autograd_on_the_slice(name):
    """train.py:269-281: ssim(img[:, y:y+h, x:x+w][None], gt[...]) on the rectangle clipped to the frame, times a non-unit upstream."""
    H, W, P, up = 38, 53, 3, -0.37
    rect = RECTS[name]
    for family in ("noise", "render_white"):
        a, b = K.make(family, H, W, P)
        got = R.ssim_crop(a, b, rect, up, np.float64)
        x0, y0, x1, y1 = R.clip_rect(rect, H, W)
        if x1 <= x0 or y1 <= y0:
            assert float(got["value"]) == 0.0 and not got["grad"].any()
            continue
        x = torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
        v = conv2d_ssim_map(x[:, y0:y1, x0:x1][None], torch.from_numpy(b.astype(np.float64))[:, y0:y1, x0:x1][None]).mean()
        (up * v).backward()
        assert abs(float(got["value"]) - float(v.detach())) <= 1e-12
        _close64(got["grad"], x.grad.numpy(), f"{name} {family} gradient", rel=1e-9)
        outside = got["grad"].copy()
        outside[:, y0:y1, x0:x1] = 0.0
        assert not outside.any()
        assert (x1 - x0) * (y1 - y0) < rect[2] * rect[3] or name in ("interior", "one_pixel")   # the overhang divides by the clipped area


@pytest.mark.parametrize("name", list(K.GOLDEN_CROPS))
def test_float64_crop_against_the_fixture_of_the_references_own_ssim(name):
    fx = np.load(FIXTURE)
    family, H, W, P, rect = K.GOLDEN_CROPS[name]
    assert tuple(fx[f"{name}/rect"]) == rect and rect[2] <= 80 and rect[3] <= 64
    a, b = K.make(family, H, W, P)
    got = R.ssim_crop(a, b, rect, 1.0, np.float64)
    x, y, w, h = rect
    assert abs(float(got["value"]) - float(fx[f"{name}/value"])) <= 1e-13
    _close64(got["grad"][:, y:y + h, x:x + w], fx[f"{name}/grad"], name, rel=1e-9)
    if name == "render_black_tile_edges":
        assert (x + w) % R.TILE == 0 and (y + h) % R.TILE == 0


# ---- the twin, the e32 table and the two conditions on the bound --------------------------------------------------------------------
def _both(family, H, W, P, g):
    a, b = K.make(family, H, W, P)
    out = {}
    for dt in (np.float64, np.float32):
        m, A, B, C = R.ssim_planes(a, b, dt)
        out[dt] = dict(map=m, A=A, B=B, C=C, grad=R.ssim_backward(a, b, g, A, B, C, dt))
    return out[np.float64], out[np.float32]


def test_twin_against_float64_per_family_and_the_bound_meets_its_two_conditions():
    H, W, P = 47, 64, 3
    uniform = np.float32(1.0 / (P * H * W))
    print(f"\n    e32 = max|twin32 - f64| / max|f64| at {P} x {H} x {W}, uniform dL/dmap (the mean)")
    print("    family          " + "".join(f"{t:>10s}" for t in TENSORS) + "     value")
    rows = {}
    for family in K.FAMILIES:
        r64, r32 = _both(family, H, W, P, uniform)
        rows[family] = (r64, r32)
        rel = [float(np.abs(r32[t] - r64[t]).max()) / (float(np.abs(r64[t]).max()) or 1.0) for t in TENSORS]
        a, b = K.make(family, H, W, P)
        full = (0, 0, W, H)
        dv = abs(float(R.ssim_crop(a, b, full, 1.0, np.float32)["value"]) - float(R.ssim_crop(a, b, full, 1.0, np.float64)["value"]))
        print(f"    {family:16s}" + "".join(f"{v:10.1e}" for v in rel) + f"{dv:10.1e}")
        for t in TENSORS:
            assert np.isfinite(r32[t]).all() and np.isfinite(r64[t]).all(), (family, t)
    # 1. on the inputs the suite drew so far the measured bound is tighter than its fixed ones
    r64, r32 = rows["noise"]
    assert float(R.local_bound(r32["grad"], r64["grad"]).max()) < 2e-5 * float(np.abs(r64["grad"]).max())
    a, b = K.make("noise", H, W, P)
    v64, v32 = (R.ssim_crop(a, b, (0, 0, W, H), 1.0, dt)["value"] for dt in (np.float64, np.float32))
    assert R.scalar_bound(v32, v64) < 2e-6
    assert abs(float(v64) - float(r64["map"].mean())) < 1e-14
    # 2. the flat half of half_and_half does not loosen the textured half: for every tensor the median of the bound over the noise
    # half stays within 2 x of the pure-noise case.  Both E(p) and the floor are local; with the floor taken from the whole tensor
    # (printed for comparison, never below the local one) B and C would miss this about twentyfold, max|B| being 1 / C2 on flat white
    h64, h32 = rows["half_and_half"]
    left = slice(0, W // 2)
    ratio = lambda f, t: float(np.median(f(h32[t], h64[t])[..., left]) / np.median(f(r32[t], r64[t])[..., left]))  # noqa: E731
    print("    median of the bound over the noise half, half_and_half / noise: " + ", ".join(
        f"{t} {ratio(R.local_bound, t):.2f}" for t in TENSORS))
    print("    the same with the floor of the whole tensor's maximum:          " + ", ".join(
        f"{t} {ratio(R.global_floor_bound, t):.2f}" for t in TENSORS))
    for t in TENSORS:
        assert ratio(R.local_bound, t) <= 2.0, t
        for rows_t in (rows["half_and_half"], rows["noise"]):
            assert (R.local_bound(rows_t[1][t], rows_t[0][t]) <= R.global_floor_bound(rows_t[1][t], rows_t[0][t])).all(), t


def test_fused_window_taps_alone_leave_the_factor_two_bound_on_flat_backgrounds():
    """Why csrc/ssim.hip and csrc/ssim_crop.hip are built without FMA contraction rather than given a larger factor: the twin with nothing
    changed but its 22 taps fused (each MORE accurate than a multiply and an add) keeps the bound on noise and leaves it, by rounding
    alone, where the variances cancel -- there the twin's own error is no measure of another correct float32 evaluation's."""
    def worst(family, shape, tensor):
        H, W = shape
        P = K.planes_of(shape)
        a, b = K.make(family, H, W, P)
        g = K.upstream_map(H, W, P)
        out = []
        for dt, fused in ((np.float64, False), (np.float32, False), (np.float32, True)):
            m, A, B, C = R.ssim_planes(a, b, dt, fused_taps=fused)
            out.append(dict(map=m, A=A, B=B, C=C, grad=R.ssim_backward(a, b, g, A, B, C, dt, fused_taps=fused))[tensor])
        r64, r32, fused32 = out
        return float((np.abs(fused32 - r64) / R.global_floor_bound(r32, r64)).max())
    shares = {(f, t): max(worst(f, s, t) for s in ((16, 32), (32, 47), (47, 33))) for f in ("noise", "render_white", "out_of_range")
              for t in ("A", "grad")}
    print("\n    fused taps, worst share of the factor-two bound: " + ", ".join(f"{f} {t} {v:.2f}" for (f, t), v in shares.items()))
    assert shares["noise", "A"] <= 1.0 and shares["noise", "grad"] <= 1.0
    assert max(shares["render_white", "A"], shares["render_white", "grad"], shares["out_of_range", "grad"]) > 1.2


def test_local_bound_is_local_in_both_of_its_terms():
    ref = np.zeros((1, 40, 40))
    ref[0, 0, 0] = 3.0
    twin = ref.copy()
    twin[0, 20, 20] += 1e-3
    b = R.local_bound(twin, ref)
    floor = 4 * 2.0 ** -23 * 3.0
    assert b.shape == ref.shape and np.isclose(b[0, 20, 20], 2e-3) and np.isclose(b[0, 10, 30], 2e-3)
    assert b[0, 9, 10] == floor and b[0, 5, 5] == floor and b[0, 10, 9] == floor         # within 10 pixels of the 3.0 only
    assert np.isclose(b[0, 10, 10], 2e-3 + floor)                                            # within 10 pixels of both
    assert b[0, 9, 20] == 0.0 and b[0, 20, 31] == 0.0 and b[0, 35, 5] == 0.0                # the floor is local too
    g = R.global_floor_bound(twin, ref)
    assert (g >= b).all() and g.min() == floor and np.isclose(g[0, 20, 20], 2e-3 + floor)


# ---- csrc/loss.hip ------------------------------------------------------------------------------------------------------------------
def _phase1_inputs(n, seed, bound_values=(0.0, 1.0)):
    r = np.random.default_rng([31, n, seed])
    f = lambda *s: r.uniform(0.0, 1.0, s).astype(np.float32)  # noqa: E731
    d = dict(color=f(3, n), alpha=f(n), extra=f(18, n), gt_image=f(3, n), gt_normal=f(3, n), alpha_target=(f(n) > 0.5).astype(np.float32))
    d["bound"] = np.asarray(bound_values, np.float32)[r.integers(0, len(bound_values), n)]
    tie = r.uniform(0, 1, n) < 0.3   # background pixels: the rendering equals the target exactly
    d["color"][:, tie] = d["gt_image"][:, tie]
    return d


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_phase1_restatement_against_the_torch_statements(n):
    d = _phase1_inputs(n, 0)
    d["bound"][0] = 1.0
    w = (1.0, 0.1, 0.01, 0.05)
    for nt, at in ((0, 5), (3, 3), (5, 1)):
        got = R.phase1_loss(weights=w, normal_triple=nt, axis_triple=at, dtype=np.float64, **d)
        t = {k: torch.from_numpy(v.astype(np.float64)) for k, v in d.items()}
        sel = t["bound"] == 1   # train.py:261-265 index with bound_mask == 1
        l1 = lambda x, y: torch.abs(x.t()[sel] - y.t()[sel]).mean()  # noqa: E731
        li = l1(t["color"], t["gt_image"])
        la = ((t["alpha"][sel] - t["alpha_target"][sel]) ** 2).mean()
        ln = l1(t["extra"][3 * nt:3 * nt + 3], t["gt_normal"])
        lx = l1(t["extra"][3 * at:3 * at + 3], t["gt_normal"])
        nb = int(sel.sum())
        want = [np.float32(w[0]) * li + np.float32(w[1]) * la + np.float32(w[2]) * ln + np.float32(w[3]) * lx, nb, 1 / (3 * nb), 1 / nb,
                li, la, ln, lx]
        assert np.allclose(got, np.array([float(v) for v in want]), rtol=1e-12, atol=0)
        twin = R.phase1_loss(weights=w, normal_triple=nt, axis_triple=at, dtype=np.float32, **d)
        assert twin.dtype == np.float32 and twin[1] == nb and np.allclose(twin, got, rtol=1e-5)


def test_phase1_bound_rule_is_not_zero_and_the_empty_mask_divides_by_one():
    d = _phase1_inputs(300, 1)
    d["bound"] = np.tile(np.array([0.0, -0.0, 1.0, 0.5, 255.0, np.nan], np.float32), 50)
    ones = dict(d, bound=np.tile(np.array([0, 0, 1, 1, 1, 1], np.float32), 50))
    for dt in (np.float64, np.float32):
        a = R.phase1_loss(weights=(1, 1, 1, 1), normal_triple=0, axis_triple=5, dtype=dt, **d)
        b = R.phase1_loss(weights=(1, 1, 1, 1), normal_triple=0, axis_triple=5, dtype=dt, **ones)
        assert a[1] == 200 and np.array_equal(a, b)
        e = R.phase1_loss(weights=(1, 1, 1, 1), normal_triple=0, axis_triple=5, dtype=dt, **dict(d, bound=np.zeros(300, np.float32)))
        assert np.array_equal(e, np.array([0, 0, 1 / 3, 1, 0, 0, 0, 0], dt))


@pytest.mark.parametrize("n,lam", [(1, 0.1), (257, 0.1), (4097, 0.0), (300, 3.0)])
def test_alpha_mask_restatement_against_autograd(n, lam):
    r = np.random.default_rng([5, n])
    color, gt = r.uniform(0, 1, (3, n)).astype(np.float32), r.uniform(0, 1, (3, n)).astype(np.float32)
    alpha, mask = r.uniform(0, 1, n).astype(np.float32), (r.uniform(0, 1, n) > 0.5).astype(np.float32)
    color[:, ::3] = gt[:, ::3]                          # exact ties
    color[0, 0], gt[0, 0] = -0.0, 0.0                   # -0.0 against 0.0 is a tie
    dcolor, dalpha = R.alpha_mask_grad(color, alpha, gt, mask, lam)
    c, a = torch.from_numpy(color).requires_grad_(True), torch.from_numpy(alpha).requires_grad_(True)
    (torch.abs(c - torch.from_numpy(gt)).mean() + lam * ((a - torch.from_numpy(mask)) ** 2).mean()).backward()
    assert dcolor.dtype == np.float32 and dalpha.dtype == np.float32
    assert np.array_equal(dcolor, c.grad.numpy())       # +-1 / (3 n) and exact zeros on the ties
    assert not dcolor[:, ::3].any() and not np.signbit(dcolor[:, ::3]).any()
    assert np.allclose(dalpha, a.grad.numpy(), rtol=4 * 2.0 ** -23, atol=0)
    if lam == 0.0:
        assert not dalpha.any()
    nan = color.copy()
    nan[1, n // 2] = np.nan
    assert R.alpha_mask_grad(nan, alpha, gt, mask, lam)[0][1, n // 2] == 0.0   # the three-way sign: neither > 0 nor < 0
