"""Seeded (img1, img2) pairs for the image-loss tests: [planes, H, W] float32 each, img1 the rendering, img2 the target.

    noise          a uniform target, rendering = target + 0.2 N(0, 1) clamped to [0, 1]: what the suite drew before these families
    render_white   a flat white background, a smooth shaded blob; rendering = target + 1 % noise INSIDE the blob only, so the flat
    render_black   region is bit-identical in both images (there sg = E[x^2] - mu^2 cancels against C2 = 9e-4)
    identical      rendering == target (noise)
    const0, const1 both images all 0 / all 1
    low_contrast   variance about C2: 0.5 + 0.03 N(0, 1), rendering = target + 0.01 N(0, 1)
    half_and_half  the columns [0, W // 2) of `noise`, the columns [W // 2, W) of `render_white` (same shape, same seed): a flat region
                   must not loosen the bound of a textured one
    impulse        a single 1 at (2, W - 3) on zeros against half of it: the footprint, the padding, an x / y swap on a non-square image
    out_of_range   `noise` x 8 - 4: values beyond [0, 1] and negatives, as a normal or HDR image may hold them"""
import numpy as np

FAMILIES = ("noise", "render_white", "render_black", "identical", "const0", "const1", "low_contrast", "half_and_half", "impulse",
            "out_of_range")
# H x W from {1, 5, 6, 11, 15, 16, 17, 32, 33, 47}: below the window radius, on it, on the tile and one past it, non-square
SHAPES = ((1, 17), (5, 33), (6, 11), (11, 5), (15, 16), (16, 32), (17, 33), (32, 47), (33, 15), (47, 1), (47, 33))
PLANES = (1, 3, 4)


def planes_of(shape):
    """Every shape with one of the plane counts, in turn."""
    return PLANES[SHAPES.index(tuple(shape)) % len(PLANES)]


def _rng(family, H, W, planes):
    return np.random.default_rng([FAMILIES.index(family), H, W, planes])


def _noise(H, W, planes):
    r = _rng("noise", H, W, planes)
    b = r.uniform(0.0, 1.0, (planes, H, W))
    a = np.clip(b + 0.2 * r.standard_normal((planes, H, W)), 0.0, 1.0)
    return a, b


def _render(family, H, W, planes, background):
    r = _rng(family, H, W, planes)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx, ry, rx = (H - 1) / 2.0, (W - 1) / 2.0, max(0.36 * H, 0.6), max(0.3 * W, 0.6)
    q = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2
    blob = q <= 1.0
    b = np.empty((planes, H, W))
    for p in range(planes):   # a Lambert-like falloff towards the rim, a different tint and light direction per plane
        shade = (0.25 + 0.15 * p / planes) + (0.6 - 0.1 * p / planes) * np.sqrt(np.clip(1.0 - q, 0.0, 1.0)) \
            * (0.75 + 0.25 * np.cos(0.35 * x + 0.2 * y + p))
        b[p] = np.where(blob, shade, background)
    b = b.astype(np.float32).astype(np.float64)
    a = np.where(blob[None], b + 0.01 * r.standard_normal((planes, H, W)), b)
    return a, b


def make(family, H, W, planes):
    if family == "noise":
        a, b = _noise(H, W, planes)
    elif family == "render_white":
        a, b = _render(family, H, W, planes, 1.0)
    elif family == "render_black":
        a, b = _render(family, H, W, planes, 0.0)
    elif family == "identical":
        a = b = _rng(family, H, W, planes).uniform(0.0, 1.0, (planes, H, W))
    elif family in ("const0", "const1"):
        a = b = np.full((planes, H, W), float(family[-1]))
    elif family == "low_contrast":
        r = _rng(family, H, W, planes)
        b = 0.5 + 0.03 * r.standard_normal((planes, H, W))
        a = b + 0.01 * r.standard_normal((planes, H, W))
    elif family == "half_and_half":
        (a, b), (ar, br) = _noise(H, W, planes), _render("render_white", H, W, planes, 1.0)
        a, b = a.copy(), b.copy()
        a[:, :, W // 2:], b[:, :, W // 2:] = ar[:, :, W // 2:], br[:, :, W // 2:]
    elif family == "impulse":
        a = np.zeros((planes, H, W))
        a[:, min(2, H - 1), max(W - 3, 0)] = 1.0
        b = 0.5 * a
    elif family == "out_of_range":
        a, b = _noise(H, W, planes)
        a, b = 8.0 * a - 4.0, 8.0 * b - 4.0
    else:
        raise KeyError(family)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def upstream_map(H, W, planes, seed=0):
    """A non-uniform dL/dmap: noise x a 0 / 1 mask (about a third of the pixels get no gradient at all), float32."""
    r = np.random.default_rng([977, H, W, planes, seed])
    g = r.standard_normal((planes, H, W)) * (r.uniform(0.0, 1.0, (planes, H, W)) > 0.35)
    return np.ascontiguousarray(g / (planes * H * W), np.float32)


# the two rendering-like crops of tests/golden/ssim_crop.npz (made by the reference's own ssim() in float64):
#   name: (family, H, W, planes, rect (x, y, w, h))
GOLDEN_CROPS = {
    "render_white_interior": ("render_white", 64, 80, 3, (9, 7, 40, 33)),
    "render_black_tile_edges": ("render_black", 64, 80, 3, (5, 3, 43, 45)),   # right and bottom edges at 48 = 3 x 16
}
