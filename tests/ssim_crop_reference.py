"""Inputs and host-side restatements for the crop SSIM (mygauhuman_amd.loss_utils.bounding_rect / ssim_crop, csrc/ssim_crop.hip).

    bounding_rect_np(mask)   cv2.boundingRect restated with numpy from OpenCV's documented definition (the up-right rectangle of
                             the nonzero pixels: x, y = smallest column and row, w = largest column - x + 1, h likewise; an empty
                             set gives (0, 0, 0, 0)).  OpenCV itself is not run anywhere in this repository.
    case_inputs(name)        the masks and image pairs of the fixture cases, rebuilt bit for bit from an index hash
                             (tests/golden/make_golden_ssim_crop.py stores only the reference's outputs)
    crop_ssim(...)           train.py:269-281 with tests/torch_reference.ssim_torch in place of the reference's ssim()"""
import numpy as np
import torch

from tests.pbr_reference import _u01
from tests.torch_reference import ssim_torch


def bounding_rect_np(mask):
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return (0, 0, 0, 0)
    x, y = int(xs.min()), int(ys.min())
    return (x, y, int(xs.max()) - x + 1, int(ys.max()) - y + 1)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _box(H, W, x, y, w, h):
    m = np.zeros((H, W), np.float64)
    m[y:y + h, x:x + w] = 1.0
    return m


def _holes(H, W, salt):
    """A blob with holes punched into it, and four stray single pixels further out that set the box on every side."""
    m = _box(H, W, 30, 25, 50, 40)
    m[_u01((H, W), salt) < 0.3] = 0.0
    m[7, 61] = m[88, 44] = m[51, 13] = m[33, 117] = 1.0
    return m


# name: (H, W, mask builder, number of groups, expected rect (x, y, w, h))
CASES = {
    "interior": (100, 130, lambda H, W: _box(H, W, 17, 9, 41, 33), 1, (17, 9, 41, 33)),
    "full_frame": (48, 70, lambda H, W: np.pad(np.zeros((H - 2, W - 2)), 1, constant_values=1.0), 1, (0, 0, 70, 48)),
    "corner": (100, 130, lambda H, W: _box(H, W, W - 37, H - 29, 37, 29), 1, (93, 71, 37, 29)),
    "one_pixel": (100, 130, lambda H, W: _box(H, W, 50, 40, 1, 1), 1, (50, 40, 1, 1)),
    "sliver_11x200": (210, 40, lambda H, W: _box(H, W, 6, 5, 11, 200), 1, (6, 5, 11, 200)),
    "sliver_200x3": (20, 210, lambda H, W: _box(H, W, 7, 9, 200, 3), 1, (7, 9, 200, 3)),
    "holes": (100, 130, lambda H, W: _holes(H, W, 77), 1, (13, 7, 105, 82)),
    "two_groups": (100, 130, lambda H, W: _box(H, W, 21, 35, 67, 45), 2, (21, 35, 67, 45)),
}
PLANES = 3


def case_inputs(name):
    """dict(mask [H, W] float64 of 0 / 1, img1 / img2: lists (one entry per group) of [3, H, W] float64 tensors holding float32
    values; img1 is img2 plus noise, clamped to [0, 1], as a rendering is to its target)."""
    H, W, build, groups, _ = CASES[name]
    salt = 100 * (1 + list(CASES).index(name))
    img1, img2 = [], []
    for g in range(groups):
        b = _f32(_u01((PLANES, H, W), salt + 10 * g + 1))
        a = _f32(np.clip(b + 0.4 * (_u01((PLANES, H, W), salt + 10 * g + 2) - 0.5), 0.0, 1.0))
        img1.append(torch.from_numpy(a))
        img2.append(torch.from_numpy(b))
    return dict(mask=build(H, W), img1=img1, img2=img2)


def crop_ssim(img1, img2, rect, ssim=ssim_torch):
    """ssim(img1[:, y:y+h, x:x+w][None], img2[:, y:y+h, x:x+w][None]) as train.py:270-274 writes it."""
    x, y, w, h = (int(v) for v in rect)
    return ssim(img1[:, y:y + h, x:x + w].unsqueeze(0), img2[:, y:y + h, x:x + w].unsqueeze(0))


def value_and_grad(img1, img2, rect, ssim=ssim_torch):
    """(value, d value / d img1 as a full [C, H, W] array) in the dtype of the inputs."""
    a = img1.detach().clone().requires_grad_(True)
    v = crop_ssim(a, img2, rect, ssim)
    v.backward()
    return float(v.detach()), a.grad.numpy()
