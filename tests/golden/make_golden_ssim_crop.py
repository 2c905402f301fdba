"""Generate tests/golden/ssim_crop.npz (CPU, float64) from the reference's OWN utils.loss_utils.ssim, applied to the crop exactly as
train.py:269-281 writes it -- ssim(img[:, y:y+h, x:x+w].unsqueeze(0), gt[:, y:y+h, x:x+w].unsqueeze(0)):

    python tests/golden/make_golden_ssim_crop.py /path/to/reference

utils/loss_utils.py is imported with a stand-in for cv2 (utils.image_utils imports it at module top), as make_golden_pbr_loss.py does.
OpenCV is therefore NOT run: the rectangle comes from tests/ssim_crop_reference.bounding_rect_np, a numpy restatement of
cv2.boundingRect that is pinned by OpenCV's documented definition (the up-right bounding rectangle of the nonzero pixels: x and y the
smallest column and row, w and h the extents, (0, 0, 0, 0) for an empty set), not by running OpenCV.

The inputs are not stored: tests/ssim_crop_reference.case_inputs() rebuilds them bit for bit from an index hash.  Stored per case
and group: the rect, the value, and the gradient with respect to img1 INSIDE the rect ([C, h, w]; the slice takes no gradient
outside it, which the generator asserts).

Two rendering-like crops follow (tests/image_loss_cases.GOLDEN_CROPS: a flat background and a smooth shaded body, where the
variances cancel against C2), under their own names with the same three arrays; tests/test_image_loss_reference_host.py holds the
float64 restatement of tests/image_loss_reference.py to them."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import image_loss_cases as K  # noqa: E402
from tests import ssim_crop_reference as R  # noqa: E402


def import_reference(ref_root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref_root)
    from utils import loss_utils
    return loss_utils


def main(ref_root):
    lu = import_reference(ref_root)
    out = {}
    for case, (H, W, _, groups, want_rect) in R.CASES.items():
        x = R.case_inputs(case)
        rect = R.bounding_rect_np(x["mask"])
        assert rect == want_rect, (case, rect)
        out[f"{case}/rect"] = np.asarray(rect, np.int32)
        for g in range(groups):
            v, grad = R.value_and_grad(x["img1"][g], x["img2"][g], rect, lu.ssim)
            rx, ry, rw, rh = rect
            inside = grad[:, ry:ry + rh, rx:rx + rw].copy()
            grad[:, ry:ry + rh, rx:rx + rw] = 0.0
            assert not grad.any(), case
            out[f"{case}/{g}/value"] = np.float64(v)
            out[f"{case}/{g}/grad"] = inside.astype(np.float64)
    import torch
    for name, (family, H, W, planes, rect) in K.GOLDEN_CROPS.items():
        a, b = K.make(family, H, W, planes)
        rx, ry, rw, rh = rect
        assert rw <= 80 and rh <= 64 and rx >= 0 and ry >= 0 and rx + rw <= W and ry + rh <= H
        v, grad = R.value_and_grad(torch.from_numpy(a).double(), torch.from_numpy(b).double(), rect, lu.ssim)
        out[f"{name}/rect"] = np.asarray(rect, np.int32)
        out[f"{name}/value"] = np.float64(v)
        out[f"{name}/grad"] = grad[:, ry:ry + rh, rx:rx + rw].astype(np.float64)
    path = os.path.join(HERE, "ssim_crop.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "reference")
