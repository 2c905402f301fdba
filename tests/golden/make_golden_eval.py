"""Generate tests/golden/eval.npz (CPU) from the reference's OWN utils.image_utils.psnr and utils.loss_utils.ssim, applied to images
finished by the fill / clamp statements of render.py:264-311 as written there (tests/eval_reference.finish_torch), in float64 and in
float32:

    python tests/golden/make_golden_eval.py /path/to/reference

The reference's modules are imported with a stand-in for cv2 (utils.image_utils imports it at module top), as
make_golden_ssim_crop.py does.  The inputs are not stored: tests/eval_reference.case_inputs() rebuilds them bit for bit from an index
hash.  Stored per case: psnr and ssim in float64, the reference's float32 psnr and ssim, and a CRC-32 of the expected uint8 bytes
(save_image's rounding of every finished image, in tests/eval_reference.NAMES order)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import eval_reference as R  # noqa: E402


def import_reference(ref_root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref_root)
    from utils import image_utils, loss_utils
    return image_utils.psnr, loss_utils.ssim


def main(ref_root):
    psnr, ssim = import_reference(ref_root)
    out = {}
    for case in R.CASES:
        x = R.case_inputs(case)
        mask, bg = torch.from_numpy(x["mask"])[None], torch.from_numpy(x["background"])
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            imgs = {n: torch.from_numpy(a.copy()).to(dt) for n, a in x["images"].items()}
            fin = R.finish_torch(imgs, mask, bg.to(dt))
            p, s = R.metrics_torch(fin["render"], fin["gt"], ssim, psnr)
            out[f"{case}/psnr_{tag}"], out[f"{case}/ssim_{tag}"] = np.float64(p), np.float64(s)
            if tag == "f32":
                out[f"{case}/u8_crc"] = np.uint32(R.crc_of([R.quantise_torch(fin[n]).numpy() for n in R.NAMES]))
    path = os.path.join(HERE, "eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    for k in sorted(out):
        print(k, out[k])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "reference")
