"""Generate tests/golden/pbr_loss.npz (CPU, float64) from the reference's OWN loss code, so that the PBR-phase loss terms are pinned by
the reference, not by our restatement of it:

    python tests/golden/make_golden_pbr_loss.py /path/to/reference

  * gaussian_histogram, gaussian_entropy and get_masked_tv_loss are taken out of train.py with `ast` (train.py builds an LPIPS
    network at import, so it cannot be imported) and executed with numpy and torch in their namespace;
  * get_albedo_smooth_loss / get_roughness_smooth_loss come from utils/loss_utils.py, imported with a stand-in for cv2
    (utils.image_utils imports it at module top);
  * the L1 (train.py:316) and the roughness prior (:344) one-liners are evaluated here as written.
Each term is differentiated on its own.  The inputs are not stored: tests/pbr_loss_reference.py case_inputs() rebuilds them bit
for bit from an index hash; what is stored is every term's value and its gradient with respect to each input."""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import pbr_loss_reference as R  # noqa: E402

TRAIN_FUNCS = ("gaussian_histogram", "gaussian_entropy", "get_masked_tv_loss")


def import_reference(ref_root):
    src = open(os.path.join(ref_root, "train.py")).read()
    tree = ast.parse(src)
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in TRAIN_FUNCS]
    assert sorted(n.name for n in picked) == sorted(TRAIN_FUNCS), [n.name for n in picked]
    ns = {"np": np, "torch": torch}
    exec("from typing import Dict, List, Optional, Tuple, Union", ns)
    exec(compile(ast.Module(body=picked, type_ignores=[]), "train.py", "exec"), ns)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref_root)
    from utils import loss_utils
    return types.SimpleNamespace(**{k: ns[k] for k in TRAIN_FUNCS}, loss_utils=loss_utils)


def reference_terms(ref):
    lu = ref.loss_utils

    def terms(x):
        rgb, gt, bound, alpha = x["rgb"], x["gt"], x["bound"], x["alpha"]
        albedo, roughness, knn = x["albedo"], x["roughness"], x["knn"]
        out = dict(l1=lu.l1_loss(rgb.permute(1, 2, 0)[bound[0] == 1], gt.permute(1, 2, 0)[bound[0] == 1]),
                   tv=ref.get_masked_tv_loss(alpha, torch.cat([albedo, roughness], dim=0)),
                   entropy_albedo=ref.gaussian_entropy(albedo), entropy_roughness=ref.gaussian_entropy(roughness),
                   prior=(1.0 - roughness[alpha > 0]).mean())
        ga, gr = x["albedo_g"], x["roughness_g"]
        out["smooth_albedo"] = lu.get_albedo_smooth_loss(ga[knn][:, 1], ga[knn][:, 2])
        out["smooth_roughness"] = lu.get_roughness_smooth_loss(gr[knn][:, 1], gr[knn][:, 2])
        for k, v in out.items():  # (a term that is a constant of the inputs, e.g. both entropy branches untaken)
            if not isinstance(v, torch.Tensor):
                out[k] = torch.tensor(float(v), dtype=torch.float64)
        return out
    return terms


def main(ref_root):
    ref = import_reference(ref_root)
    fn = reference_terms(ref)
    out = {}
    for case in R.CASES:
        vals, grads = R.terms_and_grads(R.case_inputs(case), fn)
        for name, v in vals.items():
            out[f"{case}/{name}"] = np.float64(v)
            for inp, g in grads[name].items():
                if np.any(g != 0) or np.isnan(g).any():
                    out[f"{case}/{name}/d_{inp}"] = g.astype(np.float64)
    # W < 3: the reference raises (IndexError) where the fused path raises ValueError
    try:
        ref.gaussian_entropy(torch.rand(3, 4, 2, dtype=torch.float64))
        out["w_lt_3_raises"] = np.int64(0)
    except IndexError:
        out["w_lt_3_raises"] = np.int64(1)
    path = os.path.join(HERE, "pbr_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "reference")
