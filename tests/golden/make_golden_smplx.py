"""Generate the SMPL-X (55-joint) golden vectors from the IMPORTED reference Python (runs only where the reference is on disk).

Usage:  python tests/golden/make_golden_smplx.py

  smplx/lbs.py: lbs, batch_rodrigues              -> lbs_smplx.npz                (a seeded SMPL-X-shaped model: V = 300, J = 55,
                                                                                    K = 486 pose-blend columns, 20 shape columns)
  nets/mlp_delta_weight_lbs.py: LBSOffsetDecoder  -> lbs_offset_decoder_55.npz    (total_bones = 55, seeded parameters, 256 points;
                                                                                    output and the parameter gradients of (out . w).sum())
The large tables (posedirs, the decoder's parameters) are drawn as float16-representable values and stored as float16: the
reference computes on exactly those values in float32, and the two files stay well under 2 MB.  The files are data, not code.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from nets.mlp_delta_weight_lbs import LBSOffsetDecoder  # noqa: E402
from smplx.lbs import batch_rodrigues, lbs  # noqa: E402

PARENTS_SMPLX = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15, 20, 25, 26, 20, 28,
                          29, 20, 31, 32, 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53], np.int64)
NJ, NS = 55, 20


def f16_exact(a):
    return a.astype(np.float16).astype(np.float32)


def synthetic_smplx(V, seed):
    rng = np.random.default_rng(seed)
    v_template = rng.uniform(-1, 1, (V, 3)).astype(np.float32) * np.array([0.45, 0.9, 0.15], np.float32)
    shapedirs = rng.normal(0, 0.01, (V, 3, NS)).astype(np.float32)
    posedirs = f16_exact(rng.normal(0, 0.001, (9 * (NJ - 1), V * 3)))   # smplx layout [K, V*3]
    J_regressor = rng.uniform(0, 1, (NJ, V)).astype(np.float32)
    J_regressor /= J_regressor.sum(1, keepdims=True)
    weights = rng.uniform(0, 1, (V, NJ)).astype(np.float32) ** 4
    weights /= weights.sum(1, keepdims=True)
    return dict(v_template=v_template, shapedirs=shapedirs, posedirs=posedirs, J_regressor=J_regressor,
                weights=weights.astype(np.float32), parents=PARENTS_SMPLX)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    rng = np.random.default_rng(55)

    # ---- smplx lbs at 55 joints
    V = 300
    m = synthetic_smplx(V, 2)
    betas = rng.normal(0, 1, (1, NS)).astype(np.float32)          # betas + expression, like the DNA-Rendering reader's `shapes`
    pose = rng.normal(0, 0.2, (1, 3 * NJ)).astype(np.float32)     # full_pose [1, 165]
    verts, Jt, A, T = lbs(torch.from_numpy(betas), torch.from_numpy(pose), torch.from_numpy(m["v_template"])[None],
                          torch.from_numpy(m["shapedirs"]), torch.from_numpy(m["posedirs"]),
                          torch.from_numpy(m["J_regressor"]), torch.from_numpy(PARENTS_SMPLX),
                          torch.from_numpy(m["weights"]))
    rot = batch_rodrigues(torch.from_numpy(pose).view(-1, 3))
    smpl = {"smpl_" + k: v for k, v in m.items()}
    smpl["smpl_posedirs"] = m["posedirs"].astype(np.float16)
    np.savez_compressed(os.path.join(HERE, "lbs_smplx.npz"), betas=betas, pose=pose, verts=verts.numpy()[0],
                        J_transformed=Jt.numpy()[0], A=A.numpy()[0], T=T.numpy()[0], rot_mats=rot.numpy(),
                        smpl_seed=np.int64(2), smpl_V=np.int64(V), **smpl)

    # ---- the skinning-offset network at 55 bones
    P = 256
    net = LBSOffsetDecoder(total_bones=NJ)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for t in net.state_dict().values():
            t.copy_(torch.from_numpy(f16_exact((torch.rand(t.shape, generator=g) * 2 - 1).numpy() / np.sqrt(max(t.shape[-2:-1] + (1,))))))
    pts = rng.uniform(-1, 1, (1, P, 3)).astype(np.float32)
    w = rng.normal(0, 1, (1, NJ, P)).astype(np.float32)
    out = net(torch.from_numpy(pts))
    (out * torch.from_numpy(w)).sum().backward()
    sd = {"param." + k: v.detach().numpy().astype(np.float16) for k, v in net.state_dict().items()}
    grads = {"grad." + k: p.grad.numpy() for k, p in net.named_parameters()}
    np.savez_compressed(os.path.join(HERE, "lbs_offset_decoder_55.npz"), pts=pts, w=w, out=out.detach().numpy(), **sd, **grads)
    print("SMPL-X golden vectors written to", HERE)


if __name__ == "__main__":
    main()
