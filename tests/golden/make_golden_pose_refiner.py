"""Generate tests/golden/pose_refiner.npz from the IMPORTED reference Python (runs only where the reference is on disk).

Usage:  python tests/golden/make_golden_pose_refiner.py <root of the reference tree>

  nets/mlp_delta_body_pose.py: BodyPoseRefiner(total_bones=J, embedding_size=3(J-1), mlp_width=128, mlp_depth=2) -- the construction
  of scene/gaussian_model.py:95 -- at J = 24 and 55:
  * init_J{J}_*: the fresh parameters under torch.manual_seed(INIT_SEED): SHA-256 of each float32 tensor's bytes (the test compares
    bit for bit through the digest: the full tensors would not fit the size budget) and its first 16 values;
  * case_J{J}_*: the module in float64 on the CPU with its parameters made float16-representable (stored as float16: the reference
    computes on exactly those values) -- biases drawn non-zero, the last layer's rows re-scaled joint by joint so that theta of row 0
    spans 0.01 .. 3, and joint ZERO_JOINT's rows and biases zero (r = 0 exactly before the 1e-5);
    x [3, 3(J-1)] float64, a seeded upstream gradient g = dL/dRs [3, J-1, 3, 3]; for B = 3 (all rows) and B = 1 (row 0):
    Rs, dL/dx, dL/db*, and the weight gradients -- in full at B = 3; at B = 1 each weight gradient is the outer product of its bias
    gradient and the layer's input (one product per entry in the reference's autograd as well), so h1 / h2 of row 0 are stored.
The file is data, not code.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])

from nets.mlp_delta_body_pose import BodyPoseRefiner  # noqa: E402

INIT_SEED = 11
ZERO_JOINT = 5
NAMES = ("w0", "b0", "w2", "b2", "w4", "b4")


def make(J):
    return BodyPoseRefiner(total_bones=J, embedding_size=3 * (J - 1), mlp_width=128, mlp_depth=2)


def params_of(m):
    return [m.block_mlps[i].weight if k == "weight" else m.block_mlps[i].bias for i in (0, 2, 4) for k in ("weight", "bias")]


def f16(a):
    return a.astype(np.float16).astype(np.float64)


def main():
    out = {}
    for J in (24, 55):
        torch.manual_seed(INIT_SEED)
        fresh = make(J)
        for n, p in zip(NAMES, params_of(fresh)):
            a = p.detach().numpy().astype(np.float32)
            out[f"init_J{J}_{n}_sha256"] = np.array(hashlib.sha256(a.tobytes()).hexdigest())
            out[f"init_J{J}_{n}_head"] = a.reshape(-1)[:16].copy()
            out[f"init_J{J}_{n}_shape"] = np.array(a.shape, np.int64)

        nj, E = J - 1, 3 * (J - 1)
        rng = np.random.default_rng(100 + J)
        torch.manual_seed(J)
        m = make(J).double()
        x = torch.from_numpy(rng.normal(0, 0.4, (3, E)))
        with torch.no_grad():
            ps = params_of(m)
            ps[1].copy_(torch.from_numpy(f16(rng.normal(0, 0.05, 128))))
            ps[3].copy_(torch.from_numpy(f16(rng.normal(0, 0.05, 128))))
            for i in (0, 2):
                ps[i].copy_(torch.from_numpy(f16(ps[i].numpy())))
            w4 = torch.from_numpy(rng.uniform(-1, 1, (E, 128)))
            b4 = torch.from_numpy(rng.normal(0, 0.02, E))
            h2 = torch.relu(torch.relu(x[:1] @ ps[0].t() + ps[1]) @ ps[2].t() + ps[3])[0]
            targets = np.exp(rng.permutation(np.linspace(np.log(0.01), np.log(3.0), nj)))
            for j in range(nj):
                rj = (w4[3 * j:3 * j + 3] @ h2 + b4[3 * j:3 * j + 3]).norm()
                w4[3 * j:3 * j + 3] *= targets[j] / rj
                b4[3 * j:3 * j + 3] *= targets[j] / rj
            w4[3 * ZERO_JOINT:3 * ZERO_JOINT + 3] = 0.0
            b4[3 * ZERO_JOINT:3 * ZERO_JOINT + 3] = 0.0
            ps[4].copy_(torch.from_numpy(f16(w4.numpy())))
            ps[5].copy_(torch.from_numpy(f16(b4.numpy())))
        for n, p in zip(NAMES, ps):
            out[f"case_J{J}_{n}"] = p.detach().numpy().astype(np.float16)
            assert np.array_equal(out[f"case_J{J}_{n}"].astype(np.float64), p.detach().numpy())
        out[f"case_J{J}_x"] = x.numpy()
        g = torch.from_numpy(rng.normal(0, 1, (3, nj, 3, 3)))
        out[f"case_J{J}_g"] = g.numpy()

        acts = {}
        hooks = [m.block_mlps[i].register_forward_hook(lambda mod, inp, o, i=i: acts.__setitem__(i, inp[0].detach().clone()))
                 for i in (2, 4)]
        for B in (3, 1):
            m.zero_grad(set_to_none=True)
            xb = x[:B].clone().requires_grad_(True)
            Rs = m(xb)["Rs"]
            (Rs * g[:B]).sum().backward()
            tag = f"case_J{J}_B{B}"
            out[f"{tag}_Rs"] = Rs.detach().numpy()
            out[f"{tag}_dx"] = xb.grad.numpy()
            for n, p in zip(NAMES, params_of(m)):
                if n.startswith("b") or B == 3:
                    out[f"{tag}_d{n}"] = p.grad.numpy()
            if B == 1:
                out[f"{tag}_h1"] = acts[2][0].numpy()
                out[f"{tag}_h2"] = acts[4][0].numpy()
                for n, b, a in (("w0", "b0", x[0]), ("w2", "b2", acts[2][0]), ("w4", "b4", acts[4][0])):
                    assert np.array_equal(np.outer(out[f"{tag}_d{b}"], a.numpy()), params_of(m)[NAMES.index(n)].grad.numpy())
            theta = np.sqrt(1e-5 + (Rs.new_tensor(0) + (m.block_mlps(xb.detach()).view(-1, 3) ** 2).sum(1)).detach().numpy())
            print(f"J={J} B={B}: theta {theta.min():.4f} .. {theta.max():.3f}", flush=True)
        for h in hooks:
            h.remove()
    path = os.path.join(HERE, "pose_refiner.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
