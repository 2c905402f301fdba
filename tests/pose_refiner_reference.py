"""Float64 restatement of the reference's pose-correction network (nets/mlp_delta_body_pose.py: BodyPoseRefiner with
mlp_depth = 2, then RodriguesModule) for the tests of csrc/pose_refiner.hip / mygauhuman_amd/nets_pose.py.

    h1 = relu(x W0^T + b0)   h2 = relu(h1 W2^T + b2)   r = h2 W4^T + b4             (x [B, 3(J-1)])
    per 3-vector of r: t = sqrt(1e-5 + |r|^2), n = r / t,  R = cos(t) I + (1 - cos t) n n^T + sin(t) [n]x

The rotation is written in matrix form here, not entry by entry as the reference and nets_pose.RodriguesModule write it: a second,
independent statement of the same function (tests/golden/pose_refiner.npz pins it to the reference's own code at 1e-12)."""
import torch

PARAM_NAMES = ("block_mlps.0.weight", "block_mlps.0.bias", "block_mlps.2.weight", "block_mlps.2.bias", "block_mlps.4.weight",
               "block_mlps.4.bias")


def preactivations(x, params):
    """(z1, z2, r): the two hidden pre-activations and the network output."""
    w0, b0, w2, b2, w4, b4 = params
    z1 = x @ w0.t() + b0
    z2 = torch.relu(z1) @ w2.t() + b2
    r = torch.relu(z2) @ w4.t() + b4
    return z1, z2, r


def rodrigues(rvec):
    """[N, 3] -> [N, 3, 3]."""
    theta = torch.sqrt(1e-5 + (rvec * rvec).sum(dim=1))
    n = rvec / theta[:, None]
    c, s = torch.cos(theta)[:, None, None], torch.sin(theta)[:, None, None]
    z = torch.zeros_like(n[:, 0])
    skew = torch.stack((z, -n[:, 2], n[:, 1], n[:, 2], z, -n[:, 0], -n[:, 1], n[:, 0], z), dim=1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=rvec.dtype, device=rvec.device)[None]
    return c * eye + (1.0 - c) * n[:, :, None] * n[:, None, :] + s * skew


def forward(x, params):
    """x [B, 3(J-1)], params (w0, b0, w2, b2, w4, b4) -> Rs [B, J-1, 3, 3]; differentiable (autograd gives the reference's gradients)."""
    r = preactivations(x, params)[2]
    return rodrigues(r.reshape(-1, 3)).view(x.shape[0], -1, 3, 3)
