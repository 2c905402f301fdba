"""Plain restatements of the articulated deform path for the tests: the per-point map of GaussianModel.coarse_deform_c2source
(scene/gaussian_model.py:776-872; checks csrc/lbs.hip) and the pose chain (rodrigues -> refinement product -> rigid chain -> rest
pose removed, :894-980; checks csrc/pose.hip).  Nothing here calls the package: torch and numpy only.

Every function takes a `dtype`: torch.float64 is the reference, torch.float32 (on the CPU, same code) the checker whose own
error against float64 -- e32, by the measure of util.assert_close -- sets the bound a kernel is held to (2 x e32 + 4 ulp,
check_measured / check_reduced below).

The two gradients the LBS backward REDUCES over the points are restated in two stages: autograd runs up to the per-point
quantities (g_Ap[p] = dL/d(blended pose transform of point p), g_q2[p] = dL/d(offset-corrected point p)), and the sums

    d_A_pose[j, k]  = sum_p bw[p, j] * g_Ap[p, k]            d_off_pose[v] = sum_{p: ids[p] = v} g_q2[p]

are taken here: in float64 exactly enough, in float32 one term after the other in float32 -- the least accurate order the kernel
may use (atomics in arbitrary order; a 256-term loop per workgroup, then a sum over the workgroups).  S_abs, the sum of the
absolute contributions, is the scale such a sum is accurate to; the possibly cancelled sum itself is not.
"""
import numpy as np
import torch

ULP = 2.0 ** -23
EPS_LOG = float(np.float32(1e-9))     # log(w + 1e-9f): the float32 constant, widened
EPS_ANGLE = float(np.float32(1e-8))   # |v + 1e-8f|


def _t(a, dtype, grad=False):
    """numpy (any float type) or tensor -> a fresh CPU leaf of `dtype`; None stays None."""
    if a is None:
        return None
    t = torch.as_tensor(np.asarray(a, np.float64) if not isinstance(a, torch.Tensor) else a.detach().cpu().double()).to(dtype)
    return t.clone().requires_grad_(grad)


def inv3(m):
    """Inverse of [..., 3, 3] matrices as adjugate / determinant (cofactors written out): differentiable, works on empty batches."""
    a, b, c = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    d, e, f = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    g, h, i = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = a * c00 + b * c01 + c * c02
    adj = torch.stack([torch.stack([c00, c * h - b * i, b * f - c * e], -1),
                       torch.stack([c01, a * i - c * g, c * d - a * f], -1),
                       torch.stack([c02, b * g - a * h, a * e - b * d], -1)], -2)
    return adj / det[..., None, None]


def _mv(M, v):
    return (M * v[..., None, :]).sum(-1)


def deform64(query, normals, lbs_offsets, A_big, A_pose, off_big, off_shape, off_pose, R, Th, ids, weights, bw_hook=None):
    """The per-point map, in the dtype of its (tensor) arguments, any joint count J = weights.shape[1].  `ids` [P] int64 are the
    nearest-vertex indices (an input: the only discontinuity of the map).  normals / lbs_offsets may be None.
    Returns dict(world_pts [P,3], transforms [P,3,3], world_normals [P,3] | None, smpl_pts [P,3], bweights [P,J],
    translation [P,3]) plus the two per-point stage tensors the reduced gradients go through: Ap [P,4,4] (blended pose transform)
    and offp [P,3] (the gathered off_pose rows).  bw_hook (tests of the noise floor itself): applied to the blend weights."""
    J = weights.shape[1]
    bw = weights[ids]
    if lbs_offsets is not None:
        bw = torch.softmax(torch.log(bw + torch.tensor(EPS_LOG, dtype=bw.dtype)) + lbs_offsets, dim=-1)
    if bw_hook is not None:
        bw = bw_hook(bw)
    Ab = (bw @ A_big.reshape(J, 16)).reshape(-1, 4, 4)
    Ap = (bw @ A_pose.reshape(J, 16)).reshape(-1, 4, 4)
    offp = off_pose[ids]
    Ri = inv3(Ab[:, :3, :3])
    tb = Ab[:, :3, 3]
    shift = lambda x: x - off_big[ids] + off_shape[ids] + offp  # noqa: E731
    q2 = shift(_mv(Ri, query - tb))
    tr = shift(_mv(Ri, -tb))
    Rp, tp = Ap[:, :3, :3], Ap[:, :3, 3]
    Rinv = inv3(R)
    src = _mv(Rp, q2) + tp
    out = dict(world_pts=src @ Rinv + Th, transforms=R @ (Rp @ Ri), world_normals=None, smpl_pts=src, bweights=bw,
               translation=(_mv(Rp, tr) + tp) @ Rinv + Th, Ap=Ap, offp=offp)
    if normals is not None:
        out["world_normals"] = _mv(Rp, _mv(Ri, normals)) @ Rinv
    return out


LBS_INPUTS = ("query", "normals", "loff", "A_big", "A_pose", "off_big", "off_shape", "off_pose", "R", "Th")
LBS_GRADS = ("query", "normals", "loff", "A_pose", "off_pose")
LBS_OUTPUTS = ("world_pts", "transforms", "world_normals", "smpl_pts", "bweights", "translation")
LOSS_TERMS = {"world": ("world_pts",), "transforms": ("transforms",), "normals": ("world_normals",),
              "all": ("world_pts", "transforms", "world_normals")}
UPSTREAM = {"world_pts": "g_world", "transforms": "g_transforms", "world_normals": "g_normals"}


def _sequential_sum_f32(terms, index=None, n_out=None):
    """terms [P, ...] float32 -> their sum over p taken one term after the other in float32 (index: scatter rows instead)."""
    terms = np.ascontiguousarray(terms, np.float32)
    acc = np.zeros(terms.shape[1:] if index is None else (n_out,) + terms.shape[1:], np.float32)
    for p in range(terms.shape[0]):
        if index is None:
            acc += terms[p]
        else:
            acc[index[p]] += terms[p]
    return acc


def deform_reference(c, ids, dtype, loss="all", bw_hook=None):
    """Forward and backward of one case (tests/deform_cases.py: numpy float32 arrays) in `dtype` on the CPU.  The loss is the sum
    of <output, upstream> over LOSS_TERMS[loss] (terms whose output is absent -- normals None -- are left out).
    Returns (outputs, grads, s_abs), numpy float64: grads of query / normals / loff per point by autograd, of A_pose [J,4,4] and
    off_pose [V,3] by the two-stage form; s_abs[name] = the sum of the absolute per-point contributions of those two."""
    ids_t = torch.as_tensor(np.asarray(ids, np.int64))
    leaves = {k: _t(c[k], dtype, grad=k in LBS_GRADS) for k in LBS_INPUTS}
    w = _t(c["weights"], dtype)
    o = deform64(*[leaves[k] for k in LBS_INPUTS], ids_t, w, bw_hook=bw_hook)
    total = None
    for name in LOSS_TERMS[loss]:
        if o[name] is not None:
            term = (o[name] * _t(c[UPSTREAM[name]], dtype)).sum()
            total = term if total is None else total + term
    P, J, V = leaves["query"].shape[0], w.shape[1], leaves["off_pose"].shape[0]
    n64 = lambda t: t.detach().double().numpy()  # noqa: E731
    outs = {k: (None if o[k] is None else n64(o[k])) for k in LBS_OUTPUTS}
    wanted = [leaves[k] for k in ("query", "normals", "loff") if leaves[k] is not None] + \
             [leaves["A_pose"], leaves["off_pose"], o["Ap"], o["offp"]]
    if total is not None and total.requires_grad:
        got = list(torch.autograd.grad(total, wanted, allow_unused=True))
    else:
        got = [None] * len(wanted)
    got = [torch.zeros_like(x) if g is None else g for g, x in zip(got, wanted)]
    g_offp, g_Ap = got.pop(), got.pop()
    grads = {"off_pose_autograd": n64(got.pop()), "A_pose_autograd": n64(got.pop())}   # the one-stage sums, for cross-checking
    for k in ("query", "normals", "loff"):
        if leaves[k] is not None:
            grads[k] = n64(got.pop(0))
    bw, g_Ap12 = o["bweights"].detach(), g_Ap[:, :3, :].reshape(P, 12)
    contrib = bw[:, :, None] * g_Ap12[:, None, :]                        # [P, J, 12], products in `dtype`
    s_abs = {"A_pose": np.zeros((J, 4, 4)), "off_pose": np.zeros((V, 3))}
    s_abs["A_pose"][:, :3, :] = n64(contrib).__abs__().sum(0).reshape(J, 3, 4)
    np.add.at(s_abs["off_pose"], np.asarray(ids, np.int64), np.abs(n64(g_offp)))
    dA, doff = np.zeros((J, 4, 4)), np.zeros((V, 3))
    if dtype == torch.float32:
        dA[:, :3, :] = _sequential_sum_f32(contrib.numpy()).reshape(J, 3, 4)
        doff[:] = _sequential_sum_f32(g_offp.numpy(), np.asarray(ids, np.int64), V)
    else:
        dA[:, :3, :] = n64(contrib).sum(0).reshape(J, 3, 4)
        np.add.at(doff, np.asarray(ids, np.int64), n64(g_offp))
    grads["A_pose"], grads["off_pose"] = dA, doff
    return outs, grads, s_abs


# ------------------------------------------------------------------------------------------------------------ pose chain
def rodrigues64(v):
    """Axis-angle [J,3] -> [J,3,3]: I + sin(t) K + (1 - cos(t)) K^2, t = |v + 1e-8f|, K = skew(v / t).  1 - cos(t) is taken as
    2 sin^2(t / 2): the difference itself cancels in float32 (at t = 1e-4 it is 0 instead of 5e-9, and the gradient with respect
    to v, which divides by t, loses four digits)."""
    t = torch.sqrt(((v + torch.tensor(EPS_ANGLE, dtype=v.dtype)) ** 2).sum(-1))
    d = v / t[:, None]
    z = torch.zeros_like(t)
    K = torch.stack([torch.stack([z, -d[:, 2], d[:, 1]], -1), torch.stack([d[:, 2], z, -d[:, 0]], -1),
                     torch.stack([-d[:, 1], d[:, 0], z], -1)], -2)
    eye = torch.eye(3, dtype=v.dtype)
    return eye + torch.sin(t)[:, None, None] * K + (2.0 * torch.sin(0.5 * t) ** 2)[:, None, None] * (K @ K)


def pose_chain64(poses, joints, parents, correct_Rs=None):
    """poses [J,3] (or [3J]), joints [J,3], parents (parents[i] < i for i >= 1; parents[0] is ignored), correct_Rs [J-1,3,3] or None
    -> (rot_mats [J,3,3] after the refinement product rot[1:] @ correct_Rs, A [J,4,4] with the rest pose removed), in the dtype of
    the arguments."""
    J = joints.shape[0]
    rot = rodrigues64(poses.reshape(J, 3))
    if correct_Rs is not None:
        rot = torch.cat([rot[:1], rot[1:] @ correct_Rs.reshape(J - 1, 3, 3)], 0)
    GR, Gt = [rot[0]], [joints[0]]
    for i in range(1, J):
        p = int(parents[i])
        GR.append(GR[p] @ rot[i])
        Gt.append(GR[p] @ (joints[i] - joints[p]) + Gt[p])
    GR, Gt = torch.stack(GR), torch.stack(Gt)
    t = Gt - _mv(GR, joints)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=rot.dtype).expand(J, 1, 4)
    return rot, torch.cat([torch.cat([GR, t[:, :, None]], 2), bottom], 1)


def pose_reference(c, dtype, with_correct, loss):
    """One pose case (deform_cases.pose_case) in `dtype`: outputs A, rot_mats and the gradients of poses / correct_Rs / joints under
    the loss <A, wA> (loss "A"), <rot_mats, wR> ("rot") or both ("both").  numpy float64."""
    p, j = _t(c["poses"], dtype, True), _t(c["joints"], dtype, True)
    cr = _t(c["correct_Rs"], dtype, True) if with_correct else None
    rot, A = pose_chain64(p, j, c["parents"], cr)
    total = 0.0
    if loss in ("A", "both"):
        total = total + (A * _t(c["wA"], dtype)).sum()
    if loss in ("rot", "both"):
        total = total + (rot * _t(c["wR"], dtype)).sum()
    leaves = [p, j] + ([cr] if cr is not None else [])
    g = torch.autograd.grad(total, leaves, allow_unused=True)
    g = [torch.zeros_like(x) if y is None else y for x, y in zip(leaves, g)]
    n64 = lambda t: t.detach().double().numpy()  # noqa: E731
    out = dict(A=n64(A), rot_mats=n64(rot), d_poses=n64(g[0]), d_joints=n64(g[1]))
    if cr is not None:
        out["d_correct_Rs"] = n64(g[2])
    return out


# ------------------------------------------------------------------------------------------------------------ the measure
def measure(got, want):
    """Worst element of util.assert_close's measure: |got - want| / max(|want|, scale), scale = the 99.9th percentile of |want|
    (its maximum when that is zero).  A `want` that is zero everywhere: 0 if got is too, else inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    scale = float(np.percentile(np.abs(want), 99.9)) or float(np.abs(want).max())
    if scale == 0.0:
        return 0.0 if not np.any(got) else np.inf
    return float((np.abs(got - want) / np.maximum(np.abs(want), scale)).max())


def measure_reduced(got, want, s_abs):
    """Worst |got - want| / S_abs over the elements with contributions; an element without any (S_abs = 0) must be exactly 0."""
    got, want, s_abs = (np.asarray(x, np.float64) for x in (got, want, s_abs))
    assert got.shape == want.shape == s_abs.shape, (got.shape, want.shape, s_abs.shape)
    none = s_abs == 0.0
    if np.any(got[none] != 0.0):
        return np.inf
    return float((np.abs(got - want)[~none] / s_abs[~none]).max()) if (~none).any() else 0.0


FACTOR = 2.0   # the bound is FACTOR x e32 + 4 ulp unless a test gives a tensor another factor (<= 8), with the reason next to it


def _verdict(name, e32, ek, record, factor):
    assert FACTOR <= factor <= 8.0
    tol = factor * e32 + 4.0 * ULP
    print(f"{name}: float32 checker {e32:.3e}  kernel {ek:.3e}  bound {tol:.3e}  kernel/checker {ek / e32 if e32 else float('nan'):.2f}")
    if record is not None:
        record.setdefault(name, []).append((e32, ek, tol))
    assert np.isfinite(ek), f"{name}: the kernel's result is not finite (or non-zero where nothing contributes)"
    assert ek <= tol, f"{name}: kernel {ek:.3e} > {factor:g} x {e32:.3e} + 4 ulp = {tol:.3e}"
    assert tol <= 1e-4, f"{name}: the measured bound {tol:.3e} exceeds the 1e-4 of the fixed-tolerance tests"


def check_measured(name, got, want64, ref32, record=None, factor=FACTOR):
    """The measured rule, every element compared: got within 2 x (the float32 checker's own error) + 4 ulp."""
    _verdict(name, measure(ref32, want64), measure(got, want64), record, factor)


def check_reduced(name, got, want64, ref32, s_abs, record=None, factor=FACTOR):
    """The measured rule for a gradient summed over the points: the scale of an element is its S_abs."""
    _verdict(name, measure_reduced(ref32, want64, s_abs), measure_reduced(got, want64, s_abs), record, factor)
