"""Inputs and float64 checkers shared by the attribute / activation tests (test_gpu_attributes_f64.py on the GPU,
test_attributes_inputs_host.py without one): seeded float32 inputs, the torch chain of tests/torch_reference.py on the CPU in
float64 and float32, the error measure of util.assert_close, and the margins of the three non-differentiable selections.

The bound every comparison uses is MEASURED, not chosen: for each tensor the float32 CPU evaluation of the same torch chain is
compared with the float64 one (that is the checker's own arithmetic, e32); the kernel has to stay within 2 x e32 (another
summation order, fused multiply-adds) plus a floor of 4 float32 ulps of the tensor's scale.
"""
import functools

import numpy as np
import torch

from tests import util

ULP = 2.0 ** -23
P_LIST = (1, 63, 64, 65, 255, 256, 257, 513)
# (layout, M, degree): "one" = shs as one [P,M,3] tensor, "pair" = (features_dc, features_rest), "misaligned" = one contiguous
# tensor whose data_ptr is 4 bytes past a 16-byte boundary (forces the per-row, non-staged forward and backward)
GROUPS = (("one", 16, 3), ("one", 16, 2), ("one", 16, 0), ("pair", 16, 3), ("pair", 16, 2), ("pair", 16, 0),
          ("one", 9, 2), ("one", 9, 1), ("one", 4, 1), ("one", 1, 0), ("one", 0, 0), ("misaligned", 16, 3))
CASES = [(P,) + g for g in GROUPS for P in P_LIST]
MOD = 1.3

# A Gaussian is left out of the comparisons that depend on a selection when float32 and float64 could select differently:
#   scales  relative gap between the two smallest scales (the inputs are the same numbers in both precisions, so only an exact tie
#           can differ; exact ties stay with the `equal` case of test_gpu_attributes.py)
#   flip    |axis . dir| -- both are unit vectors, the float32 dot product is off by a few 1e-7
#   clamp   |colour + 0.5| per channel -- a sum of at most 16 terms of magnitude <= ~1, off by a few 1e-7 in float32
# 1e-5 is thirty times those errors and still rare: about 1e-5 of the Gaussians per selection.
MARGIN = 1e-5
MAX_EXCLUDED_FRAC = 0.005

# seeds for which the float64 reference alone keeps the excluded fraction within the cap (test_attributes_inputs_host.py asserts
# it); a case that needs another seed than the default gets an entry here
SEED_OVERRIDES = {}


def seed_of(P, layout, M, deg):
    key = (P, layout, M, deg)
    return SEED_OVERRIDES.get(key, 1000 * P + 100 * GROUPS.index((layout, M, deg)) + 7)


def make_inputs(P, M, seed):
    """float32 numpy arrays: the inputs of frame_attributes, camera, and the N(0,1) upstream gradients (covariance x 1e4)."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    d = dict(means3D=f(rng.uniform(-1, 1, (P, 3))), transforms=f(rng.normal(0, 1, (P, 3, 3)) * 0.3 + np.eye(3)),
             world_normals=f(rng.normal(0, 1, (P, 3))), scales=f(np.exp(rng.normal(-4, 0.5, (P, 3)))),
             rot_cov=f(rng.normal(0, 1, (P, 4))), rot_axis=f(rng.normal(0, 1, (P, 4))), albedo=f(rng.uniform(0, 1, (P, 3))),
             roughness=f(rng.uniform(0, 1, (P, 3))), occlusion=f(rng.uniform(0, 1, (P, 3))))
    if M:
        d["shs"] = f(np.concatenate([rng.normal(0, 1, (P, 1, 3)), rng.normal(0, 0.3, (P, M - 1, 3))], 1))
    cam = np.array([0.3, -0.2, -3.0], np.float32)
    view = f(np.linalg.qr(rng.normal(0, 1, (4, 4)))[0])
    ups = dict(cov=f(rng.normal(0, 1, (P, 6)) * 1e4), colors=f(rng.normal(0, 1, (P, 3))), features=f(rng.normal(0, 1, (P, 18))))
    return d, cam, view, ups


def chain_cpu(d, cam, view, ups, deg, dtype):
    """frame_attributes_torch on the CPU in `dtype`: (outputs, input gradients) as float64 numpy arrays."""
    from tests.torch_reference import frame_attributes_torch
    t = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    leaf = {k: t(v).requires_grad_(True) for k, v in d.items()}
    cov, col, feat = frame_attributes_torch(leaf["means3D"], leaf["transforms"], leaf["world_normals"], leaf["scales"], MOD,
                                            leaf["rot_cov"], leaf["rot_axis"], leaf["albedo"], leaf["roughness"], leaf["occlusion"],
                                            leaf.get("shs"), deg, t(cam), t(view))
    loss = (cov * t(ups["cov"])).sum() + (feat * t(ups["features"])).sum()
    if col is not None:
        loss = loss + (col * t(ups["colors"])).sum()
    loss.backward()
    outs = dict(cov3D=cov, features=feat)
    if col is not None:
        outs["colors"] = col
    n64 = lambda x: x.detach().to(torch.float64).numpy()  # noqa: E731
    # (an input the chain does not depend on differentiably -- means3D at degree 0 -- has no gradient in autograd: zeros)
    return {k: n64(v) for k, v in outs.items()}, {k: n64(torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaf.items()}


def selection_margins(d, cam, deg):
    """Per-Gaussian float64 margins of the three selections: dict(scales [P], flip [P], clamp [P]) (clamp: the smallest of the
    three channels; +inf without SH coefficients)."""
    from mygauhuman_amd import covariance
    from mygauhuman_amd.sh_utils import eval_sh
    t = lambda a: torch.from_numpy(a).to(torch.float64)  # noqa: E731
    s = np.sort(d["scales"].astype(np.float64), axis=1)
    gap = (s[:, 1] - s[:, 0]) / s[:, 1]
    dirs = t(d["means3D"]) - t(cam).reshape(1, 3)
    dirn = dirs / dirs.norm(dim=1, keepdim=True)
    q = t(d["rot_axis"])
    axis = covariance.get_minimum_axis(t(d["scales"]), q / q.norm(dim=1, keepdim=True))
    flip = (axis * dirn).sum(1).abs().numpy()
    clamp = np.full(len(gap), np.inf)
    if "shs" in d:
        clamp = (eval_sh(deg, t(d["shs"]).transpose(1, 2), dirn) + 0.5).abs().min(dim=1).values.numpy()
    return dict(scales=gap, flip=flip, clamp=clamp)


def excluded_rows(d, cam, deg):
    """(axis rows, colour rows): boolean [P] masks of the Gaussians below MARGIN.  The axis selection (argsort, flip) touches the
    axis feature and the gradients of rot_axis / transforms / means3D through it; the clamp touches colours and the SH gradients."""
    m = selection_margins(d, cam, deg)
    return (m["scales"] < MARGIN) | (m["flip"] < MARGIN), m["clamp"] < MARGIN


@functools.lru_cache(maxsize=None)
def reference(P, layout, M, deg):
    """Computed once per case and shared: inputs, float64 and float32 CPU results, exclusion mask.  Callers must not write to it."""
    d, cam, view, ups = make_inputs(P, M, seed_of(P, layout, M, deg))
    out64, grad64 = chain_cpu(d, cam, view, ups, deg, torch.float64)
    out32, grad32 = chain_cpu(d, cam, view, ups, deg, torch.float32)
    ax, cl = excluded_rows(d, cam, deg)
    return dict(d=d, cam=cam, view=view, ups=ups, out64=out64, grad64=grad64, out32=out32, grad32=grad32, excluded=ax | cl)


def measure(got, want, keep_rows=None):
    """The worst element of util.assert_close's measure: |got - want| / max(|want|, scale), scale = the 99.9th percentile of
    |want| (its maximum when that is zero).  keep_rows: boolean over the leading dimension, False = not compared."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    scale = float(np.percentile(np.abs(want), 99.9)) or float(np.abs(want).max())
    if scale == 0.0:
        return 0.0 if not np.any(got) else np.inf
    err = np.abs(got - want) / np.maximum(np.abs(want), scale)
    if keep_rows is not None:
        err = err[keep_rows]
    return float(err.max()) if err.size else 0.0


def check_measured(name, got, want64, ref32, keep_rows=None, ratios=None):
    """The measured rule: got within 2 x (float32 checker's own error) + 4 ulps, by util.assert_close's measure.  Prints the
    figures, records got's ratio to the bound's float32 term in `ratios`, then asserts."""
    e32 = measure(ref32, want64, keep_rows)
    ek = measure(got, want64, keep_rows)
    tol = 2.0 * e32 + 4.0 * ULP
    print(f"{name}: float32 checker {e32:.3e}  kernel {ek:.3e}  bound {tol:.3e}  kernel/checker {ek / e32 if e32 else float('nan'):.2f}")
    if ratios is not None:
        ratios.setdefault(name, []).append((ek, e32))
    mask = None
    if keep_rows is not None:
        mask = np.broadcast_to(np.asarray(keep_rows).reshape((-1,) + (1,) * (np.ndim(want64) - 1)), np.shape(want64))
    util.assert_close(name, got, want64, tol=tol, mask=mask, max_bad_frac=0.0, outer_tol=tol)
