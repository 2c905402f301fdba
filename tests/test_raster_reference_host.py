"""The CPU oracle against an independent float64 restatement of the rasterizer (tests/raster_reference.py), under general
cameras and at the edges of projection and blending (tests/scenes.py), plus the coverage each scene family promises.

The restatement's gradients come from autograd, not from a hand-derived backward, so these tests pin the oracle's
backward -- and through it the HIP kernels -- against a derivation it does not share, at parity tolerances."""
import math
import os

import numpy as np
import pytest
import torch

from mygauhuman_amd import cameras
from tests import raster_reference as rr
from tests import scenes, util

BG = np.array([0.2, 0.5, 0.7], np.float32)
MAX_MARGIN_FRAC = 0.03
# float32 oracle vs float64, relative to each tensor's 99.9th-percentile magnitude (util.assert_close).  Needles (scale
# ratios >= 1e3) lose more in float32: their short-axis scale gradient is a difference of large terms.
TOL = {"needle": dict(dL_dscales=2e-2, dL_drotations=2e-3, dL_dmeans3D=2e-3, default=3e-4)}


def tolerance(family, name):
    t = TOL.get(family, {})
    return t.get(name, t.get("default", 1e-4))


CASES = [(f, m) for f in scenes.FAMILIES for m in ("sh", "precomp")]
IDENTITY = [(300, 80, 56, 1, 0.05, 0.1), (600, 128, 96, 2, 0.03, 0.2)]


def identity_scene(P, W, H, seed, scale, behind):
    return util.make_scene(P, W, H, seed, 3, scale, behind)


def grad_names(mode):
    return [n for n in rr.GRAD_NAMES if mode == "sh" or n not in ("dL_dsh", "dL_dscales", "dL_drotations")]


def compare_to_float64(name, got, ref64, keep, tol=1e-4, max_bad_frac=0.0, outer_tol=None):
    """Images against the restatement outside its margin mask; returns the largest error relative to the tensor scale."""
    m = np.broadcast_to(keep, ref64.shape)
    util.assert_close(name, got, ref64, tol=tol, mask=m, max_bad_frac=max_bad_frac, outer_tol=outer_tol)
    return rel_err(got, ref64, m)


def rel_err(got, want, mask=None):
    got, want = np.asarray(got, np.float64).reshape(want.shape), np.asarray(want, np.float64)
    scale = float(np.percentile(np.abs(want), 99.9)) or float(np.abs(want).max()) or 1.0
    e = np.abs(got - want) / np.maximum(np.abs(want), scale)
    if mask is not None:
        e = np.where(mask, e, 0.0)
    return float(e.max()) if e.size else 0.0


# ------------------------------------------------------------------------------------------------ coverage of the families
def check_coverage(family, cam, g, ref64, grads=None):
    """Asserts that a family exercises what it is for; returns the counts for the record."""
    W, H = cam["W"], cam["H"]
    radii = ref64["radii"]
    out = {"visible": int((radii > 0).sum()), "margin_frac": round(float(ref64["margin"].mean()), 4)}
    assert ref64["margin"].mean() < MAX_MARGIN_FRAC, (family, ref64["margin"].mean())
    if family in ("general", "general_skew"):
        vm, pm, K = cam["viewmatrix"].ravel(), cam["projmatrix"].ravel(), cam["K"]
        for i in (1, 4, 6, 9):
            assert abs(vm[i]) > 0.05 and abs(pm[i]) > 0.05, (i, vm[i], pm[i])
        assert abs(pm[8]) > 0.05 and abs(pm[9]) > 0.05
        assert np.linalg.norm(cam["campos"]) > 0.5
        assert abs(K[0, 2] - W / 2) >= 0.1 * W and abs(K[1, 2] - H / 2) >= 0.1 * H
        assert abs(K[0, 0] / K[1, 1] - 1) >= 0.05
        assert (K[0, 1] != 0) == (family == "general_skew")
        assert out["visible"] >= 200
    elif family == "frustum":
        vis = radii > 0
        for key, lim in (("txtz", ref64["limx"]), ("tytz", ref64["limy"])):
            for sign in (-1, 1):
                side = vis & (sign * ref64[key] > lim)
                out[f"{'+' if sign > 0 else '-'}{key[1]}"] = int(side.sum())
                assert side.sum() >= 5, (key, sign, side.sum())
                if grads is not None:
                    moved = np.abs(grads["dL_dmeans3D"][side]).sum(1) > 0
                    assert moved.sum() >= 5, (key, sign, moved.sum())
    elif family == "near":
        z = ref64["z"]
        big = (radii > max(W, H) / 2) & (z <= 0.6)
        out["near_big"], out["culled_near"] = int(big.sum()), int(((z < 0.2) & (radii == 0)).sum())
        assert big.sum() >= 8 and out["culled_near"] >= 8
        assert np.all(radii[z <= 0.2] == 0)
    elif family == "opaque":
        out["clamped_px"], out["terminated_px"] = round(float(ref64["clamped"].mean()), 4), round(float(ref64["terminated"].mean()), 4)
        assert ref64["clamped"].mean() >= 0.01 and ref64["terminated"].mean() >= 0.10
    elif family == "needle":
        s = g["scales"].astype(np.float64)
        out["min_ratio"] = round(float((s.max(1) / s.min(1)).min()), 1)
        assert out["min_ratio"] >= 1e3 and out["visible"] >= 200
    return out


# ------------------------------------------------------------------------------------------------------------------ tests
def test_camera_from_K_reproduces_make_camera():
    """make_camera now goes through camera_from_K: every field bit-identical to the direct construction it replaced."""
    for W, H, fov, R, T in ((64, 48, 50.0, None, None), (160, 96, 37.0, scenes._euler(0.3, -0.2, 0.1), [0.2, -0.4, 1.5])):
        got = cameras.make_camera(W, H, fov, R, T)
        Rm = np.eye(3) if R is None else np.asarray(R, np.float64)
        Tv = np.zeros(3) if T is None else np.asarray(T, np.float64)
        f = W / (2.0 * math.tan(math.radians(fov) * 0.5))
        K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], np.float32)
        view_T = cameras.world2view(Rm, Tv).T.copy()
        full = (view_T.astype(np.float32) @ cameras.projection_from_K(K, H, W).T.copy().astype(np.float32)).astype(np.float32)
        campos = np.linalg.inv(view_T.astype(np.float64))[3, :3].astype(np.float32)
        fovx, fovy = cameras.focal2fov(float(K[0, 0]), W), cameras.focal2fov(float(K[1, 1]), H)
        want = dict(W=W, H=H, K=K, viewmatrix=view_T, projmatrix=full, campos=campos, tanfovx=math.tan(fovx * 0.5),
                    tanfovy=math.tan(fovy * 0.5), FoVx=fovx, FoVy=fovy)
        assert set(got) == set(want)
        for k, v in want.items():
            if isinstance(v, np.ndarray):
                assert got[k].dtype == v.dtype
                np.testing.assert_array_equal(got[k].view(np.uint32), v.astype(got[k].dtype).view(np.uint32), err_msg=k)
            else:
                assert got[k] == v, k


def test_camera_from_K_intrinsics():
    """Skew, off-centre principal point and fx != fy reach the projection matrix where getProjectionMatrix_refine puts them:
    a camera-space point projects to the pixel K says (up to ndc2pix's half-pixel offset)."""
    W, H = 120, 90
    K = scenes.general_K(W, H, skew=True).astype(np.float64)
    cam = cameras.camera_from_K(W, H, K, scenes._euler(0.4, 0.3, -0.25), [0.3, -0.7, 1.1])
    assert cam["tanfovx"] == pytest.approx(W / (2 * K[0, 0]), rel=1e-6)
    assert cam["tanfovy"] == pytest.approx(H / (2 * K[1, 1]), rel=1e-6)
    rng = np.random.default_rng(0)
    t = np.stack([rng.uniform(-1, 1, 20), rng.uniform(-1, 1, 20), rng.uniform(2, 5, 20)], 1)
    vm = cam["viewmatrix"].astype(np.float64).reshape(4, 4)
    p = (t - vm[3, :3]) @ np.linalg.inv(vm[:3, :3])
    np.testing.assert_allclose(scenes.view_space(cam, dict(means3D=p)), t, atol=1e-9)
    pm = cam["projmatrix"].astype(np.float64).reshape(4, 4)
    ph = p @ pm[:3] + pm[3]
    pix = ((ph[:, :2] / ph[:, 3:] + 1) * [W, H] - 1) * 0.5
    want = np.stack([K[0, 0] * t[:, 0] / t[:, 2] + K[0, 1] * t[:, 1] / t[:, 2] + K[0, 2],
                     K[1, 1] * t[:, 1] / t[:, 2] + K[1, 2]], 1) - 0.5
    np.testing.assert_allclose(pix, want, atol=2e-3)
    np.testing.assert_allclose(cam["campos"], -(np.linalg.inv(vm[:3, :3]).T @ vm[3, :3]) @ np.eye(3), atol=1e-5)


def test_restatement_sh_matches_golden(golden_dir):
    """The restatement's SH polynomial == the reference's eval_sh (tests/golden/sh_eval.npz, float32 vectors)."""
    g = np.load(os.path.join(golden_dir, "sh_eval.npz"))
    sh = torch.from_numpy(g["sh"].transpose(0, 2, 1).astype(np.float64))
    d = torch.from_numpy(g["dirs"].astype(np.float64))
    for deg in range(4):
        np.testing.assert_allclose(rr.sh_eval(deg, sh, d).numpy(), g[f"rgb_deg{deg}"], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("family", scenes.FAMILIES)
def test_family_coverage(family):
    cam, g = scenes.make(family, 0)
    ref64 = rr.forward(cam, g, BG, "sh")
    check_coverage(family, cam, g, ref64)


def _oracle_vs_float64(oracle, family, cam, g, mode, seed):
    ref = util.oracle_forward(oracle, cam, g, BG, mode)
    r64 = rr.forward(cam, g, BG, mode)
    H, W = cam["H"], cam["W"]
    np.testing.assert_array_equal(ref["pre"]["radii"], r64["radii"])
    keep = ~r64["margin"] & (ref["img"]["fragile"] == 0)
    assert keep.mean() > 1 - MAX_MARGIN_FRAC
    errs = {}
    for k in ("color", "depth", "alpha"):
        errs[k] = compare_to_float64(k, ref["img"][k], r64[k], keep)
    dc, dd, da = rr.upstream(H, W, seed, keep)
    want = rr.backward(cam, g, BG, mode, dc, dd, da)
    got = oracle.rasterize_backward(ref, dc, dd, da)
    for n in grad_names(mode):
        assert np.abs(want[n]).max() > 0, n
        util.assert_close(n, got[n].reshape(want[n].shape), want[n], tol=tolerance(family, n))
        errs[n] = rel_err(got[n], want[n])
    return ref, r64, got, errs


@pytest.mark.parametrize("family,mode", CASES)
def test_oracle_matches_float64_restatement(oracle, family, mode):
    cam, g = scenes.make(family, 0)
    ref, r64, got, errs = _oracle_vs_float64(oracle, family, cam, g, mode, seed=FAMILIES_SEED[family])
    check_coverage(family, cam, g, r64, got)


@pytest.mark.parametrize("case", range(len(IDENTITY)))
@pytest.mark.parametrize("mode", ["sh", "precomp"])
def test_oracle_matches_float64_identity_camera(oracle, case, mode):
    P, W, H, seed, scale, behind = IDENTITY[case]
    cam, g = identity_scene(*IDENTITY[case])
    _oracle_vs_float64(oracle, "identity", cam, g, mode, seed)


FAMILIES_SEED = {f: i for i, f in enumerate(scenes.FAMILIES)}
