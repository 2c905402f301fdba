"""The HIP rasterizer under general cameras (pitch, roll, translation, off-centre principal point, fx != fy, skew) and at the
edges of projection and blending (frustum clamp, near plane, 0.99 alpha clamp with early termination, needles): the scene
families of tests/scenes.py through the raw `_C` bindings, against the CPU oracle and against the float64 restatement of
tests/raster_reference.py (evaluated on the CPU), for the three binning back-ends and both backward reductions.  Also
mark_visible under the general cameras and render() end to end with a general camera."""
import types

import numpy as np
import pytest
import torch

from tests import raster_reference as rr
from tests import scenes, util
from tests.test_raster_reference_host import BG, CASES, MAX_MARGIN_FRAC, check_coverage, grad_names, rel_err, tolerance

pytestmark = pytest.mark.gpu

_PREP = {}


def _prepared(oracle, family, mode):
    """Oracle and float64 results of one family, computed once per module run (CPU)."""
    key = (family, mode)
    if key not in _PREP:
        cam, g = scenes.make(family, 0)
        ref = util.oracle_forward(oracle, cam, g, BG, mode)
        r64 = rr.forward(cam, g, BG, mode)
        H, W = cam["H"], cam["W"]
        keep = (ref["img"]["fragile"] == 0) & ~r64["margin"]
        assert keep.mean() > 1 - MAX_MARGIN_FRAC
        up = rr.upstream(H, W, scenes.FAMILIES.index(family), keep)
        want = oracle.rasterize_backward(ref, *up)
        want64 = rr.backward(cam, g, BG, mode, *up)
        cov = check_coverage(family, cam, g, r64, want)
        _PREP[key] = types.SimpleNamespace(cam=cam, g=g, ref=ref, r64=r64, keep=keep, up=up, want=want, want64=want64, cov=cov)
    return _PREP[key]


@pytest.fixture(params=["radix", "bucket", "bucket_tight"])
def binning(request):
    from mygauhuman_amd import _lib
    _lib.check(_lib.lib.gsr_set_binning_mode(_lib.BINNING_GLOBAL_RADIX if request.param == "radix" else _lib.BINNING_TILE_BUCKET),
               "gsr_set_binning_mode")
    util.set_tile_cull(request.param == "bucket_tight")
    yield request.param
    _lib.lib.gsr_set_binning_mode(_lib.DEFAULT_BINNING)
    util.set_tile_cull(_lib.DEFAULT_TILE_CULL)


@pytest.fixture(params=[0, 1], ids=["atomics", "deterministic"])
def deterministic(request):
    from mygauhuman_amd import _lib
    _lib.set_tuning("deterministic", request.param)
    yield request.param
    _lib.set_tuning("deterministic", 0)


@pytest.mark.parametrize("family,mode", CASES)
def test_family_against_oracle_and_float64(oracle, family, mode, binning, deterministic):
    s = _prepared(oracle, family, mode)
    cam, g, ref, r64 = s.cam, s.g, s.ref, s.r64
    W, H = cam["W"], cam["H"]
    f = util.hip_forward(cam, g, BG, mode, debug=True)
    pre, b = ref["pre"], ref["bin"]
    # ---- integer state bit-exact, per-Gaussian float state bit-exact (same operation order, no FMA contraction)
    np.testing.assert_array_equal(f["radii"].cpu().numpy(), pre["radii"])
    np.testing.assert_array_equal(f["radii"].cpu().numpy(), r64["radii"])
    assert f["R"] == b["R"]
    util.assert_lists_are_sublists(f, b, ((W + 15) // 16) * ((H + 15) // 16))
    if binning != "bucket_tight":
        np.testing.assert_array_equal(util.hip_query(f, "POINT_LIST").view(np.uint32), b["point_list"])
    vis = pre["radii"] > 0
    for q, k in (("DEPTHS", "depths"), ("MEANS2D", "means2D"), ("CONIC_OPACITY", "conic_opacity"), ("RGB", "rgb")):
        np.testing.assert_array_equal(util.hip_query(f, q)[vis], pre[k][vis], err_msg=q)
    # ---- images: oracle at 1e-4 (as test_gpu_fuzz), float64 at 1e-4 outside its margin mask
    solid = ref["img"]["fragile"] == 0
    for k in ("color", "depth", "alpha"):
        got = f[k].cpu().numpy()
        util.assert_close(k, got, ref["img"][k], mask=np.broadcast_to(solid, got.shape), max_bad_frac=1e-4)
        util.assert_close(k + " vs float64", got, r64[k], mask=np.broadcast_to(s.keep, got.shape), max_bad_frac=1e-4)
    # ---- every gradient
    got = util.hip_backward(f, *s.up, debug=True)
    for n in grad_names(mode):
        want, want64 = s.want[n], s.want64[n]
        x = got[n].reshape(want.shape)
        # needles: float32 roundings of two equally valid evaluation orders differ by what the oracle loses to float64
        t64 = tolerance(family, n)
        t32 = max(1e-4, t64 if family == "needle" else 0.0)
        util.assert_close(n, x, want, tol=t32, max_bad_frac=max(3e-4, 2.5 / want.size), outer_tol=10 * t32)
        util.assert_close(n + " vs float64", x, want64, tol=t64, max_bad_frac=max(3e-4, 2.5 / want.size), outer_tol=10 * t64)


def test_family_error_record(oracle, capsys):
    """Largest error against float64, oracle and HIP (default knobs), per family: printed for the record."""
    lines = []
    for family, mode in CASES:
        s = _prepared(oracle, family, mode)
        f = util.hip_forward(s.cam, s.g, BG, mode)
        got = util.hip_backward(f, *s.up)
        m = np.broadcast_to(s.keep, s.r64["color"].shape)
        eo = max([rel_err(s.ref["img"]["color"], s.r64["color"], m)] + [rel_err(s.want[n], s.want64[n]) for n in grad_names(mode)])
        eh = max([rel_err(f["color"].cpu().numpy(), s.r64["color"], m)] + [rel_err(got[n], s.want64[n]) for n in grad_names(mode)])
        lines.append(f"{family:13s} {mode:7s} oracle {eo:.2e} hip {eh:.2e} {s.cov}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("family", scenes.FAMILIES)
def test_mark_visible_general_cameras(oracle, family):
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    cam, g = scenes.make(family, 1)
    got = _C.mark_visible(util.to_dev(g["means3D"]), util.to_dev(cam["viewmatrix"]), util.to_dev(cam["projmatrix"]))
    want = oracle.mark_visible(g["means3D"], cam["viewmatrix"], cam["projmatrix"])
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if family == "near":
        assert 0 < want.sum() < len(want)


def test_render_general_camera_matches_oracle_composition(oracle):
    """render() with a pitched, rolled, translated camera with an off-centre principal point and fx != fy, against the oracle
    composition of test_gpu_render (fused 18-channel blend, campos in the attribute kernel, fused phase-1 loss inputs)."""
    from mygauhuman_amd import cameras
    from mygauhuman_amd.gaussian_renderer import render
    from tests.test_gpu_render import _human_scene, _oracle_render
    s = _human_scene(oracle)
    W, H = s.cam_np["W"], s.cam_np["H"]
    K = scenes.general_K(W, H).astype(np.float64)
    K[0, 2], K[1, 2] = 0.42 * W, 0.60 * H  # the body stays in view
    eye = np.array([0.9, -0.8, -2.4])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    Rc2w = np.stack([right, down, fwd], 1) @ scenes._euler(0.0, 0.0, 0.3)  # + 17 degrees of roll
    cam_np = cameras.camera_from_K(W, H, K, Rc2w, -Rc2w.T @ eye)
    vm, pm = cam_np["viewmatrix"].ravel(), cam_np["projmatrix"].ravel()
    assert min(abs(vm[i]) for i in (1, 4, 6, 9)) > 0.05 and min(abs(pm[i]) for i in (1, 4, 6, 9)) > 0.05
    c = s.cam
    s.cam = cameras.ViewCamera(cam_np, "cuda", c.smpl_param, c.big_pose_smpl_param, c.big_pose_world_vertex)
    s.cam_np = cam_np
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    out = render(1, s.cam, s.model, pipe, util.to_dev(bg))
    ref, _ = _oracle_render(oracle, s, bg)
    assert float((ref["pre"]["radii"] > 0).mean()) > 0.9
    assert float((out["radii"].cpu().numpy() == ref["pre"]["radii"]).mean()) > 0.995
    diff = np.abs(out["render"].detach().cpu().numpy() - ref["img"]["color"])
    assert np.percentile(diff, 99.9) < 2e-3 and diff.mean() < 5e-5, (diff.max(), diff.mean())
    adiff = np.abs(out["render_alpha"].detach().cpu().numpy() - ref["img"]["alpha"])
    assert np.percentile(adiff, 99.9) < 2e-3 and adiff.mean() < 5e-5
    ddiff = np.abs(out["render_depth"].detach().cpu().numpy() - ref["img"]["depth"])
    assert np.percentile(ddiff, 99.9) < 1e-2 and ddiff.mean() < 2e-4
    loss = sum(out[k].mean() for k in ("render", "normal", "albedo", "world_normal")) + out["render_alpha"].mean()
    loss.backward()
    for name, p in zip(("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity"), s.model.parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, name
