"""Where the gradients of the per-frame attribute stage end up (attributes.py, activations.py, gradlink.py, the rasterizer's
position parking): aliased / detached / viewed / cloned albedo and roughness on frame_attributes itself, and frozen branches,
two cameras, repeated backward, partial losses, the rasterizer's own covariance / SH path, cached transforms and a foreign
`extra` inside a gradlink.frame_link().

Direct cases: every leaf gradient against the float64 CPU chain, measured rule of tests/attributes_cases.py.
Hand-built frames (frame_activations + frame_attributes + forward_multi): against the float64 chain fed with the rasterizer's
own input gradients (taken from a run in which the rasterizer reads separate leaves), bound = the measured rule + 1e-5 for the
run-to-run noise of the blend backward's float atomics; and against the same frame with the link off at that 1e-5.
render() cases and the foreign-extra frame: against the float64 chain (test_gpu_render._chain64 with the case's frozen or
overridden inputs; the float64 activations) applied to the gradients the rasterizer returned for its own inputs in the very run
under test -- recorded at the binding -- under the same bound, and against the same case with the link off at 1e-5.  (The
rasterizer's own backward has its oracle comparison in test_gpu_rasterizer.py and test_gpu_render.py; what is checked here is
where its gradients, and the attribute stage's, end up.)
After every linked frame nothing stays parked.
"""
import types

import numpy as np
import pytest
import torch

from tests import attributes_cases as ac
from tests import util
from tests.test_gpu_render import _human_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"
NOISE = 1e-5   # link on vs off: the measure of test_gradients_joined_in_kernel_equal_autograd_accumulation


# ------------------------------------------------------------------------------------------ directly on frame_attributes
def _wire(case, a, x):
    """(albedo, roughness) arguments of the five cases from the leaves a (and x)."""
    if case == "same_object":
        return a, a
    if case == "roughness_detached":
        return a, a.detach()
    if case == "albedo_detached":
        return x.detach(), x
    if case == "view":
        return a, a.view_as(a)
    if case == "clone":
        return a, a.clone()
    raise ValueError(case)


def _direct(fn, case, r, dtype, dev):
    t = lambda v: torch.from_numpy(v).to(dev).to(dtype)  # noqa: E731
    leaf = {k: t(v).requires_grad_(True) for k, v in r["d"].items() if k != "roughness"}
    a = leaf.pop("albedo")
    alb, rough = _wire(case, a, a)
    cov, col, feat = fn(leaf["means3D"], leaf["transforms"], leaf["world_normals"], leaf["scales"], ac.MOD, leaf["rot_cov"],
                        leaf["rot_axis"], alb, rough, leaf["occlusion"], leaf["shs"], 3, t(r["cam"]), t(r["view"]))
    ((cov * t(r["ups"]["cov"])).sum() + (col * t(r["ups"]["colors"])).sum() + (feat * t(r["ups"]["features"])).sum()).backward()
    leaf["albedo"] = a
    return {k: (None if v.grad is None else v.grad.detach().cpu().to(torch.float64).numpy()) for k, v in leaf.items()}


@pytest.mark.parametrize("case", ["same_object", "roughness_detached", "albedo_detached", "view", "clone"])
def test_albedo_and_roughness_gradients_follow_autograd(case):
    """One storage is not one autograd variable: only the same tensor object passed twice (both uses wanting a gradient) gets the
    single summed write; a detached, viewed or cloned partner gets exactly what autograd gives the torch chain."""
    from mygauhuman_amd.attributes import frame_attributes
    from tests.torch_reference import frame_attributes_torch
    P = 300
    d, cam, view, ups = ac.make_inputs(P, 16, 4242)
    r = dict(d=d, cam=cam, view=view, ups=ups)
    want = _direct(frame_attributes_torch, case, r, torch.float64, "cpu")
    ref32 = _direct(frame_attributes_torch, case, r, torch.float32, "cpu")
    got = _direct(frame_attributes, case, r, torch.float32, DEV)
    ax, cl = ac.excluded_rows(d, cam, 3)
    keep = ~(ax | cl)
    g_alb = ups["features"][:, 6:9].astype(np.float64)
    g_rough = np.repeat(ups["features"][:, 12:15].astype(np.float64).sum(1, keepdims=True) / 3.0, 3, axis=1)
    term = {"same_object": g_alb + g_rough, "roughness_detached": g_alb, "albedo_detached": g_rough, "view": g_alb + g_rough,
            "clone": g_alb + g_rough}[case]
    assert got["albedo"] is not None, "the leaf behind albedo / roughness received no gradient"
    np.testing.assert_allclose(want["albedo"], term, rtol=1e-12, atol=1e-12)
    for k in want:
        assert got[k] is not None, k
        ac.check_measured(f"{case}: d_{k}", got[k], want[k], ref32[k], keep)


# ------------------------------------------------------------------------------------------ hand-built frames in a frame_link
@pytest.fixture()
def links(monkeypatch):
    from mygauhuman_amd import gradlink
    made, real = [], gradlink.FrameLink

    class Spy(real):
        __slots__ = ()

        def __init__(self):
            super().__init__()
            made.append(self)
    monkeypatch.setattr(gradlink, "FrameLink", Spy)
    return made


RASTER_GRADS = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "extra")


@pytest.fixture()
def raster_calls(monkeypatch):
    """Records every call of the rasterizer's backward binding: the camera position it was given, which of the six feature-image
    gradients arrived as None, and the gradients it returned for its own inputs (what the attribute stage is handed)."""
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    calls, real = [], _C.rasterize_gaussians_backward

    def spy(*a, **kw):
        out = real(*a, **kw)
        n = lambda t: None if t is None else t.detach().cpu().to(torch.float64).numpy()  # noqa: E731
        feats = kw.get("dL_dout_extra")
        calls.append(dict(campos=n(a[17]), feature_grad_is_none=None if feats is None else [g is None for g in feats],
                          grads={k: n(o) for k, o in zip(RASTER_GRADS, out)}))
        return out
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", spy)
    return calls


def _check_against_chain(what, got, want, ref32):
    """Leaf gradients against the float64 chain: the measured rule (2 x the float32 chain's own error + 4 ulps) plus the 1e-5 noise
    term of the blend backward's atomics.  A leaf the chain does not reach (None) must have no or an all-zero gradient."""
    for k in want:
        if want[k] is None:
            assert got[k] is None or not got[k].any(), f"{what}: d_{k} must be absent or zero"
            continue
        assert got[k] is not None and np.isfinite(got[k]).all(), f"{what}: d_{k}"
        e32 = ac.measure(ref32[k], want[k])
        tol = 2 * e32 + 4 * ac.ULP + NOISE
        print(f"{what}: d_{k}: float32 chain {e32:.3e}  hip {ac.measure(got[k].reshape(want[k].shape), want[k]):.3e}  bound {tol:.3e}")
        util.assert_close(f"{what}: d_{k} vs float64 chain", got[k].reshape(want[k].shape), want[k], tol=tol, max_bad_frac=0.0, outer_tol=tol)


def _nothing_parked(links, n):
    assert len(links) == n, (len(links), n)
    for link in links:
        assert link.means_grad is None and link.rot_grad is None, "a gradient stayed parked: nobody consumed it"


P_FRAME, W_FRAME, H_FRAME = 600, 64, 48
LEAVES = ("xyz", "opacity", "albedo", "scaling", "rotation", "normal", "shs")


def _frame_inputs(seed=9):
    cam, g = util.make_scene(P_FRAME, W_FRAME, H_FRAME, seed, 3, 0.05)
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    op = np.clip(g["opacities"].astype(np.float64), 1e-3, 1 - 1e-3)
    raw = dict(xyz=f(g["means3D"]), opacity=f(np.log(op / (1 - op))), albedo=f(rng.normal(0, 1, (P_FRAME, 3))),
               scaling=f(np.log(g["scales"])), rotation=f(rng.normal(0, 1, (P_FRAME, 4))), normal=f(rng.normal(0, 1, (P_FRAME, 3))),
               shs=f(g["shs"]))
    T = f(rng.normal(0, 1, (P_FRAME, 3, 3)) * 0.1 + np.eye(3))
    wts = dict(color=f(rng.normal(0, 1, (3, H_FRAME, W_FRAME))), depth=f(rng.normal(0, 1, (1, H_FRAME, W_FRAME))),
               alpha=f(rng.normal(0, 1, (1, H_FRAME, W_FRAME))), feats=f(rng.normal(0, 1, (6, 3, H_FRAME, W_FRAME))))
    return cam, raw, T, wts, f(rng.uniform(0, 1, (P_FRAME, 18))), f(rng.uniform(0, 1, (P_FRAME, 3)))


def _hip_frame(variant, link_on, split_xyz=False):
    """One frame: frame_activations -> frame_attributes -> forward_multi -> weighted loss -> backward.
    variant: "default" | "cov_frozen" (rot_cov = raw.detach()) | "foreign_extra" (the rasterizer gets the registered means3D but a
    fresh leaf as `extra`, fixed colours and the activated scales / rotations: nothing of the attribute call reaches it).
    split_xyz: the rasterizer reads its positions from a leaf of its own (a measuring run: its position gradient on its own)."""
    from mygauhuman_amd import gradlink
    from mygauhuman_amd.activations import frame_activations
    from mygauhuman_amd.attributes import frame_attributes
    from mygauhuman_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    cam, raw, T, wts, extra_np, fixed_col = _frame_inputs()
    d = util.to_dev
    leaf = {k: d(v).requires_grad_(True) for k, v in raw.items()}
    rs = GaussianRasterizationSettings(image_height=H_FRAME, image_width=W_FRAME, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                       bg=d(np.array([0.1, 0.2, 0.3], np.float32)), scale_modifier=1.0, viewmatrix=d(cam["viewmatrix"]),
                                       projmatrix=d(cam["projmatrix"]), sh_degree=3, campos=d(cam["campos"]), prefiltered=False,
                                       debug=False)
    mid = {}
    with gradlink.frame_link(link_on):
        op, alb, sc, rot, nrm, occ = frame_activations(leaf["opacity"], leaf["albedo"], leaf["scaling"], leaf["rotation"], leaf["normal"])
        rot_cov = leaf["rotation"].detach() if variant == "cov_frozen" else leaf["rotation"]
        cov, col, feat = frame_attributes(leaf["xyz"], d(T), nrm, sc, 1.0, rot_cov, rot, alb, alb, occ, leaf["shs"], 3, rs.campos,
                                          rs.viewmatrix)
        xyz_r = d(raw["xyz"]).requires_grad_(True) if split_xyz else leaf["xyz"]
        m2d = torch.zeros((P_FRAME, 3), device=DEV, requires_grad=True)
        rast = GaussianRasterizer(rs)
        if variant == "foreign_extra":
            leaf["extra"] = d(extra_np).requires_grad_(True)
            out = rast.forward_multi(means3D=xyz_r, means2D=m2d, opacities=op, extra_colors=leaf["extra"], colors_precomp=d(fixed_col),
                                     scales=sc, rotations=rot, sync_free=False)
        else:
            for k, v in (("cov", cov), ("col", col), ("feat", feat), ("op", op)):
                v.retain_grad()
                mid[k] = v
            out = rast.forward_multi(means3D=xyz_r, means2D=m2d, opacities=op, extra_colors=feat, colors_precomp=col,
                                     cov3D_precomp=cov, sync_free=False)
    color, radii, depth, alpha, feats = out
    assert float((radii > 0).float().mean()) > 0.5
    loss = (color * d(wts["color"])).sum() + (depth * d(wts["depth"])).sum() + (alpha * d(wts["alpha"])).sum()
    loss = loss + sum((fi * d(w)).sum() for fi, w in zip(feats, wts["feats"]))
    loss.backward()
    n = lambda t: None if t is None else t.detach().cpu().to(torch.float64).numpy()  # noqa: E731
    return ({k: n(v.grad) for k, v in leaf.items()}, {k: n(v.grad) for k, v in mid.items()},
            n(xyz_r.grad) if split_xyz else None)


def _chain_frame(variant, gouts, dtype):
    """The float64 / float32 CPU chain of _hip_frame up to the rasterizer's inputs, pulled back with the rasterizer's gradients."""
    import torch.nn.functional as F
    from tests.torch_reference import frame_attributes_torch
    cam, raw, T, _, _, _ = _frame_inputs()
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    leaf = {k: t(v).requires_grad_(True) for k, v in raw.items()}
    op, alb, sc = torch.sigmoid(leaf["opacity"]), torch.sigmoid(leaf["albedo"]), torch.exp(leaf["scaling"])
    rot, nrm = F.normalize(leaf["rotation"]), leaf["normal"] / leaf["normal"].norm(dim=1, keepdim=True)
    rot_cov = leaf["rotation"].detach() if variant == "cov_frozen" else leaf["rotation"]
    cov, col, feat = frame_attributes_torch(leaf["xyz"], t(T), nrm, sc, 1.0, rot_cov, rot, alb, alb, op.repeat(1, 3), leaf["shs"], 3,
                                            t(cam["campos"]), t(cam["viewmatrix"]))
    grads = torch.autograd.grad([cov, col, feat, op], [leaf[k] for k in LEAVES], [t(gouts[k]) for k in ("cov", "col", "feat", "op")])
    return {k: g.to(torch.float64).numpy() for k, g in zip(LEAVES, grads)}


@pytest.mark.parametrize("variant", ["default", "cov_frozen"])
def test_hand_built_frame_gradients_match_the_float64_chain_and_the_unlinked_frame(links, variant):
    """cov_frozen: rot_cov = raw.detach() -- the raw quaternion only receives the gradient that comes through its normalisation
    (the attribute kernel's rot_cov gradient is neither parked nor returned)."""
    on, _, _ = _hip_frame(variant, True)
    _nothing_parked(links, 1)
    off, _, _ = _hip_frame(variant, False)
    split, mid, g_xyz_raster = _hip_frame(variant, False, split_xyz=True)
    want, ref32 = _chain_frame(variant, mid, torch.float64), _chain_frame(variant, mid, torch.float32)
    want["xyz"], ref32["xyz"] = want["xyz"] + g_xyz_raster, ref32["xyz"] + g_xyz_raster
    for k in LEAVES:
        assert on[k] is not None and np.isfinite(on[k]).all(), k
        util.assert_close(f"{variant}: d_{k} link on vs off", on[k], off[k], tol=NOISE, max_bad_frac=0.0)
        e32 = ac.measure(ref32[k], want[k])
        print(f"{variant}: d_{k}: float32 chain {e32:.3e}  frame {ac.measure(on[k], want[k]):.3e}")
        util.assert_close(f"{variant}: d_{k} vs float64 chain", on[k], want[k], tol=2 * e32 + 4 * ac.ULP + NOISE, max_bad_frac=0.0,
                          outer_tol=2 * e32 + 4 * ac.ULP + NOISE)


def _chain_foreign(rec, dtype):
    """foreign_extra: the rasterizer's own input gradients pulled back through the float64 / float32 activations; the positions
    and the foreign `extra` are leaves the rasterizer reads directly."""
    import torch.nn.functional as F
    _, raw, _, _, _, _ = _frame_inputs()
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    leaf = {k: t(raw[k]).requires_grad_(True) for k in ("opacity", "scaling", "rotation")}
    outs = [torch.sigmoid(leaf["opacity"]), torch.exp(leaf["scaling"]), F.normalize(leaf["rotation"])]
    g = torch.autograd.grad(outs, list(leaf.values()), [t(rec["grads"][k]) for k in ("opacity", "scales", "rotations")])
    want = {k: x.to(torch.float64).numpy() for k, x in zip(leaf, g)}
    want.update(xyz=rec["grads"]["means3D"], extra=rec["grads"]["extra"], albedo=None, normal=None, shs=None)
    return want


def test_positions_keep_the_rasterizer_gradient_when_extra_is_not_this_frames_features(links, raster_calls):
    """forward_multi is fed the means3D the attribute call registered, but an `extra` from elsewhere and nothing else of that call:
    the attribute backward never runs, so a parked position gradient would have no consumer -- it must reach means3D through
    autograd, as with the link off; every leaf gradient is the rasterizer's own gradient pulled back through the float64
    activations."""
    on, _, _ = _hip_frame("foreign_extra", True)
    _nothing_parked(links, 1)
    rec = raster_calls[0]
    off, _, _ = _hip_frame("foreign_extra", False)
    assert on["xyz"] is not None, "means3D lost the rasterizer's gradient (parked for a backward that never runs)"
    for k in ("xyz", "extra", "opacity", "scaling", "rotation"):
        assert on[k] is not None and np.abs(on[k]).max() > 0, k
        util.assert_close(f"foreign extra: d_{k} link on vs off", on[k], off[k], tol=NOISE, max_bad_frac=0.0)
    for k in ("albedo", "normal", "shs"):
        assert (on[k] is None or not on[k].any()) and (off[k] is None or not off[k].any()), k
    _check_against_chain("foreign extra", on, _chain_foreign(rec, torch.float64), _chain_foreign(rec, torch.float32))


# ------------------------------------------------------------------------------------------ render() cases
KEYS = ("render", "normal", "albedo", "occlusion", "roughness", "world_normal", "render_axis", "render_alpha")
BG = np.array([0.1, 0.2, 0.3], np.float32)
NAMES = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "normal", "albedo")


def _pipe(**kw):
    return types.SimpleNamespace(debug=False, compute_cov3D_python=kw.pop("cov", True), convert_SHs_python=kw.pop("sh", True), **kw)


def _loss(o, keys=KEYS):
    return sum(o[k].mean() * (i + 1) for i, k in enumerate(keys))


def _second_camera(s):
    from mygauhuman_amd import cameras
    c = cameras.look_at_camera(s.cam_np["W"], s.cam_np["H"], eye=[-0.8, 0.2, -2.4], target=[0.0, -0.1, 0.0], fov_deg=50.0)
    return c, cameras.ViewCamera(c, "cuda", s.cam.smpl_param, s.cam.big_pose_smpl_param, s.cam.big_pose_world_vertex)


def _render_case(oracle, case, on):
    """Runs one case with GRAD_LINK = on; returns (parameter gradients or None by name, number of frames, the scene, the numpy
    cameras of the frames that were differentiated)."""
    import mygauhuman_amd.gaussian_renderer as gr
    gr.GRAD_LINK = on
    s = _human_scene(oracle, P=1500, V=600, seed=7, motion=(case == "cached_transforms"))
    m, bg, frames, cams = s.model, util.to_dev(BG), 1, [s.cam_np]
    if case == "positions_frozen":
        m._xyz.requires_grad_(False)
        _loss(gr.render(1, s.cam, m, _pipe(), bg)).backward()
    elif case == "two_cameras":
        frames = 2
        c2, cam2 = _second_camera(s)
        cams.append(c2)
        (_loss(gr.render(1, s.cam, m, _pipe(), bg)) + _loss(gr.render(1, cam2, m, _pipe(), bg))).backward()
    elif case in ("backward_twice", "backward_once"):
        loss = _loss(gr.render(1, s.cam, m, _pipe(), bg))
        loss.backward(retain_graph=True)
        if case == "backward_twice":
            loss.backward()
    elif case == "alpha_only":
        _loss(gr.render(1, s.cam, m, _pipe(), bg), ("render_alpha",)).backward()
    elif case == "rasterizer_cov_and_override_color":
        col = torch.rand((m.get_xyz.shape[0], 3), generator=torch.Generator().manual_seed(1)).to(DEV)
        _loss(gr.render(1, s.cam, m, _pipe(cov=False, sh=False), bg, override_color=col)).backward()
    elif case == "cached_transforms":
        class PoseDec(torch.nn.Module):
            def forward(self, posevec):
                return {"Rs": torch.eye(3, device=posevec.device)[None, None].repeat(1, 23, 1, 1)}

        class WDec(torch.nn.Module):
            def forward(self, pts):
                return torch.zeros(1, 24, pts.shape[1], device=pts.device)
        m.pose_decoder, m.lweight_offset_decoder = PoseDec(), WDec()
        with torch.no_grad():
            first = gr.render(1, s.cam, m, _pipe(), bg, return_smpl_rot=True)
        frames = 2
        _loss(gr.render(1, s.cam, m, _pipe(), bg, transforms=first["transforms"], translation=first["translation"])).backward()
    else:
        raise ValueError(case)
    grads = {n: (None if p.grad is None else p.grad.detach().cpu().to(torch.float64).numpy()) for n, p in zip(NAMES, m.parameters())}
    return grads, frames, s, cams


def _pull_back(oracle, case, s, cams, recs, dtype):
    """The leaf gradients the float64 (or float32) chain of test_gpu_render._chain64 -- activations, LBS deform, covariance, SH
    colour, feature colours, with the case's frozen / overridden inputs -- gives for the rasterizer's own input gradients `recs`
    (one record per rasterizer backward, matched to its camera by the camera position), summed over the records."""
    from tests.test_gpu_render import _chain64
    ids = oracle.nearest_vertex(s.g["means3D"], s.big_verts)
    total = {n: None for n in NAMES}
    for rec in recs:
        cam_np = min(cams, key=lambda c: float(np.abs(np.asarray(c["campos"], np.float64) - rec["campos"]).max()))
        leaf = {n: p.detach().cpu().to(dtype).requires_grad_(not (n == "xyz" and case == "positions_frozen"))
                for n, p in zip(NAMES, s.model.parameters())}
        dec = None
        if case == "cached_transforms":   # identity pose correction, zero skinning-weight offsets: what the two decoders of the case return
            dec = dict(delta=torch.zeros((23, 3, 3), dtype=dtype), w=torch.zeros(24, dtype=dtype))
        ch = _chain64(types.SimpleNamespace(**{**vars(s), "cam_np": cam_np}), leaf, ids, dec, dtype)
        pairs = [("means3D", "means3D"), ("opacity", "opacity"), ("features", "extra")]
        if case == "rasterizer_cov_and_override_color":   # the rasterizer builds the covariance itself and the colours are constants
            pairs += [("scaling", "scales"), ("rotation", "rotations")]
        else:
            pairs += [("cov6", "cov3D"), ("colors", "colors")]
        pairs = [(a, b) for a, b in pairs if ch[a].requires_grad]   # (frozen positions: the posed means are constants of the chain)
        outs = [ch[a] for a, _ in pairs]
        gouts = [torch.from_numpy(rec["grads"][b]).to(dtype).reshape(ch[a].shape) for a, b in pairs]
        inputs = [n for n in NAMES if leaf[n].requires_grad]
        for n, g in zip(inputs, torch.autograd.grad(outs, [leaf[n] for n in inputs], gouts, allow_unused=True)):
            if g is not None:
                g = g.to(torch.float64).numpy()
                total[n] = g if total[n] is None else total[n] + g
    return total


@pytest.fixture()
def grad_link_switch():
    import mygauhuman_amd.gaussian_renderer as gr
    before = gr.GRAD_LINK
    yield
    gr.GRAD_LINK = before


@pytest.mark.parametrize("case", ["positions_frozen", "two_cameras", "backward_twice", "alpha_only",
                                  "rasterizer_cov_and_override_color", "cached_transforms"])
def test_render_gradients_with_the_link_equal_those_without(oracle, links, raster_calls, grad_link_switch, case):
    """render() on the small human scene with the link on: every parameter gradient against (a) the float64 chain applied to the
    gradients the rasterizer returned for its own inputs in that very run and (b) the same render() with GRAD_LINK off."""
    on, frames, s, cams = _render_case(oracle, case, True)
    _nothing_parked(links, frames)
    recs = list(raster_calls)
    assert len(recs) == 2 if case in ("two_cameras", "backward_twice") else len(recs) == 1
    off, _, _, _ = _render_case(oracle, case, False)
    for n in NAMES:
        a, b = on[n], off[n]
        assert (a is None) == (b is None), n
        if a is not None:
            assert np.isfinite(a).all(), n
            util.assert_close(f"{case}: d_{n} link on vs off", a, b, tol=NOISE, max_bad_frac=0.0)
    _check_against_chain(case, on, _pull_back(oracle, case, s, cams, recs, torch.float64),
                         _pull_back(oracle, case, s, cams, recs, torch.float32))
    live = {n for n in NAMES if on[n] is not None and np.abs(on[n]).max() > 0}
    if case == "positions_frozen":
        assert on["xyz"] is None and live >= {"f_dc", "scaling", "rotation", "opacity", "normal", "albedo"}
    elif case == "alpha_only":
        # alpha depends on the geometry and the opacity only, and the rasterizer's backward is handed None -- not a zero image --
        # for each of the six feature images
        assert recs[0]["feature_grad_is_none"] == [True] * 6, recs[0]["feature_grad_is_none"]
        assert live == {"xyz", "scaling", "rotation", "opacity"}, live
    elif case == "rasterizer_cov_and_override_color":
        assert live == {"xyz", "scaling", "rotation", "opacity", "normal", "albedo"}, live
    else:
        assert live == set(NAMES), live
        assert not any(recs[0]["feature_grad_is_none"])
    if case == "backward_twice":
        once, _, _, _ = _render_case(oracle, "backward_once", True)
        for n in NAMES:
            util.assert_close(f"d_{n}: two backward calls = twice one", on[n], 2.0 * once[n], tol=NOISE, max_bad_frac=0.0)
