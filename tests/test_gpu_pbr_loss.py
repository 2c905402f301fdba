"""The fused PBR-phase training loss on the GPU (csrc/pbr_loss.hip behind mygauhuman_amd.pbr.loss): every term and gradient against
the fixture made by the reference's own code (tests/golden/make_golden_pbr_loss.py) and against the float64 restatement
(tests/pbr_loss_reference.py) from 2 x 3 to 1024², the edge cases, run-to-run bits, the smoothness gather at 200k Gaussians, and a
whole PBR training step (render() -> pbr_shading -> PbrPhaseLoss + ssim + env-map TV) against the same step with the torch
composition and recorded by graph.GraphedFrame."""
import os
import types

import numpy as np
import pytest
import torch

from tests import pbr_loss_reference as R

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbr_loss.npz")
TOL = 1e-4
SIZES = [(2, 3), (17, 23), (512, 512), (1024, 1024), (540, 720)]


def _close(name, got, want, tol=TOL):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = want.detach().double().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if np.isnan(want).any() or np.isnan(got).any():
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        got, want = np.nan_to_num(got), np.nan_to_num(want)
    scale = float(np.abs(want).max()) if want.size else 0.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= tol * scale + 1e-30, f"{name}: max error {err:.3e} against a magnitude of {scale:.3e}"


def _gpu(x):
    """float32 leaves on the GPU (knn stays integer)."""
    return {k: (v.float().cuda().requires_grad_(k in R.GRAD_INPUTS) if v.is_floating_point() else v.cuda()) for k, v in x.items()}


def _fused_terms(g):
    """Each term through the standalone entry points ({name: (value, {input: grad})}) and the whole PbrPhaseLoss."""
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss, gaussian_entropy, get_masked_tv_loss
    out = {}

    def run(name, fn, inputs):
        for k in inputs:
            g[k].grad = None
        v = fn()
        v.backward()
        out[name] = (float(v), {k: g[k].grad.clone() if g[k].grad is not None else torch.zeros_like(g[k]) for k in inputs})
    sm = MaterialSmoothness(g["knn"])
    run("tv", lambda: get_masked_tv_loss(g["alpha"], torch.cat([g["albedo"], g["roughness"]], 0)), ("alpha", "albedo", "roughness"))
    run("entropy_albedo", lambda: gaussian_entropy(g["albedo"]), ("albedo",))
    run("entropy_roughness", lambda: gaussian_entropy(g["roughness"]), ("roughness",))
    run("smooth_albedo", lambda: sm(g["albedo_g"], None), ("albedo_g",))
    run("smooth_roughness", lambda: sm(g["roughness_g"], None), ("roughness_g",))
    for k in R.GRAD_INPUTS:
        g[k].grad = None
    fused = PbrPhaseLoss(g["gt"], g["bound"], g["knn"])
    loss, terms = fused(g["rgb"], g["alpha"], g["albedo"], g["roughness"], g["albedo_g"], g["roughness_g"])
    loss.backward()
    whole = (float(loss), terms.cpu().numpy(), {k: g[k].grad.clone() for k in R.GRAD_INPUTS})
    return out, whole


def _check(x, vals, grads, where):
    """Compare the fused path with per-term values / gradients (the fixture's, with rule (a) applied, or the restatement's)."""
    g = _gpu(x)
    parts, (loss, terms, dl) = _fused_terms(g)
    for name, (v, gr) in parts.items():
        _close(f"{where} {name}", v, vals[name])
        for k, t in gr.items():
            _close(f"{where} d {name} / d {k}", t, grads[name][k])
    want_terms, want_loss, want_dl = R.combine(vals, grads)
    _close(f"{where} terms", terms, [want_terms[k] for k in R.TERMS])
    _close(f"{where} loss", loss, want_loss)
    for k in R.GRAD_INPUTS:
        _close(f"{where} d loss / d {k}", dl[k], want_dl[k])


@pytest.mark.parametrize("case", list(R.CASES))
def test_matches_reference_fixture(case):
    fx = np.load(FIXTURE)
    x = R.case_inputs(case)
    names = ("l1", "tv", "entropy_albedo", "entropy_roughness", "smooth_albedo", "smooth_roughness", "prior")
    vals = {n: float(fx[f"{case}/{n}"]) for n in names}
    grads = {}
    for n in names:
        grads[n] = {}
        for k in R.GRAD_INPUTS:
            key = f"{case}/{n}/d_{k}"
            # rule (a): the reference's NaN gradient of a constant entropy column is the fused path's zero
            grads[n][k] = np.nan_to_num(fx[key], nan=0.0) if key in fx.files else np.zeros(tuple(x[k].shape))
    _check(x, vals, grads, case)


@pytest.mark.parametrize("H,W", SIZES)
def test_matches_restatement(H, W):
    x = R.case_inputs(None, H, W, 2000, 7 + H)
    vals, grads = R.terms_and_grads(x)
    _check(x, vals, grads, f"{H}x{W}")


# ---- edge cases ---------------------------------------------------------------------------------------------------------------
def test_empty_bound_and_zero_alpha():
    from mygauhuman_amd.pbr import PbrPhaseLoss
    for case, term, inp in (("empty_bound", 0, "rgb"), ("zero_alpha", 4, "roughness")):
        g = _gpu(R.case_inputs(case))
        loss, terms = PbrPhaseLoss(g["gt"], g["bound"])(g["rgb"], g["alpha"], g["albedo"], g["roughness"])
        loss.backward()
        assert torch.isnan(loss) and torch.isnan(terms[term]), case
        others = [i for i in range(5) if i != term]
        assert torch.isfinite(terms[others]).all(), case
        for k in ("rgb", "alpha", "albedo", "roughness"):
            assert torch.isfinite(g[k].grad).all(), (case, k)
        if case == "empty_bound":
            assert (g["rgb"].grad == 0).all()
        else:  # alpha = 0: no prior gradient, and the TV's mask products are all zero
            assert (g["alpha"].grad == 0).all() and float(terms[1]) == 0.0


def _composition_entropy(x):
    """train.py:47-71 as torch ops (the composition the fused path replaces): its branches read the device."""
    v = x.view(-1, x.shape[-1])
    sigma = v.var(dim=0)
    centers = (torch.arange(15, device=x.device, dtype=x.dtype) + 0.5) / 15
    h = ((-0.5 * ((v[None] - centers[:, None, None]) / sigma).pow(2)).exp() / (sigma * np.sqrt(np.pi * 2)) * (1.0 / 15)).sum(1)
    e = 0
    for i in range(3):
        hi = h[..., i]
        hi = hi / hi.sum() + 1e-6 if hi.sum() > 1e-6 else torch.ones_like(hi)
        e = e + torch.sum(-hi * torch.log(hi))
    return e


def test_constant_column_gets_zero_gradient_where_the_composition_gets_nan():
    from mygauhuman_amd.pbr import gaussian_entropy
    x = R.case_inputs("edges")["albedo"].float().cuda()   # column 0 constant, columns 1, 2 not
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    ea, eb = _composition_entropy(a), gaussian_entropy(b)
    ea.backward()
    eb.backward()
    _close("entropy value", eb, float(ea))
    assert torch.isnan(a.grad[:, :, 0]).all()               # the composition: 0 * inf on every pixel of the constant column
    assert (b.grad[:, :, 0] == 0).all()                       # the fused path: rule (a)
    _close("entropy gradient of the other columns", b.grad[:, :, 1:], a.grad[:, :, 1:])
    assert (b.grad[:, :, 3:] == 0).all()


def test_argument_errors_are_raised_on_the_host():
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss, gaussian_entropy
    with pytest.raises(ValueError, match="at least 3"):
        gaussian_entropy(torch.rand(3, 8, 2, device="cuda"))
    P = 100
    knn = torch.randint(0, P, (P, 3), device="cuda")
    for bad in (-1, P):
        k = knn.clone()
        k[7, 2] = bad
        with pytest.raises(ValueError, match="knn indices"):
            MaterialSmoothness(k)
    sm = MaterialSmoothness(knn)
    with pytest.raises(ValueError, match=r"\[100, C\]"):
        sm(torch.rand(P + 1, 3, device="cuda"))
    fused = PbrPhaseLoss(torch.rand(3, 8, 8, device="cuda"), torch.ones(1, 8, 8, device="cuda"), knn)
    img = [torch.rand(3, 8, 8, device="cuda"), torch.rand(1, 8, 8, device="cuda"), torch.rand(3, 8, 8, device="cuda"),
           torch.rand(1, 8, 8, device="cuda")]
    with pytest.raises(ValueError, match=r"\[100, C\]"):
        fused(*img, torch.rand(P - 1, 3, device="cuda"), torch.rand(P, 1, device="cuda"))
    with pytest.raises(ValueError, match="W >= 3"):
        PbrPhaseLoss(torch.rand(3, 8, 2, device="cuda"), torch.ones(1, 8, 2, device="cuda"))


def test_targets_in_place_and_shared_knn_tables():
    """Float32 contiguous targets are read in place (an in-place update is seen by the next call); a bool mask is copied and
    says so; a MaterialSmoothness passed as knn is shared, not rebuilt."""
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss
    g = _gpu(R.case_inputs("random"))
    args = (g["rgb"], g["alpha"], g["albedo"], g["roughness"], g["albedo_g"], g["roughness_g"])
    sm = MaterialSmoothness(g["knn"])
    gt = g["gt"].detach().clone()
    fused = PbrPhaseLoss(gt, g["bound"], sm)
    assert fused.targets_in_place and fused.smooth is sm
    before = fused(*args)[1].clone()
    gt.copy_(torch.rand_like(gt))
    after = fused(*args)[1]
    fresh = PbrPhaseLoss(gt.clone(), g["bound"], sm)(*args)[1]
    assert not torch.equal(before[0], after[0]) and torch.equal(after, fresh)
    copied = PbrPhaseLoss(gt, g["bound"] == 1, sm)
    assert not copied.targets_in_place and torch.equal(copied(*args)[1], fresh)


def test_two_calls_give_the_same_bits():
    from mygauhuman_amd.pbr import PbrPhaseLoss
    g = _gpu(R.case_inputs(None, 512, 512, 20000, 3))
    fused = PbrPhaseLoss(g["gt"], g["bound"], g["knn"])
    runs = []
    for _ in range(2):
        for k in R.GRAD_INPUTS:
            g[k].grad = None
        loss, terms = fused(g["rgb"], g["alpha"], g["albedo"], g["roughness"], g["albedo_g"], g["roughness_g"])
        loss.backward()
        runs.append([loss.detach().clone(), terms.clone()] + [g[k].grad.clone() for k in R.GRAD_INPUTS])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_non_contiguous_render_rgb():
    """train.py passes pbr_shading's [H, W, 3] output permuted to [3, H, W]: read in place, gradient in the same layout."""
    from mygauhuman_amd.pbr import PbrPhaseLoss
    g = _gpu(R.case_inputs("random"))
    hwc = g["rgb"].detach().permute(1, 2, 0).contiguous().requires_grad_(True)
    fused = PbrPhaseLoss(g["gt"], g["bound"])
    outs = []
    for rgb in (hwc.permute(2, 0, 1), g["rgb"]):
        loss, _ = fused(rgb, g["alpha"], g["albedo"], g["roughness"])
        loss.backward()
        outs.append(float(loss))
    assert outs[0] == outs[1]
    assert torch.equal(hwc.grad.permute(2, 0, 1), g["rgb"].grad)


def test_smoothness_matches_composition_at_200k():
    from mygauhuman_amd.pbr import MaterialSmoothness
    P = 200_000
    gen = torch.Generator(device="cuda").manual_seed(0)
    knn = torch.randint(0, P, (P, 3), device="cuda", generator=gen)
    knn[:, 0] = torch.arange(P, device="cuda")
    base = torch.rand(P, 3, device="cuda", generator=gen) * 0.98 + 0.02
    ga, gr = base.clone().requires_grad_(True), base[:, :1].clone().requires_grad_(True)
    ca, cr = base.clone().requires_grad_(True), base[:, :1].clone().requires_grad_(True)
    MaterialSmoothness(knn)(ga, gr).backward()

    def term(g):
        a, b = g[knn][:, 1], g[knn][:, 2]
        return (torch.abs(a - b) / (b + 1e-6)).mean()
    comp = term(ca) + term(cr)
    comp.backward()
    fused = MaterialSmoothness(knn)(ga.detach(), gr.detach())
    _close("smoothness value", fused, float(comp))
    _close("d smoothness / d albedo_g", ga.grad, ca.grad)
    _close("d smoothness / d roughness_g", gr.grad, cr.grad)


# ---- a whole PBR training step -------------------------------------------------------------------------------------------------
def _pbr_scene():
    """A baked camera of the synthetic human, a light, and the PBR-phase inputs of train.py:296-313 around them."""
    import mygauhuman_amd
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.pbr import CubemapLight, get_brdf_lut
    from tests import pbr_reference as PR
    from tests.test_gpu_render import _human_scene
    s = _human_scene(None)
    s.pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    s.bg = torch.zeros(3, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    s.env = torch.rand((1, 16, 32), device="cuda", generator=gen) * 0.01
    torch.manual_seed(0)
    s.cubemap = CubemapLight(base_res=32).cuda()
    s.lut = get_brdf_lut(os.path.join(os.path.dirname(FIXTURE), "pbr_brdf_256_256.bin")).cuda()
    s.dirs = torch.from_numpy(PR.envmap_dirs([64, 128]).astype(np.float32)).cuda()[None].contiguous()
    s.cam.occlusion = None
    mygauhuman_amd.install_dropin(bake=True)
    # bakes the camera once.  Without autograd: a graph over the parameters that outlives this call would keep their
    # gradient-accumulation nodes, made on this (default) stream, and a later capture's backward would fork onto that stream
    with torch.no_grad():
        out = gr.render(30001, s.cam, s.model, s.pipe, s.bg, envmap=s.env)
    assert s.cam.occlusion is not None
    s.H, s.W = out["render"].shape[1:]
    s.view_dirs = torch.nn.functional.normalize(torch.randn(s.H, s.W, 3, device="cuda", generator=gen), dim=-1)
    s.gt = torch.rand(3, s.H, s.W, device="cuda", generator=gen)
    s.bound = (out["render_alpha"].detach() > 0.05).float()
    xyz = s.model._xyz.detach()
    s.knn = torch.cdist(xyz, xyz).topk(3, largest=False).indices
    s.crop = (s.H // 8, s.H - s.H // 8, s.W // 4, s.W - s.W // 4)   # the per-camera boundingRect crop, fixed
    return s


def _shade(s, o):
    from mygauhuman_amd.pbr import pbr_shading
    s.cubemap.build_mips()
    alpha = o["render_alpha"]
    rough = o["roughness"][0:1] * (1.0 - 0.04) + 0.04
    res = pbr_shading(light=s.cubemap, normals=o["world_normal"].permute(1, 2, 0).detach(), view_dirs=s.view_dirs,
                      mask=alpha.permute(1, 2, 0), albedo=o["albedo"].permute(1, 2, 0), roughness=rough.permute(1, 2, 0),
                      metallic=None, tone=False, gamma=False, occlusion=o["occlusion"][0:1].permute(1, 2, 0), brdf_lut=s.lut)
    return res["render_rgb"].permute(2, 0, 1), alpha, rough


def _rest_of_loss(s, rgb):
    """The fused ssim on the fixed crop and the environment-map TV (train.py:319-324, :348-361)."""
    import mygauhuman_amd.nvdiffrast.torch as dr
    from mygauhuman_amd.loss_utils import ssim
    y0, y1, x0, x1 = s.crop
    loss = 0.01 * (1.0 - ssim(rgb[:, y0:y1, x0:x1][None], s.gt[:, y0:y1, x0:x1][None]))
    em = dr.texture(s.cubemap.base[None], s.dirs, filter_mode="linear", boundary_mode="cube")[0]
    return loss + 0.01 * (((em[1:] - em[:-1]) ** 2).mean() + ((em[:, 1:] - em[:, :-1]) ** 2).mean())


def test_pbr_training_step_matches_the_torch_composition():
    """render() -> build_mips -> pbr_shading -> PbrPhaseLoss + fused ssim on a fixed crop + env-map TV -> backward, on a camera whose
    occlusion is baked: the Gaussians' and the light's gradients equal those of the same step with the torch composition."""
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.pbr import PbrPhaseLoss
    try:
        s = _pbr_scene()
        fused = PbrPhaseLoss(s.gt, s.bound, s.knn)
        params = list(s.model.parameters()) + [s.cubemap.base]
        results = []
        for composition in (False, True):
            for p in params:
                p.grad = None
            o = gr.render(30001, s.cam, s.model, s.pipe, s.bg, envmap=s.env)
            rgb, alpha, rough = _shade(s, o)
            if composition:
                loss = _composition(rgb, s.gt, s.bound, alpha, o["albedo"], rough, s.model.get_albedo, s.model.get_roughness, s.knn)
            else:
                loss, terms = fused(rgb, alpha, o["albedo"], rough, s.model.get_albedo, s.model.get_roughness)
                assert torch.isfinite(terms).all()
            loss = loss + _rest_of_loss(s, rgb)
            loss.backward()
            results.append((float(loss), [None if p.grad is None else p.grad.detach().clone() for p in params]))
        (lf, gf), (lc, gc) = results
        assert np.isfinite(lc), "the composition is not finite on this scene"
        _close("step loss", lf, lc)
        for i, (a, b) in enumerate(zip(gf, gc)):
            assert (a is None) == (b is None), i
            if b is None:
                continue
            assert torch.isfinite(b).all(), f"the composition is not finite on this scene (gradient {i})"
            _close(f"step gradient {i}", a, b.cpu().numpy())
        assert float(s.cubemap.base.grad.abs().sum()) > 0
    finally:
        gr.BAKE = False


def test_pbr_training_step_is_captured_by_graphed_frame():
    """render() -> build_mips -> pbr_shading -> PbrPhaseLoss + fused ssim on a fixed crop + env-map TV -> backward, on a camera whose
    occlusion is baked, recorded by graph.GraphedFrame: the capture passes its own verification, and a replay equals the eager
    step (Gaussian and light gradients at 2e-5), also after the target is updated in place."""
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.graph import GraphedFrame
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss
    try:
        s = _pbr_scene()
        fused = PbrPhaseLoss(s.gt, s.bound, MaterialSmoothness(s.knn))
        assert fused.targets_in_place
        params = list(s.model.parameters()) + [s.cubemap.base]

        def step():
            o = gr.render(30001, s.cam, s.model, s.pipe, s.bg, envmap=s.env)
            rgb, alpha, rough = _shade(s, o)
            loss, terms = fused(rgb, alpha, o["albedo"], rough, s.model.get_albedo, s.model.get_roughness)
            loss = loss + _rest_of_loss(s, rgb)
            loss.backward()
            return loss.detach(), terms

        def eager():
            for p in params:
                p.grad = None
            loss, terms = step()
            torch.cuda.synchronize()
            return loss.clone(), terms.clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

        frame = GraphedFrame(step, warmup=3, zero_grads=params)
        for trial in range(2):
            if trial == 1:  # the next camera's target through the same graph: updated in place
                s.gt.copy_(torch.rand_like(s.gt))
            loss_e, terms_e, grads_e = eager()
            loss_g, terms_g = frame.replay()
            torch.cuda.synchronize()
            frame.check()
            assert torch.isfinite(terms_e).all()
            _close(f"captured loss {trial}", loss_g, loss_e, 2e-5)
            _close(f"captured terms {trial}", terms_g, terms_e, 2e-5)
            for i, (p, ge) in enumerate(zip(params, grads_e)):
                if ge is None:
                    continue
                _close(f"captured gradient {trial}.{i}", p.grad, ge, 2e-5)
        assert float(s.cubemap.base.grad.abs().sum()) > 0 and float(s.model._xyz.grad.abs().sum()) > 0
    finally:
        gr.BAKE = False


def _composition(rgb, gt, bound, alpha, albedo, rough, albedo_g, roughness_g, knn):
    """train.py:316-344 as torch ops (with the weights of PbrPhaseLoss's defaults)."""
    sel = bound[0] == 1
    l1 = (rgb.permute(1, 2, 0)[sel] - gt.permute(1, 2, 0)[sel]).abs().mean()
    pred = torch.cat([albedo, rough], 0)
    tv = ((pred[:, 1:] - pred[:, :-1]) ** 2 * (alpha[:, 1:] * alpha[:, :-1])).mean() + \
        ((pred[:, :, 1:] - pred[:, :, :-1]) ** 2 * (alpha[:, :, 1:] * alpha[:, :, :-1])).mean()
    ent = _composition_entropy(albedo) + _composition_entropy(rough)

    def sm(g):
        a, b = g[knn][:, 1], g[knn][:, 2]
        return (torch.abs(a - b) / (b + 1e-6)).mean()
    lamb = (1.0 - rough[alpha > 0]).mean()
    return l1 + tv + 5e-5 * ent + 0.1 * (sm(albedo_g) + sm(roughness_g)) + 0.001 * lamb
