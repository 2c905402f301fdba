"""The rasterizer and render() at an ACTIVE SH degree below the STORED one -- sixteen stored coefficients, degree 0, 1 or 2: what
every training run starts in -- and the rasterizer's own covariance path at a scale modifier other than 1.

Scenes and CPU references are those of tests/sh_degree_cases.py (the inactive bands are the scene's times 50;
test_sh_degree_host.py pins the oracle against the float64 restatement on them).  Through the raw `_C` bindings unless stated:

  forward    bit-exact per-Gaussian state against the oracle, images within 1e-4 of the oracle and of the float64 restatement,
             for the staged kernels (M = 16, aligned), the per-row kernels (M = 16 one float past a 16-byte boundary; M = 9, 4)
             and the block tails P = 1, 127, 129, 257
  backward   every gradient against the oracle (1e-4, 2e-4 of the elements) and the float64 autograd (1e-4), the inactive bands of
             dL_dsh and the rows of culled Gaussians exactly zero, with every output starting as 0xA5 bytes inside guard bands
  poison     NaN in the inactive coefficients changes no bit of any output (deterministic reduction)
  fp16       half storage == the fp32 path on the rounded coefficients, bit for bit; NaN / inf poison in halves
  sessions   RasterSession, the fused alpha-mask and phase-1 loss backwards, ViewParallelStep: a step at degree 3, then the step
             at D in the same buffers
  exchange   pack -> gsr_sh_grad_from_views at D < 3, M = 16
  render()   active_sh_degree = 0, 1, 2 against the oracle composition, both SH routes, fused against torch ops, one FusedAdam step
  modifier   scale_modifier 0.5 / 1.7 against the oracle, and == modifier 1 on float32(m) * scales, dL_dscales included
  graph      a GraphedFrame captured at degree 1, captured again after oneupSHdegree()

Largest error relative to the tensor's scale (util.assert_close's measure) measured on an MI355X with the default knobs, over the
two full scenes and the four tails; `o` = against the oracle, `f64` = against the float64 restatement (the oracle itself is within
4.6e-6 of the restatement on these scenes, test_sh_degree_host.py).  The per-Gaussian forward state has the oracle's bits throughout.

   M  D  SH tensor   images o   images f64   gradients o   gradients f64
  16  0  aligned     1.9e-07    3.6e-06      4.3e-06       6.0e-06
  16  1  aligned     1.7e-07    3.6e-06      6.6e-06       1.4e-05
  16  2  aligned     2.3e-07    3.6e-06      5.3e-06       1.3e-05
  16  0  offset4     1.9e-07    3.6e-06      4.4e-06       6.0e-06
  16  1  offset4     1.7e-07    3.6e-06      6.6e-06       1.4e-05
  16  2  offset4     2.3e-07    3.6e-06      5.3e-06       1.3e-05
   9  0  aligned     1.6e-07    3.6e-06      4.6e-06       7.8e-06
   9  1  aligned     2.4e-07    3.6e-06      3.5e-06       6.6e-06
   4  0  aligned     2.0e-07    3.6e-06      6.2e-06       1.5e-05

  inactive bands of dL_dsh, rows of culled Gaussians     exactly 0.0 in every case, entry point and storage type
  NaN / inf in the inactive coefficients                  no bit of any output changes (fp32 and fp16 storage)
  fp16 storage against fp32 on the rounded coefficients   images and state identical; gradients identical with the fixed-order
                                                          reduction, within 2.3e-07 with atomics
  session / fused-loss / view-parallel entry points       images identical to the raw binding; gradients within 8.5e-07
                                                          (phase-1 loss 2.2e-07), after a degree-3 step in the same buffers
  scale modifier 0.5, 1.7 (degree 3)                      images within 2.1e-07 of the oracle and 5.1e-06 of float64, gradients within
                                                          1.3e-05 of both; == modifier 1 on m * scales: state and images identical,
                                                          gradients identical (fixed order) / within 2.5e-07 (atomics)
  render(), active degree 0 / 1 / 2, both SH routes      colour |diff| to the oracle composition: 99.9th percentile 2.7e-06, mean 2.2e-07
"""
import types

import numpy as np
import pytest
import torch

from tests import raster_reference as rr
from tests import sh_degree_cases as sc
from tests import util
from tests.test_gpu_guardband import guarded  # noqa: F401  (fixture)
from tests.test_raster_reference_host import grad_names, rel_err, tolerance

pytestmark = pytest.mark.gpu

BG = sc.BG
# (M, D, alignment of the SH tensor): the staged kernels need M = 16 and 16-byte alignment
GPU_LAYOUTS = ([(16, D, "aligned") for D in (0, 1, 2)] + [(16, D, "offset4") for D in (0, 1, 2)]
               + [(9, 0, "aligned"), (9, 1, "aligned"), (4, 0, "aligned")])
SCENE_CUTS = [(name, spec[0]) for name, spec in sc.SCENES.items()] + [("p600", P) for P in sc.TAILS]
CASES = [(name, P, M, D, al) for name, P in SCENE_CUTS for M, D, al in GPU_LAYOUTS]
IDS = [f"{n}_P{P}_M{M}_D{D}_{al}" for n, P, M, D, al in CASES]
FULL = [(name, spec[0]) for name, spec in sc.SCENES.items()]
GRADS = grad_names("sh")


def sh_tensor(shs, align, dtype=torch.float32):
    """The device SH tensor of a case: "aligned" (16 bytes, what torch allocates) or "offset4": a contiguous [P,M,3] view that
    starts one float past a 16-byte boundary, which the staged kernels must refuse to take."""
    t = util.to_dev(shs).to(dtype)
    if align == "offset4":
        assert dtype == torch.float32
        flat = torch.zeros(t.numel() + 8, device="cuda")
        assert flat.data_ptr() % 16 == 0
        view = flat[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        t = view
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if align == "offset4" else 0)   # (.contiguous() returns it as it is)
    return t


def forward(s, g=None, shs=None, align="aligned", modifier=1.0, debug=True):
    g = s.g if g is None else g
    shs = sh_tensor(g["shs"], align) if shs is None else shs
    f = util.hip_forward(s.cam, g, BG, "sh", debug=debug, scale_modifier=modifier, shs=shs)
    assert f["sh"].data_ptr() == shs.data_ptr()
    return f


def forward_state(f):
    """Everything the forward leaves that a later kernel reads, as host arrays (per-Gaussian state of the visible ones)."""
    radii = f["radii"].cpu().numpy()
    vis = radii > 0
    out = dict(R=np.int64(f["R"]), radii=radii, color=f["color"].cpu().numpy(), depth=f["depth"].cpu().numpy(),
               alpha=f["alpha"].cpu().numpy(), TILES_TOUCHED=util.hip_query(f, "TILES_TOUCHED"),
               N_CONTRIB=util.hip_query(f, "N_CONTRIB"), FINAL_T=util.hip_query(f, "FINAL_T"), RANGES=util.hip_query(f, "RANGES"))
    for q in ("RGB", "CLAMPED", "DEPTHS", "MEANS2D", "CONIC_OPACITY"):
        out[q] = util.hip_query(f, q)[vis]
    return out


def assert_same_bits(what, a, b):
    assert set(a) == set(b)
    for k in a:
        assert sc.bits_equal(np.asarray(a[k]), np.asarray(b[k])), f"{what}: {k} differs"


@pytest.fixture()
def deterministic():
    from mygauhuman_amd import _lib
    _lib.set_tuning("deterministic", 1)
    yield
    _lib.set_tuning("deterministic", 0)


def check_forward(s, f, record):
    """(a): the assertions of test_forward_matches_oracle on the per-Gaussian state, images against both references."""
    pre, b, img = s.ref["pre"], s.ref["bin"], s.ref["img"]
    np.testing.assert_array_equal(f["radii"].cpu().numpy(), pre["radii"])
    assert f["R"] == b["R"]
    np.testing.assert_array_equal(util.hip_query(f, "TILES_TOUCHED").view(np.uint32), pre["tiles_touched"])
    vis = s.visible
    for q, k in (("RGB", "rgb"), ("CLAMPED", "clamped"), ("DEPTHS", "depths"), ("MEANS2D", "means2D"), ("CONIC_OPACITY", "conic_opacity")):
        np.testing.assert_array_equal(util.hip_query(f, q)[vis], pre[k][vis], err_msg=q)
    solid = img["fragile"] == 0
    for k in ("color", "depth", "alpha"):
        got = f[k].cpu().numpy()
        m_o, m_64 = np.broadcast_to(solid, got.shape), np.broadcast_to(s.keep, got.shape)
        record["img o"] = max(record.get("img o", 0.0), rel_err(got, img[k], m_o))
        record["img f64"] = max(record.get("img f64", 0.0), rel_err(got, s.r64[k], m_64))
    print("forward worst: " + " ".join(f"{k} {v:.2e}" for k, v in record.items()))
    for k in ("color", "depth", "alpha"):
        got = f[k].cpu().numpy()
        util.assert_close(k, got, img[k], tol=1e-4, mask=np.broadcast_to(solid, got.shape))
        util.assert_close(k + " vs float64", got, s.r64[k], tol=tolerance("identity", k), mask=np.broadcast_to(s.keep, got.shape))


def check_backward(s, got, record):
    """(b): every gradient against the oracle (the rule of test_backward_matches_oracle) and the float64 autograd."""
    for n in GRADS:
        x = got[n].reshape(s.want[n].shape)
        record[n + " o"], record[n + " f64"] = rel_err(x, s.want[n]), rel_err(x, s.want64[n])
    print("backward worst: " + " ".join(f"{k} {v:.2e}" for k, v in record.items()))
    for n in GRADS:
        x = got[n].reshape(s.want[n].shape)
        util.assert_close(n, x, s.want[n], tol=1e-4, max_bad_frac=2e-4)
        util.assert_close(n + " vs float64", x, s.want64[n], tol=tolerance("identity", n))
    sc.assert_inactive_zero("hip", got["dL_dsh"].reshape(s.want["dL_dsh"].shape), s.ref["pre"]["radii"], s.D)


# -------------------------------------------------------------------------------------------------------------- (a) forward
@pytest.mark.parametrize("name,P,M,D,align", CASES, ids=IDS)
def test_forward_below_the_stored_degree(oracle, name, P, M, D, align):
    s = sc.reference(oracle, name, P, M, D)
    f = forward(s, align=align)
    check_forward(s, f, {})
    if (name, P) in FULL:
        assert int(util.hip_query(f, "CLAMPED")[s.visible].sum()) > 0, "no clamped channel in this scene"
        assert s.keep.mean() > 1 - sc.MAX_MARGIN_FRAC


# ------------------------------------------------------------------------------------------------------------- (b) backward
@pytest.mark.parametrize("name,P,M,D,align", CASES, ids=IDS)
def test_backward_below_the_stored_degree(oracle, guarded, name, P, M, D, align):  # noqa: F811
    """Every tensor the bindings allocate starts as 0xA5 bytes (-2.9e-16 as a float, not zero) inside guard bands: a gradient
    element the backward does not write shows, and so does a write outside an array."""
    s = sc.reference(oracle, name, P, M, D)
    f = forward(s, align=align)
    assert guarded.check("forward") >= 7
    got = util.hip_backward(f, *s.up, debug=True)
    assert guarded.check("backward") >= 7
    check_backward(s, got, {})


# --------------------------------------------------------------------------------------------------------------- (c) poison
@pytest.mark.parametrize("name,P,M,D,align", CASES, ids=IDS)
def test_nan_in_the_inactive_bands_changes_no_bit(oracle, deterministic, name, P, M, D, align):
    """The oracle's outputs are bit-identical under this poison (test_sh_degree_host.py): the reference never reads the bands
    above the active degree, so neither may the kernels -- not even to multiply by zero."""
    s = sc.reference(oracle, name, P, M, D)
    res = {}
    for tag, g in (("zeros", sc.zeroed(s.g)), ("nan", sc.poisoned(s.g)), ("times50", s.g)):
        f = forward(s, g=g, align=align)
        res[tag] = (forward_state(f), util.hip_backward(f, *s.up, debug=True))
    for tag in ("nan", "times50"):
        assert_same_bits(f"{tag} forward", res[tag][0], res["zeros"][0])
        assert_same_bits(f"{tag} backward", res[tag][1], res["zeros"][1])
    assert not any(np.isnan(v).any() for v in res["nan"][1].values())


# ----------------------------------------------------------------------------------------------------------------- (d) fp16
def _raw(s, sh, D, modifier=1.0):
    """Forward + backward through the raw bindings on device tensors; returns (forward tuple, gradient tuple, per-pixel state)."""
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    d, g, cam = util.to_dev, s.g, s.cam
    H, W, P = cam["H"], cam["W"], g["means3D"].shape[0]
    e = torch.empty(0)
    bg = d(BG)
    o = _C.rasterize_gaussians(bg, d(g["means3D"]), e, d(g["opacities"]), d(g["scales"]), d(g["rotations"]), modifier, e,
                               d(cam["viewmatrix"]), d(cam["projmatrix"]), cam["tanfovx"], cam["tanfovy"], H, W, sh, D,
                               d(cam["campos"]), False, False)
    dc, dd, da = (d(x) for x in s.up)
    gr = _C.rasterize_gaussians_backward(bg, d(g["means3D"]), o[4], e, d(g["scales"]), d(g["rotations"]), modifier, e,
                                         d(cam["viewmatrix"]), d(cam["projmatrix"]), cam["tanfovx"], cam["tanfovy"], dc, dd, da, sh,
                                         D, d(cam["campos"]), o[5], o[0], o[6], o[7], o[3], False)
    px = [_C.query_state(q, P, o[0], W, H, o[5], o[6], o[7]) for q in ("N_CONTRIB", "FINAL_T", "RGB", "CLAMPED")]
    return o, gr, px


@pytest.mark.parametrize("name,P", FULL, ids=[n for n, _ in FULL])
@pytest.mark.parametrize("D", [0, 1, 2])
@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "deterministic"])
def test_fp16_storage_below_the_stored_degree(oracle, name, P, D, det):
    """Halves are widened exactly on load: every output has the bits of the fp32 path fed the fp16-rounded coefficients (the
    pattern of test_fp16_sh_storage_equals_fp32_on_rounded_coefficients), with NaN or inf in the inactive halves as well."""
    from mygauhuman_amd import _lib
    s = sc.reference(oracle, name, P, 16, D)
    n = s.n_active
    sh16 = util.to_dev(s.g["shs"]).half()
    assert torch.isfinite(sh16).all() and float(sh16[:, n:].abs().max()) > 0
    sh32 = sh16.float()
    variants = {"half": sh16, "float": sh32}
    for tag, v in (("half nan", float("nan")), ("half inf", float("inf"))):
        t = sh16.clone()
        t[:, n:] = v
        variants[tag] = t
    _lib.set_tuning("deterministic", det)
    try:
        res = {k: _raw(s, v, D) for k, v in variants.items()}
    finally:
        _lib.set_tuning("deterministic", 0)
    base = res["float"]
    for tag in ("half", "half nan", "half inf"):
        o, gr, px = res[tag]
        worst = 0.0
        assert o[0] == base[0][0], tag
        for x, y in zip(list(o[1:5]) + px, list(base[0][1:5]) + base[2]):
            assert torch.equal(x, y), tag
        assert gr[5].dtype == torch.float32 and gr[5].shape == (P, 16, 3)
        for x, y, nm in zip(gr, base[1], rr.GRAD_NAMES):
            assert not torch.isnan(x).any(), (tag, nm)
            worst = max(worst, rel_err(x.cpu().numpy(), y.cpu().numpy().astype(np.float64)))
        print(f"{tag}: worst gradient difference to the fp32 path {worst:.2e}")
        for x, y, nm in zip(gr, base[1], rr.GRAD_NAMES):
            if det:
                assert torch.equal(x, y), (tag, nm)
            else:   # atomics sum in arbitrary order: equal to rounding
                util.assert_close(f"{tag} {nm}", x.cpu().numpy(), y.cpu().numpy(), tol=2e-5, max_bad_frac=1e-4)
        sc.assert_inactive_zero(tag, gr[5].cpu().numpy(), o[4].cpu().numpy(), D)
    sc.assert_inactive_zero("float", base[1][5].cpu().numpy(), base[0][4].cpu().numpy(), D)
    assert float(base[1][5][:, :n].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ (e) sessions, fused losses
def _session_inputs(s):
    d, g, cam = util.to_dev, s.g, s.cam
    params = dict(means3D=d(g["means3D"]), shs=d(g["shs"]), opacities=d(g["opacities"]), scales=d(g["scales"]),
                  rotations=d(g["rotations"]))
    camd = dict(cam, viewmatrix=d(cam["viewmatrix"]), projmatrix=d(cam["projmatrix"]), campos=d(cam["campos"]))
    rng = np.random.default_rng(2)
    H, W = cam["H"], cam["W"]
    gt = d(rng.uniform(0, 1, (3, H, W)).astype(np.float32))
    mask = d((rng.uniform(0, 1, (1, H, W)) > 0.5).astype(np.float32))
    return params, camd, d(BG), gt, mask


def _raw_step(params, camd, bg, D, image_grads, extra=None, grads_extra=None):
    """The raw bindings at degree D: image_grads(color, alpha, out_extra) -> (dL_dcolor, dL_ddepth, dL_dalpha)."""
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    e = torch.empty(0)
    H, W = camd["H"], camd["W"]
    o = _C.rasterize_gaussians(bg, params["means3D"], e, params["opacities"], params["scales"], params["rotations"], 1.0, e,
                               camd["viewmatrix"], camd["projmatrix"], camd["tanfovx"], camd["tanfovy"], H, W, params["shs"], D,
                               camd["campos"], False, False, extra=extra)
    dc, dd, da = image_grads(o[1], o[3], o[8] if extra is not None else None)
    kw = {} if extra is None else dict(extra=extra, dL_dout_extra=grads_extra(o[1], o[3], o[8]))
    gr = _C.rasterize_gaussians_backward(bg, params["means3D"], o[4], e, params["scales"], params["rotations"], 1.0, e,
                                         camd["viewmatrix"], camd["projmatrix"], camd["tanfovx"], camd["tanfovy"], dc, dd, da,
                                         params["shs"], D, camd["campos"], o[5], o[0], o[6], o[7], o[3], False, **kw)
    return o, dict(means3D=gr[3], sh=gr[5], opacity=gr[2], scales=gr[6], rotations=gr[7], extra=gr[8] if extra is not None else None)


def _check_step(tag, grads, want, D, radii):
    n = (D + 1) ** 2
    worst = max(rel_err(grads[k].cpu().numpy(), want[k].cpu().numpy().astype(np.float64)) for k in ("means3D", "sh", "opacity", "scales", "rotations"))
    print(f"{tag} D={D}: worst gradient difference to the raw binding {worst:.2e}")
    for k in ("means3D", "sh", "opacity", "scales", "rotations"):
        util.assert_close(f"{tag} {k}", grads[k].cpu().numpy(), want[k].cpu().numpy(), tol=2e-5, max_bad_frac=1e-4)
    sh = grads["sh"].cpu().numpy()
    assert float(np.abs(sh[:, :n]).max()) > 0
    sc.assert_inactive_zero(tag, sh, radii.cpu().numpy(), D)


def _alpha_mask_grads(gt, mask):
    def f(color, alpha, _extra):
        return torch.sign(color - gt) / color.numel(), torch.zeros_like(alpha), 0.2 * (alpha - mask) / alpha.numel()
    return f


@pytest.mark.parametrize("D", [0, 1, 2])
@pytest.mark.parametrize("entry", ["session", "alpha_mask_loss", "view_parallel_plain", "view_parallel_compact"])
def test_reused_buffers_after_a_step_at_degree_3(oracle, entry, D):
    """Each object runs one step at degree 3 -- which leaves gradients in all sixteen rows of its SH buffer -- and then the step at D
    in the same buffers: nothing clears them but the kernels."""
    from mygauhuman_amd import parallel
    from mygauhuman_amd.fastpath import RasterSession
    P0 = sc.SCENES["p600"][0]
    s = sc.reference(oracle, "p600", P0, 16, D)
    params, camd, bg, gt, mask = _session_inputs(s)
    H, W = camd["H"], camd["W"]
    n = s.n_active
    if entry == "session":
        up = tuple(util.to_dev(x) for x in s.up)
        o, want = _raw_step(params, camd, bg, D, lambda c, a, x: up)
    else:
        o, want = _raw_step(params, camd, bg, D, _alpha_mask_grads(gt, mask))
    if entry in ("session", "alpha_mask_loss"):
        R3 = _raw_step(params, camd, bg, 3, _alpha_mask_grads(gt, mask))[0][0]
        ses = RasterSession(P0, W, H, 16, "cuda", capacity=max(o[0], R3) + 1000)
        out = {k: torch.full(v.shape, float("nan"), device="cuda") for k, v in want.items() if v is not None}
        for deg in (3, D):
            col, dep, alp, rad = ses.forward(params, camd, bg, deg)
            if entry == "session":
                ses.backward(params, camd, bg, deg, up[0], up[1], up[2], out)
            else:
                ses.backward_alpha_mask_loss(params, camd, bg, deg, gt, mask, 0.1, out)
            if deg == 3:
                assert float(out["sh"][:, n:].abs().max()) > 0   # the stale values the next step has to clear
        assert not ses.overflowed()
        grads = out
    else:
        step = parallel.ViewParallelStep(params, 3, camd, bg, compact_sh=(entry == "view_parallel_compact"))
        step(camd, bg, gt, mask, reduce=False)
        assert float(step.grads["sh"][:, n:].abs().max()) > 0
        step.deg = D
        col, alp, rad = step(camd, bg, gt, mask, reduce=False)
        step.check()
        dep, grads = None, step.grads
        if step.compact is not None:   # the exchange of the own view: pack -> reconstruct at degree D over the stale buffer
            plain = grads["sh"].clone()
            step.compact.pack(step.session, camd["campos"])
            step.compact.local()
            rebuilt = step.compact.reconstruct(params["means3D"], D, n_views=1)
            assert rebuilt.data_ptr() == grads["sh"].data_ptr()
            sc.assert_inactive_zero("reconstruct", rebuilt.cpu().numpy(), rad.cpu().numpy(), D)
            util.assert_close("reconstruct", rebuilt.cpu().numpy(), plain.cpu().numpy(), tol=2e-6)
    assert torch.equal(col, o[1]) and torch.equal(alp, o[3]) and torch.equal(rad, o[4])
    if dep is not None:
        assert torch.equal(dep, o[2])
    _check_step(entry, grads, want, D, rad)


@pytest.mark.parametrize("D", [0, 1, 2])
def test_phase1_loss_backward_below_the_stored_degree(oracle, D):
    """gsr_rasterize_backward_phase1_loss with SH input at M = 16: the loss gradient formed inside the blend backward against the
    same loss written with torch ops on the forward's images, fed to the plain backward."""
    from mygauhuman_amd import _lib
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    P0 = sc.SCENES["p600"][0]
    s = sc.reference(oracle, "p600", P0, 16, D)
    params, camd, bg, gt, mask = _session_inputs(s)
    H, W = camd["H"], camd["W"]
    rng = np.random.default_rng(8)
    gt_normal = util.to_dev(rng.uniform(0, 1, (3, H, W)).astype(np.float32))
    bound_np = np.zeros((1, H, W), np.float32)
    bound_np[:, H // 6: H - H // 8, W // 5: W - W // 7] = 1.0
    bound_np *= rng.uniform(0, 1, (1, H, W)) > 0.1
    bound = util.to_dev(bound_np)
    extra = util.to_dev(rng.uniform(0, 1, (P0, _lib.N_EXTRA)).astype(np.float32))
    spec = _C.Phase1Loss(gt, gt_normal, mask, bound)
    cache = {}

    def torch_loss(color, alpha, out_extra):
        c, a, x = (t.detach().clone().requires_grad_(True) for t in (color, alpha, out_extra))
        bm = bound[0] == 1
        l1 = lambda p, q: torch.abs(p.permute(1, 2, 0)[bm] - q.permute(1, 2, 0)[bm]).mean()  # noqa: E731
        loss = l1(c, gt) + 0.1 * ((a[bound == 1] - mask[bound == 1]) ** 2).mean() + l1(x[0:3], gt_normal) + l1(x[15:18], gt_normal)
        cache["loss"] = loss.detach()
        cache["g"] = torch.autograd.grad(loss, (c, a, x))
        return cache["g"][0], torch.zeros_like(alpha), cache["g"][1]

    o, want = _raw_step(params, camd, bg, D, torch_loss, extra=extra, grads_extra=lambda c, a, x: cache["g"][2].contiguous())
    e = torch.empty(0)
    for deg in (3, D):
        f = _C.rasterize_gaussians(bg, params["means3D"], e, params["opacities"], params["scales"], params["rotations"], 1.0, e,
                                   camd["viewmatrix"], camd["projmatrix"], camd["tanfovx"], camd["tanfovy"], H, W, params["shs"], deg,
                                   camd["campos"], False, False, extra=extra)
        loss, stats = _C.phase1_loss_forward(spec, f[1], f[3], f[8])
        gr = _C.rasterize_gaussians_backward(bg, params["means3D"], f[4], e, params["scales"], params["rotations"], 1.0, e,
                                             camd["viewmatrix"], camd["projmatrix"], camd["tanfovx"], camd["tanfovy"], None, None,
                                             None, params["shs"], deg, camd["campos"], f[5], f[0], f[6], f[7], f[3], False,
                                             extra=extra, dL_dout_extra=[None] * (_lib.N_EXTRA // 3),
                                             phase1=(spec, stats, None, f[1], f[8]))
    assert torch.equal(f[1], o[1]) and torch.equal(f[3], o[3]) and torch.equal(f[4], o[4]) and torch.equal(f[8], o[8])
    np.testing.assert_allclose(float(loss), float(cache["loss"]), rtol=2e-6)
    grads = dict(means3D=gr[3], sh=gr[5], opacity=gr[2], scales=gr[6], rotations=gr[7])
    _check_step("phase1_loss", grads, want, D, f[4])
    util.assert_close("phase1_loss extra", gr[8].cpu().numpy(), want["extra"].cpu().numpy(), tol=2e-5, max_bad_frac=1e-4)


# ------------------------------------------------------------------------------------------ (f) compact exchange, real backward
@pytest.mark.parametrize("D,n_views", [(0, 2), (1, 3), (2, 2)])
def test_compact_exchange_below_the_stored_degree(D, n_views):
    """pack -> gsr_sh_grad_from_views after real backwards of `n_views` cameras at D < 3, M = 16, against the plain per-view dL_dsh
    under the measured rule: the branch of test_gpu_parallel.py that its own scenes (M == (D + 1)^2) never take."""
    from tests.test_gpu_parallel import compact_exchange_case
    P0 = sc.SCENES["p600"][0]
    cam, g = sc.scene("p600", P0, 16, D)
    assert g["shs"].shape[1] > (D + 1) ** 2
    compact_exchange_case(cam, g, D, n_views)


# ----------------------------------------------------------------------------------------------------------------- (g) render()
_ORACLE_RENDER = {}
IMAGE_KEYS = ("render", "normal", "albedo", "occlusion", "roughness", "world_normal", "render_axis", "render_alpha")


@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("sh_python", [True, False], ids=["attribute_kernel", "rasterizer_sh"])
def test_render_at_an_active_degree_below_the_stored_one(oracle, d, sh_python):
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.optim import FusedAdam
    from tests.test_gpu_render import _human_scene, _oracle_render
    s = _human_scene(oracle)
    model = s.model
    model.active_sh_degree = d
    assert model.max_sh_degree == 3 and model._features_rest.shape[1] == 15
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    if d not in _ORACLE_RENDER:   # the oracle composition of this (seeded) scene at degree d: once for both SH routes
        _ORACLE_RENDER[d] = _oracle_render(oracle, s, bg, deg=d)[0]
    ref = _ORACLE_RENDER[d]
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=sh_python)
    out = render(1, s.cam, model, pipe, util.to_dev(bg))
    # ---- the bounds of test_render_matches_oracle_composition_and_contract
    assert float((ref["pre"]["radii"] > 0).mean()) > 0.9
    assert float((out["radii"].cpu().numpy() == ref["pre"]["radii"]).mean()) > 0.995
    diff = np.abs(out["render"].detach().cpu().numpy() - ref["img"]["color"])
    adiff = np.abs(out["render_alpha"].detach().cpu().numpy() - ref["img"]["alpha"])
    print(f"render d={d}: colour p99.9 {np.percentile(diff, 99.9):.2e} mean {diff.mean():.2e}; alpha p99.9 "
          f"{np.percentile(adiff, 99.9):.2e} mean {adiff.mean():.2e}")
    assert np.percentile(diff, 99.9) < 2e-3 and diff.mean() < 5e-5, (diff.max(), diff.mean())
    assert np.percentile(adiff, 99.9) < 2e-3 and adiff.mean() < 5e-5
    # ---- gradients: only the active rows of the SH parameters receive one
    sum(out[k].mean() * (i + 1) for i, k in enumerate(IMAGE_KEYS)).backward()
    n_rest = (d + 1) ** 2 - 1
    g_dc, g_rest = model._features_dc.grad, model._features_rest.grad
    assert g_dc is not None and torch.isfinite(g_dc).all() and float(g_dc.abs().max()) > 0
    assert g_rest is not None and not torch.isnan(g_rest).any()
    assert float(g_rest[:, n_rest:].abs().max()) == 0.0, float(g_rest[:, n_rest:].abs().max())
    if d >= 1:
        assert float(g_rest[:, :n_rest].abs().max()) > 0
    fused = [p.grad.detach().clone() for p in model.parameters()]
    fused_img = {k: out[k].detach().cpu().numpy() for k in IMAGE_KEYS + ("render_depth",)}
    # ---- fused (one activation kernel, the SH tensors in place) against the property getters (torch ops)
    for p in model.parameters():
        p.grad = None
    o2 = render(1, s.cam, util.GetterOnlyModel(model), pipe, util.to_dev(bg))
    sum(o2[k].mean() * (i + 1) for i, k in enumerate(IMAGE_KEYS)).backward()
    for k in fused_img:
        np.testing.assert_allclose(fused_img[k], o2[k].detach().cpu().numpy(), atol=3e-5, err_msg=k)
    for ga, p in zip(fused, model.parameters()):
        util.assert_close("render grads", ga.cpu().numpy(), p.grad.cpu().numpy(), tol=1e-4, max_bad_frac=2e-4)
    assert float(model._features_rest.grad[:, n_rest:].abs().max()) == 0.0
    # ---- one FusedAdam step on the fused path's gradients: the inactive rows do not move and gather no moments
    rest = model._features_rest
    rest.grad = fused[2]
    before = rest.detach().clone()
    opt = FusedAdam([dict(params=[rest], lr=1e-2)], lr=0.0, eps=1e-15)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(rest.detach()[:, n_rest:], before[:, n_rest:])
    st = opt.state[rest]
    assert float(st["exp_avg"][:, n_rest:].abs().max()) == 0.0 and float(st["exp_avg_sq"][:, n_rest:].abs().max()) == 0.0
    if d >= 1:
        assert not torch.equal(rest.detach()[:, :n_rest], before[:, :n_rest]) and float(st["exp_avg"][:, :n_rest].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------- (h) scale modifier
@pytest.mark.parametrize("name,P", FULL, ids=[n for n, _ in FULL])
@pytest.mark.parametrize("m", sc.MODIFIERS)
@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "deterministic"])
def test_scale_modifier_against_the_oracle_and_its_identity(oracle, name, P, m, det):
    """The reference kernel's convention (test_sh_degree_host.py holds the oracle and the restatement to it): the covariance is
    built from float32(m) * s, and dL_dscales is the gradient with respect to that product -- no factor of m.  So modifier m on
    scales s == modifier 1 on float32(m) * s, in every bit of the forward and, with the fixed-order reduction, of the backward."""
    from mygauhuman_amd import _lib
    s = sc.reference(oracle, name, P, 16, 3, modifier=m)
    g1 = dict(s.g, scales=(np.float32(m) * s.g["scales"]).astype(np.float32))
    _lib.set_tuning("deterministic", det)
    try:
        f = forward(s, modifier=m)
        got = util.hip_backward(f, *s.up, debug=True, scale_modifier=m)
        f1 = forward(s, g=g1)
        got1 = util.hip_backward(f1, *s.up, debug=True)
    finally:
        _lib.set_tuning("deterministic", 0)
    check_forward(s, f, {})
    np.testing.assert_array_equal(util.hip_query(f, "COV3D")[s.visible], s.ref["pre"]["cov3D"][s.visible])
    check_backward(s, got, {})
    a, b = forward_state(f), forward_state(f1)
    a["COV3D"], b["COV3D"] = util.hip_query(f, "COV3D")[s.visible], util.hip_query(f1, "COV3D")[s.visible]
    assert_same_bits("modifier identity, forward", a, b)
    assert float(np.abs(got["dL_dscales"]).max()) > 0
    worst = max(rel_err(got[n], got1[n].astype(np.float64)) for n in GRADS)
    print(f"modifier {m}: worst gradient difference to modifier 1 on m * scales {worst:.2e}")
    for n in GRADS:
        if det:
            assert sc.bits_equal(got[n], got1[n]), n
        else:
            util.assert_close(n + " (identity)", got[n], got1[n], tol=2e-5, max_bad_frac=1e-4)


# --------------------------------------------------------------------------------------------------------------- the graph
def test_graphed_render_step_is_captured_again_after_oneup_sh_degree(oracle):
    """The active SH degree is a by-value kernel argument: a GraphedFrame captured at degree 1 keeps replaying degree 1 after
    oneupSHdegree(); a new capture reproduces the eager step at degree 2.  The bound is the frame's own (verify_rtol of each
    tensor's largest magnitude, what its self-check holds a replay to)."""
    import inspect

    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.graph import GraphedFrame
    from tests.test_gpu_render import _human_scene
    rtol = inspect.signature(GraphedFrame.__init__).parameters["verify_rtol"].default
    s = _human_scene(oracle, seed=11)
    model = s.model
    model.active_sh_degree = 1
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = util.to_dev(np.array([0.2, 0.3, 0.1], np.float32))
    params = list(model.parameters())
    keys = ("render", "render_alpha", "normal", "render_axis")

    def step():
        o = render(1, s.cam, model, pipe, bg)
        sum(o[k].mean() for k in keys).backward()
        return o

    def eager():
        for p in params:
            p.grad = None
        o = step()
        return o["render"].detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

    def far(a, b):
        return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)

    def check(frame, img_e, grads_e, n_rest):
        out = frame.replay()
        torch.cuda.synchronize()
        frame.check()
        assert far(out["render"].detach(), img_e) <= rtol
        for p, ge in zip(params, grads_e):
            if ge is not None:
                assert far(p.grad, ge) <= rtol
        assert float(model._features_rest.grad[:, n_rest:].abs().max()) == 0.0
        assert float(model._features_rest.grad[:, :n_rest].abs().max()) > 0

    frame = GraphedFrame(step, warmup=3, zero_grads=params)
    img1, grads1 = eager()
    check(frame, img1, grads1, 3)
    model.oneupSHdegree()
    assert model.active_sh_degree == 2
    img2, grads2 = eager()
    assert far(img2, img1) > 10 * rtol and far(grads2[2], grads1[2]) > 10 * rtol   # the two degrees are told apart by the bound
    check(frame, img1, grads1, 3)    # the old capture still renders degree 1: the degree was baked in by value
    frame = GraphedFrame(step, warmup=3, zero_grads=params)
    check(frame, img2, grads2, 8)
