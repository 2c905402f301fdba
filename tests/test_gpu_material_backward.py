"""The materials-only backward of the frozen-geometry PBR phase (csrc/blend_colors_bwd.hip, gsr_rasterize_backward_colors):
the raw entry point against the CPU oracle and the float64 restatement on the scenes of tests/material_backward_cases.py under
every binning back-end, tile order and segment setting; against the library's own full backward on the same frame (and the full
backward's rows contract afterwards); render(geometry_grad=False / "auto"); the whole PBR training step, eager and as a
GraphedFrame, with a FusedAdam step; guard bands around the two outputs."""
import types

import numpy as np
import pytest
import torch

from tests import material_backward_cases as mc
from tests import util
from tests.test_raster_reference_host import BG

pytestmark = pytest.mark.gpu


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _forward(cam, g, extra, bg=BG):
    """The fused 18-channel forward through the raw binding, precomputed colours and covariance."""
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    e = torch.empty(0)
    d = util.to_dev
    a = types.SimpleNamespace(bg=d(bg), means3D=d(g["means3D"]), colors=d(g["colors"]), opac=d(g["opacities"]), cov=d(g["cov3D"]),
                              view=d(cam["viewmatrix"]), proj=d(cam["projmatrix"]), campos=d(cam["campos"]), extra=d(extra), cam=cam)
    out = _C.rasterize_gaussians(a.bg, a.means3D, a.colors, a.opac, e, e, 1.0, a.cov, a.view, a.proj, cam["tanfovx"], cam["tanfovy"],
                                 cam["H"], cam["W"], e, 0, a.campos, False, False, extra=a.extra)
    a.R, a.color, a.depth, a.alpha, a.radii, a.geom, a.bin, a.img, a.out_extra = out
    a.P, a.W, a.H = a.means3D.shape[0], cam["W"], cam["H"]
    return a


def _images(c):
    """(main colour gradient image, the six triples' images with None for the null ones) on the device."""
    return util.to_dev(c.grads[mc.MAIN]), [util.to_dev(c.grads[t]) if t in mc.LIVE_TRIPLES else None for t in range(6)]


def _colors_backward(f, main, triples):
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    return _C.rasterize_gaussians_backward_colors(f.P, f.R, f.H, f.W, f.geom, f.bin, f.img, main, triples)


def _full_backward(f, main, triples):
    """gsr_rasterize_backward_ex on the same buffers: (dL_dcolors, dL_dextra) with zero depth and alpha upstreams."""
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    e = torch.empty(0)
    z = torch.zeros((1, f.H, f.W), device="cuda")
    out = _C.rasterize_gaussians_backward(f.bg, f.means3D, f.radii, f.colors, e, e, 1.0, f.cov, f.view, f.proj, f.cam["tanfovx"],
                                          f.cam["tanfovy"], main, z, z, e, 0, f.campos, f.geom, f.R, f.bin, f.img, f.alpha, False,
                                          extra=f.extra, dL_dout_extra=triples)
    return out[1], out[8]


@pytest.fixture
def knobs(request):
    """(binning back-end, blend_segments, tile_order) as process defaults for one test."""
    from mygauhuman_amd import _lib
    binning, seg, order = request.param
    _lib.check(_lib.lib.gsr_set_binning_mode(_lib.BINNING_GLOBAL_RADIX if binning == "radix" else _lib.BINNING_TILE_BUCKET),
               "gsr_set_binning_mode")
    util.set_tile_cull(binning == "bucket_tight")
    _lib.set_tuning("tile_order", order)
    _lib.set_tuning("blend_segments", seg)
    yield request.param
    _lib.lib.gsr_set_binning_mode(_lib.DEFAULT_BINNING)
    util.set_tile_cull(_lib.DEFAULT_TILE_CULL)
    _lib.set_tuning("tile_order", _lib.DEFAULT_TILE_ORDER)
    _lib.set_tuning("blend_segments", _lib.DEFAULT_BLEND_SEGMENTS)


DEFAULT = ("bucket_tight", 8, 1)
SWEPT = ("general", "stack_translucent", "stack_opaque")
PARITY = [(n, DEFAULT) for n in mc.NAMES if n not in SWEPT]
PARITY += [(n, (b, seg, 1)) for n in SWEPT for b in ("radix", "bucket", "bucket_tight") for seg in (0, 8)]
PARITY += [("stack_translucent", ("bucket_tight", 0, order)) for order in (0, 2, 3)]


# ---- 1. the raw entry point against the oracle and float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("name,knobs", PARITY, indirect=["knobs"], ids=[f"{n}-{k[0]}-seg{k[1]}-order{k[2]}" for n, k in PARITY])
def test_entry_point_against_oracle_and_float64(oracle, name, knobs):
    c = mc.case(oracle, name)
    f = _forward(c.cam, c.g, c.extra)
    np.testing.assert_array_equal(f.radii.cpu().numpy(), c.ref["pre"]["radii"])
    main, triples = _images(c)
    d_color, d_extra = _colors_backward(f, main, triples)
    d_color, d_extra = d_color.cpu().numpy(), d_extra.cpu().numpy()
    assert d_color.shape == (c.P, 3) and d_extra.shape == (c.P, 18)
    for t in range(6):
        if t not in mc.LIVE_TRIPLES:   # a null image: exactly zero, not merely small
            assert not d_extra[:, 3 * t:3 * t + 3].any(), f"triple {t} received no gradient image"
    culled = c.ref["pre"]["radii"] == 0
    assert not d_color[culled].any() and not d_extra[culled].any()
    if name == "stack_tail":
        ranges = util.hip_query(dict(P=f.P, R=f.R, W=f.W, H=f.H, geom=f.geom, bin=f.bin, img=f.img), "RANGES").reshape(-1, 2)
        assert (ranges[:, 0] == ranges[:, 1]).any() and (c.lists == 0).any(), "the scene is meant to have tiles with empty lists"
    if name.startswith("stack"):
        assert c.lists.max() > 1024   # beyond the 512-entry sort limit and the segment threshold
    for i in mc.LIVE_TRIPLES + (mc.MAIN,):
        got = d_color if i == mc.MAIN else d_extra[:, 3 * i:3 * i + 3]
        t32, t64, frac = mc.bounds(name, got.size)
        util.assert_close(f"{name} image {i}", got, c.want[i], tol=t32, max_bad_frac=frac, outer_tol=10 * t32)
        util.assert_close(f"{name} image {i} vs float64", got, c.want64[i], tol=t64, max_bad_frac=frac, outer_tol=10 * t64)


# ---- 2. against the library's own full backward ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general", "opaque", "stack_translucent", "stack_opaque", "stack_tail"])
def test_matches_the_full_backward_and_leaves_its_rows_alone(oracle, name):
    c = mc.case(oracle, name)
    f = _forward(c.cam, c.g, c.extra)
    main, triples = _images(c)
    full_color, full_extra = _full_backward(f, main, triples)
    d_color, d_extra = _colors_backward(f, main, triples)
    util.assert_close("dL_dcolor", d_color.cpu().numpy(), full_color.cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)
    util.assert_close("dL_dextra", d_extra.cpu().numpy(), full_extra.cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)
    # the full backward again, on the same buffers: the colour-only call left its accumulation rows as it found them
    again_color, again_extra = _full_backward(f, main, triples)
    util.assert_close("dL_dcolor again", again_color.cpu().numpy(), full_color.cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)
    util.assert_close("dL_dextra again", again_extra.cpu().numpy(), full_extra.cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)


def test_rows_contract_survives_between_flagged_backwards(oracle):
    """GSR_FWD_ZERO_ROWS / GSR_BWD_ROWS_ZEROED: rows zero on entry, zero on exit.  A colour-only call between two flagged full
    backwards must not disturb it (it never touches the rows)."""
    import ctypes as C
    from mygauhuman_amd import _lib
    from mygauhuman_amd._lib import call, lib, ptr
    c = mc.case(oracle, "general")
    d = util.to_dev
    cam, g = c.cam, c.g
    P, W, H = c.P, mc.W, mc.H
    dev = torch.device("cuda")
    t = dict(bg=d(BG), means3D=d(g["means3D"]), colors=d(g["colors"]), opac=d(g["opacities"]), cov=d(g["cov3D"]),
             view=d(cam["viewmatrix"]), proj=d(cam["projmatrix"]), campos=d(cam["campos"]), extra=d(c.extra))
    cap = 1 << 16
    geom = torch.empty(lib.gsr_geometry_bytes(P), dtype=torch.uint8, device=dev)
    img = torch.empty(lib.gsr_image_bytes(W, H), dtype=torch.uint8, device=dev)
    binb = torch.empty(lib.gsr_binning_bytes(cap, W, H), dtype=torch.uint8, device=dev)
    color, depth, alpha = (torch.empty((k, H, W), device=dev) for k in (3, 1, 1))
    out_extra = torch.empty((18, H, W), device=dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    call("gsr_rasterize_forward_async_ex", dev, geom.data_ptr(), binb.data_ptr(), cap, img.data_ptr(), P, 0, 0, ptr(t["bg"]), W, H,
         ptr(t["means3D"]), None, ptr(t["colors"]), ptr(t["opac"]), None, 1.0, None, ptr(t["cov"]), ptr(t["view"]), ptr(t["proj"]),
         ptr(t["campos"]), float(cam["tanfovx"]), float(cam["tanfovy"]), 0, ptr(color), ptr(depth), ptr(alpha), ptr(radii), 2,   # GSR_FWD_ZERO_ROWS
         ptr(status), ptr(t["extra"]), 18, ptr(out_extra), _lib.SH_F32)
    assert int(status[1]) == 0
    main, triples = _images(c)
    z = torch.zeros((1, H, W), device=dev)
    ptrs = (C.c_void_p * 6)(*[None if x is None else x.data_ptr() for x in triples])

    def flagged_full():
        o = {k: torch.empty(s, device=dev) for k, s in dict(m2=(P, 3), conic=(P, 4), op=(P, 1), col=(P, 3), m3=(P, 3), cov=(P, 6),
                                                            ex=(P, 18)).items()}
        call("gsr_rasterize_backward_ex", dev, P, 0, 0, cap, ptr(t["bg"]), W, H, ptr(t["means3D"]), None, ptr(t["colors"]), ptr(alpha),
             None, 1.0, None, ptr(t["cov"]), ptr(t["view"]), ptr(t["proj"]), ptr(t["campos"]), float(cam["tanfovx"]), float(cam["tanfovy"]),
             ptr(radii), geom.data_ptr(), binb.data_ptr(), img.data_ptr(), ptr(main), ptr(z), ptr(z), ptr(o["m2"]), ptr(o["conic"]),
             ptr(o["op"]), ptr(o["col"]), ptr(o["m3"]), ptr(o["cov"]), None, None, None, 2,   # GSR_BWD_ROWS_ZEROED
             ptr(t["extra"]), 18, ptrs, ptr(o["ex"]), _lib.SH_F32)
        return o

    first = flagged_full()
    d_color, d_extra = torch.empty((P, 3), device=dev), torch.empty((P, 18), device=dev)
    call("gsr_rasterize_backward_colors", dev, P, cap, W, H, geom.data_ptr(), binb.data_ptr(), img.data_ptr(), ptr(main), ptr(d_color),
         18, ptrs, ptr(d_extra), 0)
    second = flagged_full()
    util.assert_close("dL_dextra", d_extra.cpu().numpy(), first["ex"].cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)
    for k in first:
        util.assert_close(f"flagged full backward, {k}", second[k].cpu().numpy(), first[k].cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)


def test_deterministic_mode_is_refused(oracle):
    from mygauhuman_amd import _lib
    c = mc.case(oracle, "general")
    f = _forward(c.cam, c.g, c.extra)
    main, triples = _images(c)
    _lib.set_tuning("deterministic", 1)
    try:
        with pytest.raises(_lib.GsrError, match=r"gsr_rasterize_backward_colors failed \(-1\)"):
            _colors_backward(f, main, triples)
    finally:
        _lib.set_tuning("deterministic", 0)


def test_plain_forward_and_single_images(oracle):
    """After the plain forward (no extra channels: its workgroups sort the short lists themselves) the main colour alone; and the
    fused forward with one triple alone and no main colour: outputs that were not asked for come back as None."""
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    c = mc.case(oracle, "general")
    f = util.hip_forward(c.cam, c.g, BG, "precomp")
    main, triples = _images(c)
    d_color, d_extra = _C.rasterize_gaussians_backward_colors(f["P"], f["R"], f["H"], f["W"], f["geom"], f["bin"], f["img"], main, None)
    assert d_extra is None
    t32, t64, frac = mc.bounds("general", d_color.numel())
    util.assert_close("main colour, plain forward", d_color.cpu().numpy(), c.want64[mc.MAIN], tol=t64, max_bad_frac=frac, outer_tol=10 * t64)
    ff = _forward(c.cam, c.g, c.extra)
    d_color, d_extra = _colors_backward(ff, None, [triples[0] if t == 0 else None for t in range(6)])
    assert d_color is None and not d_extra[:, 3:].any()
    util.assert_close("triple 0 alone", d_extra[:, :3].cpu().numpy(), c.want64[0], tol=t64, max_bad_frac=frac, outer_tol=10 * t64)


# ---- 3. render() ---------------------------------------------------------------------------------------------------------------------
GEOMETRY = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
MATERIALS = ("_albedo", "_roughness", "_normal")


def _render_scene():
    """The synthetic human with a baked camera, as tests/test_gpu_pbr_loss._pbr_scene builds it."""
    from tests.test_gpu_pbr_loss import _pbr_scene
    return _pbr_scene()


def _render_loss(s, o):
    return sum((o[k] * w).sum() for k, w in zip(("albedo", "roughness", "normal"), s.weights))


def _leaf_grads(model, names):
    return {n: (None if getattr(model, n).grad is None else getattr(model, n).grad.detach().clone()) for n in names}


def _clear(model):
    for n in GEOMETRY + MATERIALS:
        getattr(model, n).grad = None


def _stages():
    from mygauhuman_amd import _lib
    r = _lib.profile_read()
    return r["blend_bwd"][1], r["preprocess_bwd"][1], r["blend_bwd_colors"][1]


def test_render_materials_only(oracle):
    from mygauhuman_amd import _lib
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    try:
        s = _render_scene()
        gen = torch.Generator(device="cuda").manual_seed(3)
        s.weights = [torch.randn((3, s.H, s.W), device="cuda", generator=gen) for _ in range(3)]
        m = s.model
        assert gr.GEOMETRY_GRAD is True
        # ---- the full path, then the short one: same images, same material gradients
        _clear(m)
        full = gr.render(30001, s.cam, m, s.pipe, s.bg, envmap=s.env)
        _render_loss(s, full).backward()
        want = _leaf_grads(m, MATERIALS)
        assert full["viewspace_points"].grad is not None and m._xyz.grad is not None
        _clear(m)
        _lib.profile_enable(_lib.PROF_STAGES)
        try:
            short = gr.render(30001, s.cam, m, s.pipe, s.bg, envmap=s.env, geometry_grad=False)
            for k in gr.RESULT_KEYS:
                a, b = short[k], full[k]
                if isinstance(b, torch.Tensor) and k != "viewspace_points":
                    assert torch.equal(a.detach(), b.detach()), f"forward result {k} differs"
            _render_loss(s, short).backward()
            torch.cuda.synchronize()
            bwd, pre, colors = _stages()
        finally:
            _lib.profile_enable([])
        assert bwd == 0 and pre == 0 and colors >= 1, (bwd, pre, colors)
        got = _leaf_grads(m, MATERIALS)
        for n in MATERIALS:
            assert (got[n] is None) == (want[n] is None), n
            if want[n] is not None:
                assert float(want[n].abs().sum()) > 0, n
                util.assert_close(n, got[n].cpu().numpy(), want[n].cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)
        # (get_roughness reads _albedo, scene/gaussian_model.py:197-199: _roughness itself is reached by neither path)
        assert want["_albedo"] is not None and want["_normal"] is not None and want["_roughness"] is None
        for n in GEOMETRY:
            assert getattr(m, n).grad is None, n
        for net in (m.pose_decoder, m.lweight_offset_decoder):
            assert net is None or all(p.grad is None for p in net.parameters())
        assert short["viewspace_points"].grad is None and short["viewspace_points"].requires_grad
        # ---- "auto": the full path while one geometry leaf trains, the short one once all are frozen
        for frozen in (False, True):
            _clear(m)
            for n in GEOMETRY:
                getattr(m, n).requires_grad_(not frozen and n == "_opacity")
            assert gr.geometry_frozen(m) is frozen
            _lib.profile_enable(_lib.PROF_STAGES)
            try:
                o = gr.render(30001, s.cam, m, s.pipe, s.bg, envmap=s.env, geometry_grad="auto")
                (_render_loss(s, o) + (0.0 if frozen else o["render_alpha"].sum())).backward()
                torch.cuda.synchronize()
                bwd, pre, colors = _stages()
            finally:
                _lib.profile_enable([])
            if frozen:
                assert (bwd, pre) == (0, 0) and colors >= 1
                assert o["viewspace_points"].grad is None
            else:
                assert bwd >= 1 and pre >= 1 and colors == 0
                assert o["viewspace_points"].grad is not None and m._opacity.grad is not None
            util.assert_close(f"_albedo, auto, frozen={frozen}", m._albedo.grad.cpu().numpy(), want["_albedo"].cpu().numpy(), tol=1e-4,
                              max_bad_frac=1e-4)
        # ---- the module switch is what None reads
        gr.GEOMETRY_GRAD = "auto"
        _clear(m)
        o = gr.render(30001, s.cam, m, s.pipe, s.bg, envmap=s.env)
        _render_loss(s, o).backward()
        assert o["viewspace_points"].grad is None and m._albedo.grad is not None
        # ---- what the short path cannot carry
        spec = _C.Phase1Loss(s.gt, s.gt, s.bound, s.bound)
        with pytest.raises(ValueError, match="fused_loss"):
            gr.render(30001, s.cam, m, s.pipe, s.bg, envmap=s.env, fused_loss=spec, geometry_grad=False)
    finally:
        gr.BAKE = False
        gr.GEOMETRY_GRAD = True


def test_render_materials_only_with_motion_decoders():
    """motion_offset_flag=True, the reference's training configuration: a pose decoder and a skinning-offset decoder with trainable
    parameters feed the deform.  The short path runs them without a graph: same images, the material gradients of the full path
    (also on the world-normal image, through world_normal = R n with this branch's transforms, and with cached transforms), an
    envmap that requires grad is reached through the occlusion image, no decoder parameter gets a gradient, and "auto" waits for
    the decoders' parameters too."""
    from mygauhuman_amd import gaussian_renderer as gr
    from tests.test_gpu_render import _human_scene
    s = _human_scene(None, seed=7, motion=True)

    class PoseDec(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(3)
            self.delta = torch.nn.Parameter(0.02 * torch.randn((23, 3, 3), generator=g).cuda())

        def forward(self, posevec):
            return {"Rs": (torch.eye(3, device="cuda")[None] + self.delta)[None]}

    class WDec(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1, 24, 1, device="cuda"))

        def forward(self, pts):
            return self.w.expand(1, 24, pts.shape[1])

    m = s.model
    m.pose_decoder, m.lweight_offset_decoder = PoseDec(), WDec()
    assert m.motion_offset_flag
    decoder_params = list(m.pose_decoder.parameters()) + list(m.lweight_offset_decoder.parameters())
    P, H, W = m._xyz.shape[0], s.cam_np["H"], s.cam_np["W"]
    gen = torch.Generator(device="cuda").manual_seed(11)
    s.cam.occlusion = torch.rand((P, 16, 32, 1), device="cuda", generator=gen)
    # (512 texels of occlusion ~ 0.5 each: the occlusion colour sum(occlusion * envmap) stays around 0.5, inside its clamp to [0, 1])
    env = (torch.rand((1, 16, 32), device="cuda", generator=gen) * 0.004).requires_grad_(True)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = torch.zeros(3, device="cuda")
    keys = ("albedo", "roughness", "normal", "world_normal", "occlusion")
    weights = [torch.randn((3, H, W), device="cuda", generator=gen) for _ in keys]

    def run(geometry_grad, **kw):
        _clear(m)
        env.grad = None
        for p in decoder_params:
            p.grad = None
        o = gr.render(30001, s.cam, m, pipe, bg, envmap=env, geometry_grad=geometry_grad, **kw)
        sum((o[k] * w).sum() for k, w in zip(keys, weights)).backward()
        grads = _leaf_grads(m, MATERIALS)
        grads["envmap"] = None if env.grad is None else env.grad.detach().clone()
        return o, grads

    def same_material_gradients(tag, got, want):
        for n in MATERIALS + ("envmap",):
            assert (got[n] is None) == (want[n] is None), (tag, n)
            if want[n] is not None:
                assert float(want[n].abs().sum()) > 0, (tag, n)
                util.assert_close(f"{tag}: {n}", got[n].cpu().numpy(), want[n].cpu().numpy(), tol=1e-4, max_bad_frac=1e-4)
        # (get_roughness reads _albedo, scene/gaussian_model.py:197-199: _roughness itself is reached by neither path)
        assert want["_roughness"] is None and want["_albedo"] is not None and want["_normal"] is not None and want["envmap"] is not None

    try:
        full, want = run(True, return_smpl_rot=True)   # (return_smpl_rot: the result carries the translation the cached runs need)
        assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in decoder_params)
        assert full["viewspace_points"].grad is not None and m._xyz.grad is not None
        short, got = run(False, return_smpl_rot=True)
        for k in gr.RESULT_KEYS:
            if isinstance(full[k], torch.Tensor) and k != "viewspace_points":
                assert torch.equal(short[k].detach(), full[k].detach()), f"forward result {k} differs"
        assert all(isinstance(full[k], torch.Tensor) for k in ("correct_Rs", "transforms", "translation"))
        same_material_gradients("decoders in the frame", got, want)
        assert all(p.grad is None for p in decoder_params), "a decoder parameter received a gradient on the short path"
        assert all(getattr(m, n).grad is None for n in GEOMETRY) and short["viewspace_points"].grad is None
        # ---- cached per-pose transforms (render.py:169-195): the other branch that forms world_normal
        cached = dict(transforms=full["transforms"].detach(), translation=full["translation"].detach())
        full_c, want_c = run(True, **cached)
        short_c, got_c = run(False, **cached)
        for k in ("albedo", "world_normal", "normal", "render", "render_alpha"):
            assert torch.equal(short_c[k].detach(), full_c[k].detach()), f"cached transforms: forward result {k} differs"
        same_material_gradients("cached transforms", got_c, want_c)
        assert all(getattr(m, n).grad is None for n in GEOMETRY)
        # ---- "auto": the six leaves frozen but a decoder still training -> the full path; the decoders frozen too -> the short one
        for n in GEOMETRY:
            getattr(m, n).requires_grad_(False)
        assert not gr.geometry_frozen(m)
        o, g_auto = run("auto")
        assert o["viewspace_points"].grad is not None and all(p.grad is not None for p in decoder_params)
        same_material_gradients("auto, decoders training", g_auto, want)
        for p in decoder_params:
            p.requires_grad_(False)
        assert gr.geometry_frozen(m)
        o, g_auto = run("auto")
        assert o["viewspace_points"].grad is None and all(p.grad is None for p in decoder_params)
        same_material_gradients("auto, everything frozen", g_auto, want)
    finally:
        gr.GEOMETRY_GRAD = True


def test_rasterizer_wrapper_refuses_what_needs_the_preprocess_backward(oracle):
    from mygauhuman_amd.diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C
    c = mc.case(oracle, "general")
    cam, g = c.cam, c.g
    d = util.to_dev
    rs = GaussianRasterizationSettings(image_height=mc.H, image_width=mc.W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=d(BG),
                                       scale_modifier=1.0, viewmatrix=d(cam["viewmatrix"]), projmatrix=d(cam["projmatrix"]), sh_degree=3,
                                       campos=d(cam["campos"]), prefiltered=False, debug=False)
    rast = GaussianRasterizer(rs)
    means2D = torch.zeros((c.P, 3), device="cuda", requires_grad=True)
    extra = d(c.extra).requires_grad_(True)
    colors = d(g["colors"]).requires_grad_(True)
    means3D = d(g["means3D"]).requires_grad_(True)
    kw = dict(means3D=means3D, means2D=means2D, opacities=d(g["opacities"]).requires_grad_(True), extra_colors=extra,
              cov3D_precomp=d(g["cov3D"]))
    with pytest.raises(ValueError, match="shs|SHs"):
        rast.forward_multi(shs=d(g["shs"]).requires_grad_(True), geometry_grad=False, **kw)
    z = torch.zeros((mc.H, mc.W), device="cuda")
    spec = _C.Phase1Loss(torch.zeros((3, mc.H, mc.W), device="cuda"), torch.zeros((3, mc.H, mc.W), device="cuda"), z, z + 1)
    with pytest.raises(ValueError, match="loss_spec"):
        rast.forward_multi(colors_precomp=colors, geometry_grad=False, loss_spec=spec, **kw)
    # and what it does carry: gradients for the two colour inputs only, depth and alpha upstreams ignored
    color, radii, depth, alpha, feats = rast.forward_multi(colors_precomp=colors, geometry_grad=False, **kw)
    main, triples = _images(c)
    loss = (color * main).sum() + depth.sum() + alpha.sum() + sum((f * w).sum() for f, w in zip(feats, triples) if w is not None)
    loss.backward()
    assert means3D.grad is None and means2D.grad is None and kw["opacities"].grad is None
    t32, t64, frac = mc.bounds("general", colors.grad.numel())
    util.assert_close("colors_precomp.grad", colors.grad.cpu().numpy(), c.want64[mc.MAIN], tol=t64, max_bad_frac=frac, outer_tol=10 * t64)
    for t in mc.LIVE_TRIPLES:
        util.assert_close(f"extra.grad {t}", extra.grad[:, 3 * t:3 * t + 3].cpu().numpy(), c.want64[t], tol=t64, max_bad_frac=frac,
                          outer_tol=10 * t64)


# ---- 4. the whole PBR step ---------------------------------------------------------------------------------------------------------
def _freeze(model):
    for n in GEOMETRY:
        getattr(model, n).requires_grad_(False)


def test_pbr_step_with_frozen_geometry_matches_the_full_backward_step():
    """The step of test_pbr_training_step_matches_the_torch_composition with the geometry frozen as update_learning_rate freezes
    it: loss, light and material gradients of the materials-only backward equal the full backward's at that test's tolerance; a
    FusedAdam step moves the materials and the light and leaves every frozen parameter and its moments bit for bit alone."""
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.optim import FusedAdam
    from mygauhuman_amd.pbr import PbrPhaseLoss
    from tests.test_gpu_pbr_loss import _close, _pbr_scene, _rest_of_loss, _shade
    try:
        s = _pbr_scene()
        m = s.model
        named = [(n, getattr(m, n)) for n in GEOMETRY + MATERIALS] + [("light", s.cubemap.base)]
        opt = FusedAdam([{"params": [p], "lr": 1e-3} for _, p in named])
        # one full-backward step with everything trainable gives the frozen parameters moments worth protecting
        fused = PbrPhaseLoss(s.gt, s.bound, s.knn)

        def step(geometry_grad):
            for _, p in named:
                p.grad = None
            o = gr.render(30001, s.cam, m, s.pipe, s.bg, envmap=s.env, geometry_grad=geometry_grad)
            rgb, alpha, rough = _shade(s, o)
            loss, terms = fused(rgb, alpha, o["albedo"], rough, m.get_albedo, m.get_roughness)
            assert torch.isfinite(terms).all()
            loss = loss + _rest_of_loss(s, rgb)
            loss.backward()
            return float(loss.detach()), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in named}

        step(True)
        opt.step()
        _freeze(m)
        lf, gf = step(True)
        ls, gs = step(False)
        _close("step loss", ls, lf)
        for n, _ in named:
            assert (gs[n] is None) == (gf[n] is None), n
            if n in GEOMETRY:
                assert gs[n] is None, n
            elif gf[n] is not None:
                _close(f"step gradient {n}", gs[n], gf[n])
        assert float(gs["light"].abs().sum()) > 0 and float(gs["_albedo"].abs().sum()) > 0
        # _roughness is reached by neither path (get_roughness reads _albedo, scene/gaussian_model.py:197-199); _normal is reached
        # with zeros: this loss reads the world normal detached (train.py:301), and no other image depends on it
        assert gs["_roughness"] is None and gs["_normal"] is not None and not gs["_normal"].any()

        def snapshot():
            out = {}
            for n, p in named:
                st = opt.state.get(p, {})
                out[n] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()) if "exp_avg" in st else (p.detach().clone(),)
            return out

        before = snapshot()
        opt.step()
        torch.cuda.synchronize()
        after = snapshot()
        for n in GEOMETRY:
            assert len(before[n]) == 3, f"{n} has no Adam moments to protect"
            for a, b in zip(before[n], after[n]):
                assert torch.equal(a, b), f"the frozen {n} (or one of its moments) moved"
        for n in ("_albedo", "light"):
            assert not torch.equal(before[n][0], after[n][0]), f"{n} did not move"
        assert torch.equal(before["_roughness"][0], after["_roughness"][0])   # no gradient, no step (see above)
    finally:
        gr.BAKE = False


def test_pbr_step_with_frozen_geometry_is_captured_by_graphed_frame():
    """Modelled on test_pbr_training_step_is_captured_by_graphed_frame: the materials-only step records into a GraphedFrame, passes
    its verification and replays equal to eager."""
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd.graph import GraphedFrame
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss
    from tests.test_gpu_pbr_loss import _close, _pbr_scene, _rest_of_loss, _shade
    try:
        s = _pbr_scene()
        _freeze(s.model)
        fused = PbrPhaseLoss(s.gt, s.bound, MaterialSmoothness(s.knn))
        params = [getattr(s.model, n) for n in MATERIALS if n != "_roughness"] + [s.cubemap.base]

        def step():
            o = gr.render(30001, s.cam, s.model, s.pipe, s.bg, envmap=s.env, geometry_grad=False)
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
            if trial == 1:
                s.gt.copy_(torch.rand_like(s.gt))
            loss_e, terms_e, grads_e = eager()
            loss_g, terms_g = frame.replay()
            torch.cuda.synchronize()
            frame.check()
            _close(f"captured loss {trial}", loss_g, loss_e, 2e-5)
            _close(f"captured terms {trial}", terms_g, terms_e, 2e-5)
            for i, (p, ge) in enumerate(zip(params, grads_e)):
                # (_normal: reached, with zeros -- this loss reads the world normal detached, train.py:301)
                assert ge is not None and (float(ge.abs().sum()) > 0 or p is s.model._normal), i
                _close(f"captured gradient {trial}.{i}", p.grad, ge, 2e-5)
        for n in GEOMETRY:
            assert getattr(s.model, n).grad is None, n
    finally:
        gr.BAKE = False


# ---- 5. guard bands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 65, "stack"])
def test_outputs_stay_inside_their_arrays(oracle, monkeypatch, P):
    from mygauhuman_amd.diff_gaussian_rasterization import _C
    from tests.test_gpu_guardband import GuardedTorch
    if P == "stack":
        c = mc.case(oracle, "stack_translucent")
        cam, g, extra = c.cam, c.g, c.extra
    else:
        cam, g = util.make_scene(P, mc.W, mc.H, seed=40 + P, deg=3, scale=0.2, behind_frac=0.0)
        extra = np.random.default_rng(P).random((P, 18)).astype(np.float32)
    f = _forward(cam, g, extra)
    gen = torch.Generator(device="cuda").manual_seed(1)
    main = torch.randn((3, mc.H, mc.W), device="cuda", generator=gen)
    triples = [torch.randn((3, mc.H, mc.W), device="cuda", generator=gen) if t != 4 else None for t in range(6)]
    guard = GuardedTorch()
    monkeypatch.setattr(_C, "torch", guard)
    d_color, d_extra = _colors_backward(f, main, triples)
    assert guard.check("colour-only backward") == 2   # dL_dcolor and dL_dextra, each inside its own guarded buffer
    monkeypatch.undo()
    # (values: items 1 and 2 above; here only that the call did its work inside the arrays)
    seen = f.radii > 0
    assert int(seen.sum()) > 0 and torch.isfinite(d_color).all() and torch.isfinite(d_extra).all()
    assert float(d_color[seen].abs().sum()) > 0 and float(d_extra[seen][:, :12].abs().sum()) > 0
    assert not d_extra[:, 12:15].any() and not d_color[~seen].any() and not d_extra[~seen].any()
