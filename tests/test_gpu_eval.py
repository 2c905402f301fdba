"""GPU tests of the evaluation view finish (mygauhuman_amd.evaluate, csrc/eval.hip).

Finished float images and uint8 buffers: BIT-IDENTICAL to the reference's torch statements run on the same device (fill, clamp and
save_image's rounding are exact operations: there is no tolerance to choose).  psnr and ssim: against float64 (the fixture the
reference's own functions made, tests/golden/eval.npz; tests/eval_reference's numpy restatement at 1024 x 1024) within
2 x the reference's own float32 error for that case + 1e-6, absolute (the rule of DESIGN.md §8).  Measured errors (one MI355X):
see DESIGN.md §15."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import eval_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "eval.npz")
GUARD_F, GUARD_B = 1234.5, 0xA5


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def _gpu(x, hwc=()):
    """The case's images on the device: [C, H, W] contiguous, or (names in hwc) permuted views of [H, W, C] tensors."""
    out = {}
    for n, a in x["images"].items():
        t = torch.from_numpy(a).cuda()
        out[n] = t.permute(1, 2, 0).contiguous().permute(2, 0, 1) if n in hwc else t
    return out


def _torch_expected(x, flip=False):
    """The reference's statements on the device: finished floats and uint8 images."""
    imgs = {n: torch.from_numpy(a.copy()).cuda() for n, a in x["images"].items()}
    if flip:
        imgs["gt_normal"] = R.flip_normal_torch(imgs["gt_normal"])
    fin = R.finish_torch(imgs, torch.from_numpy(x["mask"]).cuda()[None], torch.from_numpy(x["background"]).cuda())
    return fin, {n: R.quantise_torch(t) for n, t in fin.items()}


def _bound(err32):
    return 2.0 * err32 + 1e-6


def _check_metric(tag, got, want64, ref32):
    if math.isinf(want64):
        assert got == want64, (tag, got, want64)
        return
    err, bound = abs(got - want64), _bound(abs(ref32 - want64))
    print(f"{tag}: ours - f64 = {got - want64:+.3e}, reference f32 - f64 = {ref32 - want64:+.3e}, bound {bound:.3e}")
    assert err <= bound, (tag, got, want64, err, bound)


MASKS = {"f32": lambda m: m, "u8": lambda m: m.to(torch.uint8), "bool": lambda m: m != 0}


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_finished_images_are_bit_identical_to_the_torch_statements(fx, case, layout):
    from mygauhuman_amd import evaluate
    x = R.case_inputs(case)
    want_f, want_u8 = _torch_expected(x)
    assert R.crc_of([want_u8[n].cpu().numpy() for n in R.NAMES]) == int(fx[f"{case}/u8_crc"])
    bg = torch.from_numpy(x["background"]).cuda()
    for mk, conv in MASKS.items():
        imgs = _gpu(x, hwc=R.NAMES if layout == "hwc" else ())
        mask = conv(torch.from_numpy(x["mask"]).cuda())
        fin, u8 = evaluate.finish_view(imgs, mask if mk != "u8" else mask[None], bg, to_uint8=R.NAMES)
        for n in R.NAMES:
            assert fin[n] is imgs[n]  # in place
            assert torch.equal(fin[n], want_f[n]), (case, layout, mk, n)
            assert u8[n].shape == (x["mask"].shape[0], x["mask"].shape[1], R.CHANNELS[n]) and torch.equal(u8[n], want_u8[n]), (case, n)


@pytest.mark.parametrize("case", ["rect_black_70x90", "rect_white_70x90", "strip_white_1x200", "ones_white_256"])
def test_separate_destination_and_flip_gt_normal(case):
    from mygauhuman_amd import evaluate
    x = R.case_inputs(case)
    want_f, want_u8 = _torch_expected(x, flip=True)
    for hwc in ((), ("gt_normal", "render")):
        imgs = _gpu(x, hwc=hwc)
        keep = {n: t.clone() for n, t in imgs.items()}
        out = {n: torch.empty_like(imgs[n]) for n in ("gt", "gt_normal", "render")}
        assert all(out[n].stride() == imgs[n].stride() for n in out)
        fin, u8 = evaluate.finish_view(imgs, torch.from_numpy(x["mask"]).cuda(), torch.from_numpy(x["background"]).cuda(),
                                       to_uint8=("gt_normal", "render_alpha"), flip_gt_normal=True, out=out)
        for n in R.NAMES:
            assert torch.equal(fin[n], want_f[n]), (case, n)
            if n in out:  # the input is left alone
                assert fin[n] is out[n] and torch.equal(imgs[n], keep[n])
        assert sorted(u8) == ["gt_normal", "render_alpha"]
        assert torch.equal(u8["gt_normal"], want_u8["gt_normal"]) and torch.equal(u8["render_alpha"], want_u8["render_alpha"])


def test_refusals_on_the_device():
    from mygauhuman_amd import evaluate
    x = torch.rand(3, 16, 32, device="cuda")
    m, bg = torch.ones(16, 16, device="cuda"), torch.zeros(3, device="cuda")
    with pytest.raises(ValueError, match="'render'.*not a dense permutation"):
        evaluate.finish_view({"render": x[:, :, ::2]}, m, bg)
    with pytest.raises(ValueError, match="'pair'.*2 channels"):
        evaluate.finish_view({"pair": torch.rand(2, 16, 16, device="cuda")}, m, bg)
    with pytest.raises(ValueError, match="metric"):
        evaluate.finish_view({"render": x[:, :, :16].contiguous()}, m, bg, metrics=evaluate.EvalMetrics(1), metric=("render", "gt"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.finish_view({"render": torch.rand(3, 16, 16, device="cuda")}, m, bg.cpu())


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_metrics_against_the_reference_fixture(fx, case):
    from mygauhuman_amd import evaluate
    x = R.case_inputs(case)
    for hwc in ((), ("render",)):
        table = evaluate.EvalMetrics(1)
        evaluate.finish_view(_gpu(x, hwc=hwc), torch.from_numpy(x["mask"]).cuda(), torch.from_numpy(x["background"]).cuda(),
                             metrics=table)
        r = table.result()
        assert r["psnr"].shape == (1,) and isinstance(r["psnr_mean"], float)
        _check_metric(f"{case} psnr", r["psnr_mean"], float(fx[f"{case}/psnr_f64"]), float(fx[f"{case}/psnr_f32"]))
        _check_metric(f"{case} ssim", r["ssim_mean"], float(fx[f"{case}/ssim_f64"]), float(fx[f"{case}/ssim_f32"]))


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_metrics_at_1024_squared():
    from mygauhuman_amd import evaluate
    x = R.inputs_at(1024, 1024, 4242)
    fin = R.finish_np(x["images"], x["mask"], x["background"])
    want_p, want_s = R.psnr_np(fin["render"], fin["gt"]), R.ssim_np(fin["render"], fin["gt"])
    tfin, _ = _torch_expected(x)
    ref_p, ref_s = R.metrics_torch(tfin["render"], tfin["gt"])  # the torch float32 expression on the device
    table = evaluate.EvalMetrics(1)
    got, _ = evaluate.finish_view(_gpu(x), torch.from_numpy(x["mask"]).cuda(), torch.from_numpy(x["background"]).cuda(), metrics=table)
    r = table.result()
    for n in R.NAMES:
        assert torch.equal(got[n], tfin[n]), n
    _check_metric("1024 psnr", r["psnr_mean"], want_p, ref_p)
    _check_metric("1024 ssim", r["ssim_mean"], want_s, ref_s)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_rows_fill_in_order_are_reproducible_and_overflow_is_sticky():
    from mygauhuman_amd import evaluate
    cases = ["rect_black_70x90", "rect_white_70x90", "zeros_black_70x90_inf", "rect_black_70x90", "rect_white_70x90"]
    singles = []
    for c in cases:
        x, t = R.case_inputs(c), evaluate.EvalMetrics(1)
        evaluate.finish_view(_gpu(x), torch.from_numpy(x["mask"]).cuda(), torch.from_numpy(x["background"]).cuda(), metrics=t)
        singles.append(t.table.cpu().numpy().copy())
    assert np.array_equal(singles[0].view(np.uint64), singles[3].view(np.uint64))  # two runs, the same bits
    assert np.array_equal(singles[1].view(np.uint64), singles[4].view(np.uint64))
    table = evaluate.EvalMetrics(5)

    def push(c):
        x = R.case_inputs(c)
        evaluate.finish_view(_gpu(x), torch.from_numpy(x["mask"]).cuda(), torch.from_numpy(x["background"]).cuda(), metrics=table)
    for c in cases:
        push(c)
    r = table.result()
    rows = np.stack([r["psnr"], r["ssim"]], 1)
    assert np.array_equal(rows.view(np.uint64), np.concatenate(singles).view(np.uint64))
    assert math.isinf(r["psnr_mean"]) and r["ssim_mean"] == float(r["ssim"].sum() / 5)
    before = table.table.cpu().numpy().copy()
    push("rect_black_70x90")  # a sixth view into five rows
    assert np.array_equal(table.table.cpu().numpy().view(np.uint64), before.view(np.uint64))
    assert table.state.cpu().tolist() == [6, 1]
    with pytest.raises(RuntimeError, match="6 views"):
        table.result()
    table.reset()
    push("rect_white_70x90")
    assert np.array_equal(table.result()["psnr"].view(np.uint64), singles[1][:, 0].view(np.uint64))


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rect_black_70x90", "strip_white_1x200"])
@pytest.mark.parametrize("mask_dtype", ["f32", "u8"])
def test_guard_bands_around_every_buffer(case, mask_dtype):
    """The C entry point on buffers carved out of padded allocations: nothing outside a destination, the workspace or the table is
    written (odd sizes: 70 x 90 is no multiple of the 16-pixel tile or the 4-pixel group; the strip is one pixel high)."""
    from mygauhuman_amd import _lib
    x = R.case_inputs(case)
    H, W = x["mask"].shape
    PAD = 64

    def padded(n, dtype, fill):
        return torch.full((n + 2 * PAD,), fill, device="cuda", dtype=dtype)
    want_f, want_u8 = _torch_expected(x)
    v = _lib.EvalView()
    v.slots, v.height, v.width = len(R.NAMES), H, W
    bufs = {}
    for k, n in enumerate(R.NAMES):
        c = R.CHANNELS[n]
        src, dst, u8 = padded(c * H * W, torch.float32, GUARD_F), padded(c * H * W, torch.float32, GUARD_F), padded(c * H * W, torch.uint8, GUARD_B)
        src[PAD:PAD + c * H * W] = torch.from_numpy(x["images"][n]).cuda().reshape(-1)
        bufs[n] = (src, dst, u8)
        s = v.slot[k]
        s.src, s.dst, s.u8 = src.data_ptr() + 4 * PAD, dst.data_ptr() + 4 * PAD, u8.data_ptr() + PAD
        s.stride[:] = [H * W, W, 1]
        s.channels, s.flags = c, _lib.EVAL_FILL if n in R.FILL_NAMES else 0
    m = torch.from_numpy(x["mask"]).cuda()
    m = m if mask_dtype == "f32" else m.to(torch.uint8)
    bg = torch.from_numpy(x["background"]).cuda()
    v.mask, v.mask_dtype, v.background = m.data_ptr(), _lib.MASK_F32 if mask_dtype == "f32" else _lib.MASK_U8, bg.data_ptr()
    v.metric_image, v.metric_gt = R.NAMES.index("render"), R.NAMES.index("gt")
    nws = int(_lib.lib.gsr_eval_workspace_floats(H, W))
    ws = padded(nws, torch.float32, GUARD_F)
    table = padded(2 * 3, torch.float64, GUARD_F)
    state = torch.zeros(2, device="cuda", dtype=torch.int32)
    state[0] = 1  # the second of three rows
    v.counter, v.overflow = state.data_ptr(), state.data_ptr() + 4
    v.table, v.capacity = table.data_ptr() + 8 * PAD, 3
    _lib.check(_lib.lib.gsr_eval_view_finish(C.byref(v), ws.data_ptr() + 4 * PAD, torch.cuda.current_stream().cuda_stream), "finish")
    torch.cuda.synchronize()
    for n in R.NAMES:
        c = R.CHANNELS[n]
        src, dst, u8 = bufs[n]
        assert torch.equal(src[PAD:-PAD], torch.from_numpy(x["images"][n]).cuda().reshape(-1)), n  # dst given: src untouched
        assert torch.equal(dst[PAD:-PAD].reshape(c, H, W), want_f[n]) and torch.equal(u8[PAD:-PAD].reshape(H, W, c), want_u8[n]), n
        for b, g in ((src, GUARD_F), (dst, GUARD_F), (u8, GUARD_B)):
            assert bool((b[:PAD] == g).all()) and bool((b[-PAD:] == g).all()), n
    assert bool((ws[:PAD] == GUARD_F).all()) and bool((ws[-PAD:] == GUARD_F).all())
    t = table.cpu().numpy()
    assert (t[:PAD + 2] == GUARD_F).all() and (t[PAD + 4:] == GUARD_F).all() and (t[PAD + 2:PAD + 4] != GUARD_F).all()
    assert state.cpu().tolist() == [2, 0]


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_finish_view_records_under_graph_capture_and_replays():
    from mygauhuman_amd import evaluate
    cases = ["rect_black_70x90", "rect_white_70x90", "zeros_black_70x90_inf"]
    xs = [R.case_inputs(c) for c in cases]
    eager = []
    for x in xs:
        t = evaluate.EvalMetrics(1)
        fin, u8 = evaluate.finish_view(_gpu(x), torch.from_numpy(x["mask"]).cuda(), torch.from_numpy(x["background"]).cuda(), metrics=t,
                                       to_uint8=("render",))
        eager.append((t.table.cpu().numpy().copy(), fin["render"].clone(), u8["render"].clone()))
    static = _gpu(xs[0])
    mask, bg = torch.from_numpy(xs[0]["mask"]).cuda(), torch.from_numpy(xs[0]["background"]).cuda()
    table = evaluate.EvalMetrics(3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        evaluate.finish_view({n: t.clone() for n, t in static.items()}, mask, bg, metrics=table, to_uint8=("render",))  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    table.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # a host read in here would raise
        fin, u8 = evaluate.finish_view(static, mask, bg, metrics=table, to_uint8=("render",))
    for k, x in enumerate(xs):
        for n in R.NAMES:
            static[n].copy_(torch.from_numpy(x["images"][n]).cuda())
        mask.copy_(torch.from_numpy(x["mask"]).cuda())
        bg.copy_(torch.from_numpy(x["background"]).cuda())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(fin["render"], eager[k][1]) and torch.equal(u8["render"], eager[k][2]), k
    r = table.result()
    rows = np.stack([r["psnr"], r["ssim"]], 1)
    assert np.array_equal(rows.view(np.uint64), np.concatenate([e[0] for e in eager]).view(np.uint64))


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def _scene(S=512, n_views=4):
    from mygauhuman_amd import human_synth
    model, body = human_synth.build(20_000, device="cuda", seed=0)
    views = []
    for k in range(n_views):
        cam = human_synth.view_camera(body, S, S, k, n_views=n_views)
        cam.original_image = torch.from_numpy((R._u01((3, S, S), 900 + k) * 1.2 - 0.1).astype(np.float32)).cuda()
        cam.original_normal = torch.from_numpy(R._u01((3, S, S), 950 + k).astype(np.float32)).cuda()
        m = np.zeros((1, S, S), np.float32)
        m[:, S // 8 + 3 * k:(7 * S) // 8, S // 4 - 5 * k:(3 * S) // 4] = 1.0
        cam.bound_mask = torch.from_numpy(m).cuda()
        cam.pose_id = k
        views.append(cam)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True, sync_free_raster=True)
    return model, views, pipe


@pytest.mark.parametrize("iteration", [1, 3001])
@pytest.mark.parametrize("graphed", [False, True])
def test_render_set_against_the_reference_loop(tmp_path, iteration, graphed):
    from PIL import Image
    from mygauhuman_amd import evaluate
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.pbr import CubemapLight, get_brdf_lut, pbr_shading
    S = 512
    model, views, pipe = _scene(S)
    bg = torch.zeros(3, device="cuda")
    kw = {}
    if iteration > 3000:
        torch.manual_seed(3)
        light = CubemapLight(base_res=32).cuda()
        with torch.no_grad():
            light.base.copy_(torch.rand_like(light.base))
            light.build_mips()
        rays = torch.from_numpy((R._u01((S * S, 3), 77) - 0.5).astype(np.float32)).cuda()
        kw = dict(cubemap=light, brdf_lut=get_brdf_lut(os.path.join(GOLDEN, "pbr_brdf_256_256.bin")).cuda(), canonical_rays=rays)
    want_imgs, want_metrics = R.reference_loop(
        render, pbr_shading, views, model, pipe, bg, iteration, kw.get("cubemap"), kw.get("brdf_lut"),
        evaluate.view_dirs_of(views[0], kw["canonical_rays"], S, S) if kw else None)
    got = evaluate.render_set(views, model, pipe, bg, iteration, out_dir=str(tmp_path), graphed=graphed, return_images=True, **kw)
    assert got["lpips"] is None and got["fps"] > 0 and len(got["per_view"]["psnr"]) == len(views)
    names = sorted(want_imgs[0])
    assert len(names) == (13 if iteration > 3000 else 9)
    for i, fin in enumerate(want_imgs):
        for n in names:
            assert torch.equal(got["images"][i][n], fin[n]), (i, n)  # bit-identical finished floats
        for n in names:  # the PNGs hold the uint8 buffers, which hold the reference's rounding of the reference's finished image
            want_u8 = R.quantise_torch(fin[n]).cpu().numpy()
            png = np.asarray(Image.open(os.path.join(str(tmp_path), n, "{0:05d}.png".format(i))))
            assert np.array_equal(png, np.repeat(want_u8, 3, axis=2) if want_u8.shape[2] == 1 else want_u8), (i, n)
        pair = (fin["render_pbr" if iteration > 3000 else "render"].double().cpu().numpy(), fin["gt"].double().cpu().numpy())
        p64, s64 = R.psnr_np(*pair), R.ssim_np(*pair)
        _check_metric(f"view {i} psnr", float(got["per_view"]["psnr"][i]), p64, want_metrics[i][0])
        _check_metric(f"view {i} ssim", float(got["per_view"]["ssim"][i]), s64, want_metrics[i][1])
    assert got["psnr"] == float(got["per_view"]["psnr"].sum() / len(views))
