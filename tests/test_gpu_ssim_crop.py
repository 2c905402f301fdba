"""GPU tests of the crop SSIM (loss_utils.bounding_rect / ssim_crop, csrc/ssim_crop.hip): the rectangle against the numpy
restatement of cv2.boundingRect, bit for bit; value and gradient against the fixture the reference's own ssim() made on the crop
(tests/golden/ssim_crop.npz, float64) and against the fp32 conv2d formulation on the CPU, at the tolerances of tests/test_gpu_ssim.py;
the layouts, the grouping and the empty rectangle; and what the feature is for: a training step with the reference's SSIM term
recorded once by graph.GraphedFrame and replayed on a second camera's mask, whose rectangle and area differ.
Every element is compared: no masks, no excluded outliers."""
import os
import types

import numpy as np
import pytest
import torch

from tests import ssim_crop_reference as R
from tests.torch_reference import ssim_torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_crop.npz")
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def _rect_of(mask_np):
    return np.asarray(R.bounding_rect_np(mask_np), np.int32)


def _human_mask(H, W, x, y, w, h, seed=0):
    """A standing-human-like blob (head, torso, two legs) whose box is (x, y, w, h), ragged inside."""
    m = np.zeros((H, W), np.float32)
    m[y:y + h // 6, x + w // 3:x + 2 * w // 3] = 1
    m[y + h // 6:y + h // 2, x:x + w] = 1
    m[y + h // 2:y + h, x + w // 8:x + 3 * w // 8] = 1
    m[y + h // 2:y + h, x + 5 * w // 8:x + 7 * w // 8] = 1
    m *= np.random.default_rng(seed).uniform(0, 1, (H, W)) > 0.2
    m[y, x + w // 2] = m[y + h - 1, x + w // 4] = m[y + h // 3, x] = m[y + h // 3, x + w - 1] = 1
    return m


# ---- bounding_rect ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_bounding_rect_matches_the_restatement_on_the_fixture_masks(fx, case):
    from mygauhuman_amd import loss_utils
    mask = R.case_inputs(case)["mask"]
    want = _rect_of(mask)
    assert np.array_equal(want, fx[f"{case}/rect"])
    for t in (torch.from_numpy(mask).float(), torch.from_numpy(mask).to(torch.uint8), torch.from_numpy(mask) != 0):
        got = loss_utils.bounding_rect(t.cuda())
        assert got.dtype == torch.int32 and got.shape == (4,) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), (case, t.dtype)
        assert np.array_equal(loss_utils.bounding_rect(t.cuda()[None]).cpu().numpy(), want)   # [1, H, W] as train.py holds it


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.bool])
def test_bounding_rect_at_1024_squared(dtype):
    from mygauhuman_amd import loss_utils
    for k, (x, y, w, h) in enumerate([(311, 97, 402, 801), (0, 0, 1024, 1024), (1023, 1023, 1, 1), (5, 1000, 1011, 3)]):
        m = _human_mask(1024, 1024, x, y, w, h, seed=k)
        want = _rect_of(m)
        assert tuple(want) == (x, y, w, h)
        got = loss_utils.bounding_rect(torch.from_numpy(m).to(dtype).cuda())
        assert np.array_equal(got.cpu().numpy(), want), (dtype, k)


@pytest.mark.parametrize("shape", [(37, 53), (1, 1), (1, 77), (77, 1), (67, 129), (130, 250), (16, 64), (3, 5)])
def test_bounding_rect_corners_odd_sizes_and_the_empty_mask(shape):
    from mygauhuman_amd import loss_utils
    H, W = shape
    masks = [np.zeros(shape, np.float32)]   # all zero -> (0, 0, 0, 0)
    for (r, c) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3)):
        m = np.zeros(shape, np.float32)
        m[r, c] = 1
        masks.append(m)
    both = np.zeros(shape, np.float32)
    both[0, W - 1] = both[H - 1, 0] = 1
    masks.append(both)
    masks.append((np.random.default_rng(H * W).uniform(0, 1, shape) > 0.97).astype(np.float32))
    for i, m in enumerate(masks):
        want = _rect_of(m)
        for dtype in (torch.float32, torch.uint8, torch.bool):
            t = torch.from_numpy(m).to(dtype).cuda()
            assert np.array_equal(loss_utils.bounding_rect(t).cpu().numpy(), want), (shape, i, dtype)
        # a mask that does not start on a 16-byte boundary takes the element-load path
        for dtype in (torch.float32, torch.uint8):
            buf = torch.zeros(H * W + 3, dtype=dtype, device="cuda")
            view = buf[1:1 + H * W].view(H, W)
            view.copy_(torch.from_numpy(m).to(dtype))
            assert view.data_ptr() % 16 != 0
            assert np.array_equal(loss_utils.bounding_rect(view).cpu().numpy(), want), (shape, i, dtype, "unaligned")
    assert np.array_equal(loss_utils.bounding_rect(torch.zeros(shape, device="cuda")).cpu().numpy(), [0, 0, 0, 0])


def test_bounding_rect_negative_zero_nan_and_other_dtypes():
    from mygauhuman_amd import loss_utils
    m = torch.zeros(40, 50, device="cuda")
    m[3, 4] = -0.0                      # == 0: outside
    m[10, 20] = float("nan")            # != 0: inside
    m[30, 7] = -2.5
    assert loss_utils.bounding_rect(m).tolist() == [7, 10, 14, 21]
    assert loss_utils.bounding_rect(m.double()).tolist() == [7, 10, 14, 21]
    assert loss_utils.bounding_rect((m != 0).to(torch.int64)).tolist() == [7, 10, 14, 21]


def test_bounding_rect_writes_only_rect_and_its_workspace_and_needs_no_initial_state():
    from mygauhuman_amd import _lib, loss_utils
    nws = int(_lib.lib.gsr_bounding_rect_workspace_ints())
    m = _human_mask(300, 517, 40, 21, 222, 270)
    want = _rect_of(m)
    mask = torch.from_numpy(m).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for fill in (GUARD, -1, 0, 0x7FFFFFFF):   # whatever the workspace and rect hold beforehand
        rbuf = torch.full((4 + 4 + 4,), GUARD, dtype=torch.int32, device="cuda")
        wbuf = torch.full((64 + nws + 64,), GUARD, dtype=torch.int32, device="cuda")
        rbuf[4:8] = fill
        wbuf[64:64 + nws] = fill
        for _ in range(2):   # the second call finds what the first one left
            _lib.check(_lib.lib.gsr_bounding_rect(300, 517, mask.data_ptr(), _lib.MASK_F32, rbuf[4:8].data_ptr(),
                                                  wbuf[64:].data_ptr(), stream), "gsr_bounding_rect")
            assert np.array_equal(rbuf[4:8].cpu().numpy(), want)
        assert bool((rbuf[:4] == GUARD).all()) and bool((rbuf[8:] == GUARD).all())
        assert bool((wbuf[:64] == GUARD).all()) and bool((wbuf[64 + nws:] == GUARD).all())
    out = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    assert loss_utils.bounding_rect(mask, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError):
        loss_utils.bounding_rect(mask, out=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError):
        loss_utils.bounding_rect(mask, out=torch.zeros(5, dtype=torch.int32, device="cuda"))


# ---- ssim_crop against the fixture ------------------------------------------------------------------------------------------------
def _run(img1s, img2s, rect_np, grad=True):
    """Values and d value / d img1 of a call on device copies of float64 inputs."""
    from mygauhuman_amd import loss_utils
    rect = torch.from_numpy(np.asarray(rect_np, np.int32)).cuda()
    a = [t.float().cuda().requires_grad_(grad) for t in img1s]
    b = [t.float().cuda() for t in img2s]
    out = loss_utils.ssim_crop(a[0], b[0], rect) if len(a) == 1 else loss_utils.ssim_crop(tuple(a), tuple(b), rect)
    vals = [out] if len(a) == 1 else list(out)
    assert all(v.dim() == 0 for v in vals)
    if grad:
        sum(vals).backward()
    return [v.detach().cpu() for v in vals], [t.grad.cpu() if grad else None for t in a]


@pytest.mark.parametrize("case", list(R.CASES))
def test_ssim_crop_matches_the_reference_fixture(fx, case):
    x = R.case_inputs(case)
    rx, ry, rw, rh = rect = tuple(int(v) for v in fx[f"{case}/rect"])
    vals, grads = _run(x["img1"], x["img2"], rect)
    for g in range(R.CASES[case][3]):
        want_v, want_g = float(fx[f"{case}/{g}/value"]), fx[f"{case}/{g}/grad"]
        got_v, got_g = float(vals[g]), grads[g].numpy()
        inside = got_g[:, ry:ry + rh, rx:rx + rw]
        scale = float(np.abs(want_g).max())
        err64 = float(np.abs(inside.astype(np.float64) - want_g).max())
        # the fp32 conv2d formulation on the CPU, on the crop as train.py slices it
        v32, g32 = R.value_and_grad(x["img1"][g].float(), x["img2"][g].float(), rect)
        err32 = float(np.abs(inside - g32[:, ry:ry + rh, rx:rx + rw]).max())
        print(f"{case}/{g}: value {got_v:.9f} ref {want_v:.9f} (diff {abs(got_v - want_v):.2e}), "
              f"grad err vs f64 {err64 / scale:.2e}, vs fp32 conv2d {err32 / scale:.2e} of max|grad| {scale:.3e}")
        assert abs(got_v - want_v) < 2e-6
        assert abs(got_v - v32) < 2e-6
        assert err64 < 2e-5 * scale
        assert err32 < 1e-4 * scale
        outside = got_g.copy()
        outside[:, ry:ry + rh, rx:rx + rw] = 0.0
        assert not outside.any() and np.isfinite(got_g).all()   # exactly 0.0 outside the rect


def test_full_frame_rect_equals_ssim():
    from mygauhuman_amd import loss_utils
    for shape in ((3, 97, 131), (3, 64, 64), (1, 300, 517)):
        g = torch.Generator().manual_seed(sum(shape))
        img2 = torch.rand(shape, generator=g).cuda()
        base = (img2 + 0.2 * torch.randn(shape, generator=g).cuda()).clamp(0, 1)
        a, b = base.clone().requires_grad_(True), base.clone().requires_grad_(True)
        rect = torch.tensor([0, 0, shape[2], shape[1]], dtype=torch.int32, device="cuda")
        v = loss_utils.ssim_crop(a, img2, rect)
        w = loss_utils.ssim(b[None], img2[None])
        assert abs(float(v) - float(w)) < 2e-6
        v.backward()
        w.backward()
        scale = float(b.grad.abs().max())
        assert float((a.grad - b.grad).abs().max()) < 2e-5 * scale
        # and against the fp32 / fp64 conv2d formulation, as tests/test_gpu_ssim.py checks ssim()
        for dt, tol in ((torch.float32, 1e-4), (torch.float64, 2e-5)):
            r1 = base.cpu().to(dt).requires_grad_(True)
            r = ssim_torch(r1[None], img2.cpu().to(dt)[None])
            r.backward()
            assert abs(float(v) - float(r)) < 2e-6
            assert float((a.grad.cpu().to(dt) - r1.grad).abs().max()) < tol * scale


def test_mean_at_1024_squared_stays_within_the_value_bound():
    """The fused mean (per-tile float sums, added in double in a fixed order) against the float64 formulation at the training size."""
    from mygauhuman_amd import loss_utils
    g = torch.Generator().manual_seed(5)
    img2 = torch.rand((3, 1024, 1024), generator=g)
    img1 = (img2 + 0.2 * torch.randn((3, 1024, 1024), generator=g)).clamp(0, 1)
    for rect in ((311, 97, 402, 801), (0, 0, 1024, 1024)):
        v = loss_utils.ssim_crop(img1.cuda(), img2.cuda(), torch.tensor(rect, dtype=torch.int32, device="cuda"))
        r = R.crop_ssim(img1.double(), img2.double(), rect)
        print(f"1024^2 rect {rect}: {float(v):.9f} vs f64 {float(r):.9f}")
        assert abs(float(v) - float(r)) < 2e-6


def test_permuted_hwc_view_gives_the_bits_of_its_contiguous_copy():
    from mygauhuman_amd import loss_utils
    g = torch.Generator().manual_seed(3)
    hwc = torch.rand((90, 70, 3), generator=g).cuda()
    img2 = torch.rand((3, 90, 70), generator=g).cuda()
    rect = torch.tensor([9, 17, 33, 41], dtype=torch.int32, device="cuda")
    leaf_v, leaf_c = hwc.clone().requires_grad_(True), hwc.permute(2, 0, 1).contiguous().requires_grad_(True)
    view = leaf_v.permute(2, 0, 1)
    assert not view.is_contiguous()
    v1, v2 = loss_utils.ssim_crop(view, img2, rect), loss_utils.ssim_crop(leaf_c, img2, rect)
    assert torch.equal(v1, v2)
    v1.backward()
    v2.backward()
    assert torch.equal(leaf_v.grad.permute(2, 0, 1), leaf_c.grad) and float(leaf_c.grad.abs().max()) > 0


def test_two_groups_give_the_bits_of_two_calls_and_calls_repeat_bit_for_bit(fx):
    x = R.case_inputs("two_groups")
    rect = fx["two_groups/rect"]
    both_v, both_g = _run(x["img1"], x["img2"], rect)
    again_v, again_g = _run(x["img1"], x["img2"], rect)
    for g in range(2):
        one_v, one_g = _run(x["img1"][g:g + 1], x["img2"][g:g + 1], rect)
        assert torch.equal(both_v[g], one_v[0]) and torch.equal(both_g[g], one_g[0])
        assert torch.equal(both_v[g], again_v[g]) and torch.equal(both_g[g], again_g[g])
    assert not torch.equal(both_v[0], both_v[1])
    # groups may differ in their number of planes, and a group may need no gradient
    from mygauhuman_amd import loss_utils
    r = torch.from_numpy(rect).cuda()
    a3 = x["img1"][0].float().cuda().requires_grad_(True)
    a1 = x["img1"][1][:1].float().cuda()
    v3, v1 = loss_utils.ssim_crop((a3, a1), (x["img2"][0].float().cuda(), x["img2"][1][:1].float().cuda()), r)
    assert torch.equal(v3.detach().cpu(), both_v[0])
    want1 = R.crop_ssim(x["img1"][1][:1], x["img2"][1][:1], rect)
    assert abs(float(v1) - float(want1)) < 2e-6
    (v3 + v1).backward()
    assert torch.equal(a3.grad.cpu(), both_g[0])
    with torch.no_grad():
        assert torch.equal(loss_utils.ssim_crop(a3, x["img2"][0].float().cuda(), r).cpu(), both_v[0])


def test_upstream_factor_scales_the_gradient(fx):
    from mygauhuman_amd import loss_utils
    x = R.case_inputs("interior")
    rect = torch.from_numpy(fx["interior/rect"]).cuda()
    a, b = x["img1"][0].float().cuda(), x["img2"][0].float().cuda()
    a1, a2 = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
    loss_utils.ssim_crop(a1, b, rect).backward()
    (0.01 * (1.0 - loss_utils.ssim_crop(a2, b, rect))).backward()
    scale = float(a1.grad.abs().max())
    # the factor enters before the window sums, so every product rounds differently: each gradient is within the project's bound
    # (2e-5 of its largest magnitude) of the exact one, and so they are of each other
    assert float((a2.grad + 0.01 * a1.grad).abs().max()) < 2e-5 * 0.01 * scale


@pytest.mark.parametrize("rect", [(0, 0, 0, 0), (20, 30, 0, 15), (20, 30, 15, 0), (500, 500, 10, 10), (-40, -40, 10, 10)])
def test_empty_rect_gives_zero_value_and_zero_gradient(rect):
    """The one divergence from the reference, which raises on an empty crop: value 0.0, gradient all zeros, finite.  A rect that
    lies outside the frame is clipped to nothing on the device and is empty as well."""
    from mygauhuman_amd import loss_utils
    a = torch.rand((3, 70, 90), device="cuda").requires_grad_(True)
    b = torch.rand((3, 70, 90), device="cuda")
    v = loss_utils.ssim_crop(a, b, torch.tensor(rect, dtype=torch.int32, device="cuda"))
    assert float(v) == 0.0
    (1.0 - v).backward()
    assert bool(torch.isfinite(a.grad).all()) and float(a.grad.abs().max()) == 0.0
    # from an all-zero mask, end to end
    r = loss_utils.bounding_rect(torch.zeros((70, 90), device="cuda"))
    assert float(loss_utils.ssim_crop(a, b, r)) == 0.0


def test_a_rect_that_overhangs_the_frame_is_clipped():
    from mygauhuman_amd import loss_utils
    a, b = torch.rand((3, 70, 90), device="cuda"), torch.rand((3, 70, 90), device="cuda")
    over = loss_utils.ssim_crop(a, b, torch.tensor([60, 50, 1000, 1000], dtype=torch.int32, device="cuda"))
    want = loss_utils.ssim_crop(a, b, torch.tensor([60, 50, 30, 20], dtype=torch.int32, device="cuda"))
    assert torch.equal(over, want)


def test_bad_arguments_raise_on_the_host():
    from mygauhuman_amd import loss_utils
    a, b = torch.rand((3, 32, 48), device="cuda"), torch.rand((3, 32, 48), device="cuda")
    rect = torch.tensor([1, 2, 8, 9], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="window_size"):
        loss_utils.ssim_crop(a, b, rect, window_size=7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss_utils.ssim_crop(a, b, rect.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss_utils.ssim_crop(a.cpu(), b.cpu(), rect)
    with pytest.raises(ValueError):
        loss_utils.ssim_crop(a, b[:, :16], rect)
    with pytest.raises(ValueError):
        loss_utils.ssim_crop((a, a[:, :16]), (b, b[:, :16]), rect)
    with pytest.raises(ValueError):
        loss_utils.ssim_crop(a, b, rect.float())
    with pytest.raises(ValueError):
        loss_utils.ssim_crop(a[None], b[None], rect)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="one device"):
            loss_utils.ssim_crop(a, b, rect.to("cuda:1"))


# ---- capture: one graph, two cameras' masks -----------------------------------------------------------------------------------------
def _close(name, got, want, rtol=2e-5):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, name
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert bool(torch.isfinite(got).all()), name
    assert err <= rtol * scale + 1e-30, f"{name}: max error {err:.3e} against a magnitude of {scale:.3e}"


def _host_rect(bound):
    return R.bounding_rect_np(bound.reshape(bound.shape[-2:]).cpu().numpy())


def _replay_across_two_cameras(step, eager, params, rect, bound, second_camera):
    from mygauhuman_amd.graph import GraphedFrame
    frame = GraphedFrame(step, warmup=3, zero_grads=params)
    rects = []
    for trial in range(2):
        if trial == 1:
            second_camera()   # the next camera's targets through the same graph: updated in place
        want_rect = _host_rect(bound)
        rects.append(want_rect)
        loss_e, grads_e = eager(want_rect)
        rect.fill_(-7)   # the replay must form the rect itself
        loss_g = frame.replay()
        torch.cuda.synchronize()
        frame.check()
        assert tuple(rect.tolist()) == want_rect, trial
        _close(f"captured loss {trial}", loss_g, loss_e)
        for i, (p, ge) in enumerate(zip(params, grads_e)):
            if ge is None:
                continue
            _close(f"captured gradient {trial}.{i}", p.grad, ge)
    (x0, y0, w0, h0), (x1, y1, w1, h1) = rects
    assert (w0, h0) != (w1, h1) and w0 * h0 != w1 * h1 and (x0, y0) != (x1, y1) and w1 * h1 > 0


def test_phase1_step_with_the_crop_ssim_is_captured_and_replays_on_a_second_camera():
    """render(fused_loss=Phase1Loss) + 0.01 (2 - ssim_crop((image, normal), (gt, gt_normal), rect)) + 0.01 masked TV + scaling mean,
    with bounding_rect inside the step, recorded by graph.GraphedFrame; then bound, gt and gt_normal are overwritten in place with a
    second camera's targets (another rectangle, another area) and a replay must equal an eager step on the new targets whose
    rectangle is taken on the host and applied by slicing, as train.py:269-281 does."""
    from mygauhuman_amd import loss_utils
    from mygauhuman_amd.diff_gaussian_rasterization._C import Phase1Loss
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.pbr import get_masked_tv_loss
    from tests import util
    from tests.test_gpu_render import _human_scene
    s = _human_scene(None, seed=41)
    H, W = s.cam_np["H"], s.cam_np["W"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *shape: torch.rand(shape, device="cuda", generator=gen)  # noqa: E731
    gt, gt_normal, bkgd = rnd(3, H, W), rnd(3, H, W), (rnd(1, H, W) > 0.4).float()

    def ragged_box(y0, y1, x0, x1):
        m = torch.zeros((1, H, W), device="cuda")
        m[:, y0:y1, x0:x1] = (rnd(1, y1 - y0, x1 - x0) > 0.1).float()
        m[0, y0, x0] = m[0, y1 - 1, x1 - 1] = 1.0
        return m
    bound = ragged_box(H // 6, H - H // 8, W // 5, W - W // 7)
    spec = Phase1Loss(gt, gt_normal, bkgd, bound)
    # Phase1Loss keeps views of float32 contiguous targets: the in-place update below reaches it (a silent copy would let this
    # test pass on stale targets)
    assert spec.gt_image.data_ptr() == gt.data_ptr() and spec.gt_normal.data_ptr() == gt_normal.data_ptr()
    assert spec.bound.data_ptr() == bound.data_ptr() and spec.alpha_target.data_ptr() == bkgd.data_ptr()
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = util.to_dev(np.array([0.1, 0.2, 0.3], np.float32))
    params = list(s.model.parameters())
    rect = torch.zeros(4, dtype=torch.int32, device="cuda")

    def rest(o):
        return 0.01 * get_masked_tv_loss(o["render_alpha"], o["normal"]) + s.model.get_scaling.mean()

    def step():
        loss_utils.bounding_rect(bound, out=rect)
        o = render(1, s.cam, s.model, pipe, bg, fused_loss=spec)
        s_img, s_nrm = loss_utils.ssim_crop((o["render"], o["normal"]), (gt, gt_normal), rect)
        loss = o["loss"] + 0.01 * (2.0 - (s_img + s_nrm)) + rest(o)
        loss.backward()
        return loss.detach()

    def eager(host_rect):
        for p in params:
            p.grad = None
        x, y, w, h = host_rect
        o = render(1, s.cam, s.model, pipe, bg, fused_loss=spec)
        crop = lambda t: t[:, y:y + h, x:x + w].unsqueeze(0)  # noqa: E731
        ssim_loss = loss_utils.ssim(crop(o["render"]), crop(gt)) + loss_utils.ssim(crop(o["normal"]), crop(gt_normal))
        loss = o["loss"] + 0.01 * (2.0 - ssim_loss) + rest(o)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

    def second_camera():
        gt.copy_(rnd(3, H, W))
        gt_normal.copy_(rnd(3, H, W))
        bound.copy_(ragged_box(H // 3, H - H // 5 + 3, W // 2 - 21, W // 2 + 26))

    _replay_across_two_cameras(step, eager, params, rect, bound, second_camera)
    assert float(s.model._xyz.grad.abs().sum()) > 0


def test_pbr_step_with_the_crop_ssim_is_captured_and_replays_on_a_second_camera():
    """The PBR-phase step -- render -> build_mips -> pbr_shading -> PbrPhaseLoss + 0.01 (1 - ssim_crop(render_rgb, gt, rect)) with
    render_rgb the permuted [H, W, 3] view, read in place -- recorded once and replayed on a second camera's mask and target."""
    from mygauhuman_amd import gaussian_renderer as gr
    from mygauhuman_amd import loss_utils
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss
    from tests.test_gpu_pbr_loss import _pbr_scene, _shade
    try:
        s = _pbr_scene()
        fused = PbrPhaseLoss(s.gt, s.bound, MaterialSmoothness(s.knn))
        assert fused.targets_in_place
        assert fused.gt.data_ptr() == s.gt.data_ptr() and fused.bound.data_ptr() == s.bound.data_ptr()
        params = list(s.model.parameters()) + [s.cubemap.base]
        rect = torch.zeros(4, dtype=torch.int32, device="cuda")

        def fused_part():
            o = gr.render(30001, s.cam, s.model, s.pipe, s.bg, envmap=s.env)
            rgb, alpha, rough = _shade(s, o)
            loss, _ = fused(rgb, alpha, o["albedo"], rough, s.model.get_albedo, s.model.get_roughness)
            return loss, rgb

        def step():
            loss_utils.bounding_rect(s.bound, out=rect)
            loss, rgb = fused_part()
            assert not rgb.is_contiguous()
            loss = loss + 0.01 * (1.0 - loss_utils.ssim_crop(rgb, s.gt, rect))
            loss.backward()
            return loss.detach()

        def eager(host_rect):
            for p in params:
                p.grad = None
            x, y, w, h = host_rect
            loss, rgb = fused_part()
            loss = loss + 0.01 * (1.0 - loss_utils.ssim(rgb[:, y:y + h, x:x + w].unsqueeze(0), s.gt[:, y:y + h, x:x + w].unsqueeze(0)))
            loss.backward()
            torch.cuda.synchronize()
            return loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

        def second_camera():
            s.gt.copy_(torch.rand_like(s.gt))
            m = torch.zeros_like(s.bound)
            m[:, s.H // 4:s.H // 2 + 7, s.W // 3:s.W // 3 + 45] = 1.0
            m[:, s.H // 4 + 3:s.H // 4 + 9, s.W // 3 + 5:s.W // 3 + 11] = 0.0
            s.bound.copy_(m)

        _replay_across_two_cameras(step, eager, params, rect, s.bound, second_camera)
        assert float(s.cubemap.base.grad.abs().sum()) > 0 and float(s.model._xyz.grad.abs().sum()) > 0
    finally:
        gr.BAKE = False
