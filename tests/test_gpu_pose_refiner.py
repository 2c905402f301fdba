"""The pose-correction network on the GPU (csrc/pose_refiner.hip behind nets_pose.FusedBodyPoseRefiner): Rs and every gradient
against the float64 restatement (tests/pose_refiner_reference.py, itself pinned to the reference by tests/golden/pose_refiner.npz),
each held to about twice the error of the same module in torch f32 ops; run-to-run bits, gradient accumulation, the strided pose
view render() passes, the configurations that stay on the torch ops, the C entry points' output bounds, and render() with the fused
module against the same module in torch ops, eager and captured by graph.GraphedFrame."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from mygauhuman_amd import nets_pose
from mygauhuman_amd._lib import check, lib
from tests import pose_refiner_reference as ref

pytestmark = pytest.mark.gpu


def _build(J, init="large", seed=0):
    """the reference's construction; "large": non-zero biases and a last layer that makes rotations of up to ~4 rad"""
    torch.manual_seed(seed)
    m = nets_pose.FusedBodyPoseRefiner(total_bones=J, embedding_size=3 * (J - 1), mlp_width=128, mlp_depth=2).cuda()
    if init == "large":
        with torch.no_grad():
            m.block_mlps[0].bias.normal_(0, 0.1)
            m.block_mlps[2].bias.normal_(0, 0.1)
            m.block_mlps[4].weight.uniform_(-0.3, 0.3)
            m.block_mlps[4].bias.normal_(0, 0.1)
    return m


def _params(m):
    return [t for i in (0, 2, 4) for t in (m.block_mlps[i].weight, m.block_mlps[i].bias)]


def _err(a, want):
    return float((a.detach().double() - want).abs().max())


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("B", [1, 2, 5, 16])
@pytest.mark.parametrize("init", ["reference", "large"])
def test_rs_matches_float64(J, B, init):
    m = _build(J, init, seed=B)
    x = torch.randn(B, 3 * (J - 1), device="cuda") * 0.5
    got = m(x)["Rs"]
    assert type(got.grad_fn).__name__ == "_FusedPoseRefinerBackward" and got.shape == (B, J - 1, 3, 3)
    with torch.no_grad():
        torch32 = m.forward_torch(x)["Rs"]
        want = ref.forward(x.double(), [p.double() for p in _params(m)])
    e_fused, e_torch = _err(got, want), _err(torch32, want)
    assert e_fused <= 2 * e_torch + 1e-6, (e_fused, e_torch)


def _fragile_rows(x, ps, margin):
    """rows with a hidden pre-activation within margin x (that layer's largest) of zero, in float64: an f32 forward may take the
    other side of the ReLU there, which moves whole rows of the weight gradients (tests/test_gpu_nets.py's fragile points)"""
    z1, z2, _ = ref.preactivations(x.double(), [p.double() for p in ps])
    frag = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    for z in (z1, z2):
        frag |= (z.abs() < margin * z.abs().max()).any(dim=1)
    return frag


def _grads(m, x, g, fused):
    m.use_fused = fused
    m.zero_grad(set_to_none=True)
    xx = x.clone().requires_grad_(True)
    (m(xx)["Rs"] * g).sum().backward()
    m.use_fused = True
    return [p.grad.clone() for p in _params(m)] + [xx.grad.clone()]


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("B", [1, 2, 5, 16])
def test_gradients_match_float64_autograd(J, B):
    m = _build(J, "large", seed=100 + B)
    gen = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, 3 * (J - 1), device="cuda", generator=gen) * 0.5
    g = torch.randn(B, J - 1, 3, 3, device="cuda", generator=gen)
    frag = _fragile_rows(x, _params(m), 1e-5)
    assert int(frag.sum()) < B or B == 1
    g[frag] = 0.0
    fused, torch32 = _grads(m, x, g, True), _grads(m, x, g, False)
    ps64 = [p.detach().double().requires_grad_(True) for p in _params(m)]
    x64 = x.double().requires_grad_(True)
    (ref.forward(x64, ps64) * g.double()).sum().backward()
    want = [p.grad for p in ps64] + [x64.grad]
    for name, a, t, w in zip(("dW0", "db0", "dW2", "db2", "dW4", "db4", "dx"), fused, torch32, want):
        scale = float(w.abs().max())
        if scale == 0.0:
            continue                                    # (B = 1 and the one row was fragile)
        e_fused, e_torch = _err(a, w), _err(t, w)
        assert e_fused <= 2 * e_torch + 1e-6 * scale, (name, e_fused / scale, e_torch / scale)


def test_backward_is_deterministic_and_accumulates_like_torch():
    m = _build(55, "large", seed=7)
    x = torch.randn(5, 162, device="cuda") * 0.5
    g = torch.randn(5, 54, 3, 3, device="cuda")
    a, b = _grads(m, x, g, True), _grads(m, x, g, True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))     # no atomics: the same bits
    # .grad accumulates across two backward passes as torch's does
    m.zero_grad(set_to_none=True)
    for _ in range(2):
        (m(x)["Rs"] * g).sum().backward()
    for p, one in zip(_params(m), a[:6]):
        assert torch.equal(p.grad, one + one)


def test_strided_pose_view_is_read_in_place():
    """render() passes smpl_param["poses"][:, 3:], a non-contiguous view; its gradient reaches the poses tensor"""
    for J, B in ((24, 1), (55, 3)):
        m = _build(J, "large", seed=J)
        poses = (torch.randn(B, 3 * J, device="cuda") * 0.5).requires_grad_(True)
        view = poses[:, 3:]
        assert view.stride() == (3 * J, 1) and view.data_ptr() != poses.data_ptr()
        got = m(view)["Rs"]
        dense = view.detach().contiguous().requires_grad_(True)
        want = m(dense)["Rs"]
        assert torch.equal(got, want)
        g = torch.randn_like(got)
        (got * g).sum().backward()
        (want * g).sum().backward()
        assert torch.equal(poses.grad[:, 3:], dense.grad) and float(poses.grad[:, :3].abs().max()) == 0.0
    # a column stride as well: a transposed [E, B] tensor
    m = _build(24, "large", seed=1)
    xt = torch.randn(69, 4, device="cuda").t()
    assert xt.stride() == (1, 4)
    with torch.no_grad():
        assert torch.equal(m(xt)["Rs"], m(xt.contiguous())["Rs"])


def test_unfused_configurations_equal_forward_torch():
    torch.manual_seed(3)
    cases = ((nets_pose.FusedBodyPoseRefiner(total_bones=24, embedding_size=69, mlp_width=256, mlp_depth=4), 2),
             (nets_pose.FusedBodyPoseRefiner(total_bones=30, embedding_size=87, mlp_width=128, mlp_depth=2), 2),
             (nets_pose.FusedBodyPoseRefiner(total_bones=24, embedding_size=69, mlp_width=128, mlp_depth=2), 17))
    for m, B in cases:
        m = m.cuda()
        x = torch.randn(B, m.block_mlps[0].in_features, device="cuda")
        assert m.fused_params(x) is None
        got = m(x)["Rs"]
        assert type(got.grad_fn).__name__ != "_FusedPoseRefinerBackward"
        with torch.no_grad():
            assert torch.equal(got, m.forward_torch(x)["Rs"])


def _ptrs(ts):
    return (C.c_void_p * 3)(*[t.data_ptr() for t in ts])


def test_entry_points_write_exactly_their_outputs():
    """every output in the middle of a sentinel-filled buffer: the guard bands stay untouched, the outputs are written whole"""
    GUARD, S = 4096, 1234.5
    for J, B in ((24, 1), (55, 5), (55, 16)):
        m = _build(J, "large", seed=J + B)
        E = 3 * (J - 1)
        x = torch.randn(B, E, device="cuda") * 0.5
        g = torch.randn(B, J - 1, 3, 3, device="cuda")
        ps = [p.detach() for p in _params(m)]
        sizes = [B * (J - 1) * 9] + [p.numel() for p in ps] + [B * E]
        bufs = [torch.full((n + 2 * GUARD,), S, device="cuda") for n in sizes]
        outs = [b[GUARD:GUARD + n] for b, n in zip(bufs, sizes)]
        s = torch.cuda.current_stream().cuda_stream
        check(lib.gsr_pose_refiner_forward(J, B, 128, x.data_ptr(), E, 1, _ptrs(ps[0::2]), _ptrs(ps[1::2]), outs[0].data_ptr(), s),
              "forward")
        dws, dbs = outs[1:7:2], outs[2:7:2]
        check(lib.gsr_pose_refiner_backward(J, B, 128, x.data_ptr(), E, 1, _ptrs(ps[0::2]), _ptrs(ps[1::2]), g.data_ptr(),
                                            _ptrs(dws), _ptrs(dbs), outs[7].data_ptr(), s), "backward")
        torch.cuda.synchronize()
        for b, o, n in zip(bufs, outs, sizes):
            assert bool((b[:GUARD] == S).all()) and bool((b[GUARD + n:] == S).all())
            assert not bool((o == S).any()) and bool(torch.isfinite(o).all())
        with torch.no_grad():
            assert torch.equal(outs[0].view(B, J - 1, 3, 3), m(x)["Rs"])


def _render_setup(fused, seed=3, body="smpl"):
    from mygauhuman_amd import human_synth
    model, bodyarr = human_synth.build(4000, None, "cuda", seed=seed, motion=True, decoder="reference_size", body=body,
                                       pose_decoder="reference_size")
    dec = model.pose_decoder
    with torch.no_grad():
        dec.block_mlps[4].weight.mul_(2e3)      # rotations of ~0.1 rad instead of the initial ~1e-4: gradients with some weight
    dec.use_fused = fused
    cam = human_synth.view_camera(bodyarr, 160, 128, 1, n_views=8, device="cuda")
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    return model, cam, pipe


@pytest.mark.parametrize("body", ["smpl", "smplx"])
def test_render_with_the_fused_pose_refiner_equals_its_torch_ops(body):
    """render() with motion_offset_flag (gaussian_renderer/__init__.py:100-106): correct_Rs from the fused module against the same
    module in torch ops -- images, every leaf gradient and both decoders' gradients (offset network on its f32 instruction)"""
    from mygauhuman_amd import nets
    from mygauhuman_amd.gaussian_renderer import render
    res = {}
    try:
        nets.set_precision("f32")
        for fused in (True, False):
            model, cam, pipe = _render_setup(fused, body=body)
            o = render(1, cam, model, pipe, torch.zeros(3, device="cuda"))
            assert o["correct_Rs"].shape == (1, cam.smpl_param["poses"].shape[1] // 3 - 1, 3, 3)
            assert (type(o["correct_Rs"].grad_fn).__name__ == "_FusedPoseRefinerBackward") == fused
            (o["render"].mean() + 0.5 * o["render_alpha"].mean() + o["normal"].mean()).backward()
            decs = list(model.pose_decoder.parameters()) + list(model.lweight_offset_decoder.parameters())
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in decs)
            res[fused] = ([o[k].detach() for k in ("render", "render_alpha", "normal")],
                          [p.grad.clone() for p in decs] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    finally:
        nets.set_precision("bf16x3")
    for a, b in zip(res[True][0], res[False][0]):
        assert float((a - b).abs().max()) <= 1e-4
    assert len(res[True][1]) == len(res[False][1])
    for a, b in zip(res[True][1], res[False][1]):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-4 * scale + 1e-12, float((a - b).abs().max()) / max(scale, 1e-30)


def test_render_step_with_the_fused_pose_refiner_as_one_graph_equals_eager():
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.graph import GraphedFrame
    model, cam, pipe = _render_setup(True, seed=5)
    bg = torch.tensor([0.2, 0.3, 0.1], device="cuda")
    params = list(model.parameters()) + list(model.pose_decoder.parameters()) + list(model.lweight_offset_decoder.parameters())
    keys = ("render", "render_alpha", "normal", "render_axis")

    def step():
        o = render(1, cam, model, pipe, bg)
        sum(o[k].mean() for k in keys).backward()
        return o

    def eager():
        for p in params:
            p.grad = None
        o = step()
        return o["render"].detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

    frame = GraphedFrame(step, warmup=3, zero_grads=params)
    for trial in range(2):
        if trial == 1:   # the next frame's pose, updated in place: the captured strided view reads it
            cam.smpl_param["poses"].add_(0.05 * torch.randn_like(cam.smpl_param["poses"]))
        img_e, grads_e = eager()
        out = frame.replay()
        torch.cuda.synchronize()
        frame.check()
        assert torch.equal(out["render"].detach(), img_e), trial
        for p, ge in zip(params, grads_e):
            if ge is None:
                continue
            scale = float(ge.abs().max()) + 1e-20
            assert float((p.grad - ge).abs().max()) / scale < 2e-5, trial


def test_adam_on_a_target_rotation_lowers_the_loss():
    m = _build(24, "reference", seed=9)
    x = torch.randn(2, 69, device="cuda") * 0.5
    with torch.no_grad():
        target = nets_pose.RodriguesModule()(torch.randn(46, 3, device="cuda") * 0.5).view(2, 23, 3, 3)
    opt = torch.optim.Adam(m.parameters(), lr=3e-3)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        Rs = m(x)["Rs"]
        assert type(Rs.grad_fn).__name__ == "_FusedPoseRefinerBackward"
        loss = (Rs - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses[::8]
