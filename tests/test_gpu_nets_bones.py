"""The skinning-offset network on the fused kernels at SMPL-X's 55 bones (csrc/mlp.hip with two 32-row output tiles,
nets.py): forward and parameter gradients against the float64 restatement of tests/test_gpu_nets.py and against the reference's own
module (tests/golden/lbs_offset_decoder_55.npz), a training loop, render() end to end -- and the 24-bone entry points unchanged."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_nets as base   # (the float64 restatement, the randomisation and the fragile points of the 24-bone tests)

pytestmark = pytest.mark.gpu

NB = 55


@pytest.fixture(params=["bf16x3", "f32"])
def precision(request):
    from mygauhuman_amd import nets
    nets.set_precision(request.param)
    yield request.param
    nets.set_precision("bf16x3")


def _decoder(seed):
    from mygauhuman_amd.nets import FusedLBSOffsetDecoder
    dec = FusedLBSOffsetDecoder(total_bones=NB).cuda()
    dec.use_fused = True
    base._randomise(dec, seed)
    return dec


def _points(P, g=None):
    return (torch.rand(1, P, 3, device="cuda", generator=g) * 2 - 1) * torch.tensor([0.45, 0.9, 0.15], device="cuda")


@pytest.mark.parametrize("P", [1, 31, 128, 129, 4097, 200_000])
def test_fused_55_bone_decoder_matches_float64_restatement(P, precision):
    torch.manual_seed(P)
    dec = _decoder(P)
    pts = _points(P)
    with torch.no_grad():
        got = dec(pts)
    want = base._ref64(dec, pts).detach()
    assert got.shape == (1, NB, P) and got.permute(0, 2, 1).is_contiguous()
    scale = float(want.abs().max())
    err = float((got.double() - want).abs().max())
    assert err <= (2e-6 if precision == "f32" else 2e-5) * scale, err / scale


@pytest.mark.parametrize("P", [1, 100, 128, 1025, 3000, 70_000])
def test_fused_55_bone_decoder_parameter_gradients_match_float64_autograd(P, precision):
    from mygauhuman_amd.nets import FusedLBSOffsetDecoder
    dec = _decoder(P)
    g = torch.Generator(device="cuda").manual_seed(P + 1)
    pts = _points(P, g)
    w = torch.randn(1, NB, P, device="cuda", generator=g)
    frag = base._fragile_points(dec, pts, 1e-4)
    assert int(frag.sum()) <= max(1, P // 5)
    w[:, :, frag] = 0.0
    out = dec(pts)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ != "AddmmBackward0"   # the fused autograd function ran
    (out * w).sum().backward()
    got = [p.grad.clone() for p in dec.parameters()]
    dec64 = FusedLBSOffsetDecoder(total_bones=NB).cuda().double()
    dec64.load_state_dict({k: v.double() for k, v in dec.state_dict().items()})
    (dec64.forward_torch(pts.double()) * w.double()).sum().backward()
    for (name, _), a, b in zip(dec.named_parameters(), got, [p.grad for p in dec64.parameters()]):
        scale = float(b.abs().max())
        if P == 1 and scale == 0.0:
            continue
        err = float((a.double() - b).abs().max()) / scale
        assert err <= (1e-5 if precision == "f32" else 5e-5), (name, err)


def test_fused_55_bone_decoder_matches_the_reference_fixture(golden_dir, precision):
    """The reference's own LBSOffsetDecoder(total_bones=55) (nets/mlp_delta_weight_lbs.py) on 256 points: its output, and its
    parameter gradients of (out * w).sum().  The fixture's gradients include points whose pre-activations lie within 1e-4 of a ReLU
    kink, where any f32 evaluation may take the other side; their share (linear in w) is taken out of the fixture's numbers with the
    float64 restatement and their w set to zero here, so what is compared is the reference's gradient over the remaining points."""
    from mygauhuman_amd.nets import FusedLBSOffsetDecoder
    gz = np.load(os.path.join(golden_dir, "lbs_offset_decoder_55.npz"))
    dec = FusedLBSOffsetDecoder(total_bones=NB).cuda()
    dec.load_state_dict({k[len("param."):]: torch.from_numpy(gz[k].astype(np.float32)) for k in gz.files if k.startswith("param.")})
    dec.use_fused = True
    pts = torch.from_numpy(gz["pts"]).cuda()
    w = torch.from_numpy(gz["w"]).cuda()
    want_out = torch.from_numpy(gz["out"]).cuda().double()
    with torch.no_grad():
        got = dec(pts)
    scale = float(want_out.abs().max())
    assert float((got.double() - want_out).abs().max()) <= (2e-6 if precision == "f32" else 2e-5) * scale
    frag = base._fragile_points(dec, pts, 1e-4)
    assert int(frag.sum()) <= 256 // 5
    w_frag = torch.zeros_like(w)
    w_frag[:, :, frag] = w[:, :, frag]
    dec64 = FusedLBSOffsetDecoder(total_bones=NB).cuda().double()
    dec64.load_state_dict({k: v.double() for k, v in dec.state_dict().items()})
    (dec64.forward_torch(pts.double()) * w_frag.double()).sum().backward()
    share = {n: p.grad for n, p in dec64.named_parameters()}
    out = dec(pts)
    assert type(out.grad_fn).__name__ != "AddmmBackward0"
    (out * (w - w_frag)).sum().backward()
    for name, p in dec.named_parameters():
        want = torch.from_numpy(gz["grad." + name]).cuda().double() - share[name]
        err = float((p.grad.double() - want).abs().max()) / float(want.abs().max())
        assert err <= (1e-5 if precision == "f32" else 5e-5), (name, err)


def test_fused_55_bone_decoder_repacks_after_a_parameter_update_and_trains():
    torch.manual_seed(0)
    dec = _decoder(0)
    pts = torch.rand(1, 1000, 3, device="cuda") - 0.5
    with torch.no_grad():
        a = dec(pts).clone()
        dec.bw_fc.bias.add_(1.0)          # an optimizer step changes the parameters in place
        b = dec(pts)
    assert b.shape == (1, NB, 1000) and torch.allclose(b, a + 1.0, atol=1e-5)
    opt = torch.optim.SGD(dec.parameters(), lr=1e-2)
    target = torch.randn(1, NB, 1000, device="cuda")
    losses = []
    for _ in range(20):
        opt.zero_grad()
        out = dec(pts)
        assert type(out.grad_fn).__name__ != "AddmmBackward0"
        loss = (out - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] and all(np.isfinite(losses))


def _mk(ts):
    return (C.c_void_p * 5)(*[t.data_ptr() for t in ts])


def test_24_bone_entry_points_unchanged():
    """The _nb(24) entry points are the old symbols: the same packed buffer and forward bit for bit on both instructions, and the
    same backward up to the order of the float atomics."""
    from mygauhuman_amd import nets
    from mygauhuman_amd._lib import check, lib, ptr
    torch.manual_seed(5)
    dec = nets.FusedLBSOffsetDecoder().cuda()
    base._randomise(dec, 5)
    params = [t.detach() for m in dec._layers() for t in (m.weight, m.bias)]
    P = 3000
    x = _points(P)[0].contiguous()
    s = torch.cuda.current_stream().cuda_stream
    n = lib.gsr_lbs_offset_mlp_packed_floats()
    assert lib.gsr_lbs_offset_mlp_packed_floats_nb(24) == n
    old_pk, new_pk = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    check(lib.gsr_lbs_offset_mlp_pack(_mk(params[0::2]), _mk(params[1::2]), ptr(old_pk), s), "pack")
    check(lib.gsr_lbs_offset_mlp_pack_nb(24, _mk(params[0::2]), _mk(params[1::2]), ptr(new_pk), s), "pack_nb")
    assert torch.equal(old_pk, new_pk)
    g = torch.randn(P, 24, device="cuda")
    try:
        for mode in ("f32", "bf16x3"):
            nets.set_precision(mode)
            o_old, o_new = torch.empty(P, 24, device="cuda"), torch.empty(P, 24, device="cuda")
            check(lib.gsr_lbs_offset_mlp_forward(P, ptr(x), ptr(old_pk), ptr(o_old), s), "forward")
            check(lib.gsr_lbs_offset_mlp_forward_nb(24, P, ptr(x), ptr(new_pk), ptr(o_new), s), "forward_nb")
            assert torch.equal(o_old, o_new), mode
            d_old, d_new = torch.empty(P, 24, device="cuda"), torch.empty(P, 24, device="cuda")
            check(lib.gsr_debug_lbs_offset_mlp_forward_bf16x3(P, ptr(x), ptr(old_pk), ptr(d_old), s), "bf16x3")
            check(lib.gsr_debug_lbs_offset_mlp_forward_bf16x3_nb(24, P, ptr(x), ptr(new_pk), ptr(d_new), s), "bf16x3_nb")
            assert torch.equal(d_old, d_new)
            grads = {}
            for tag in ("old", "new"):
                gr = [torch.zeros_like(p) for p in params]
                nw = lib.gsr_lbs_offset_mlp_backward_workspace_floats_nb(24, P)
                assert nw == lib.gsr_lbs_offset_mlp_backward_workspace_floats(P)
                ws = torch.empty(nw, device="cuda")
                if tag == "old":
                    check(lib.gsr_lbs_offset_mlp_backward(P, ptr(x), ptr(old_pk), ptr(g), ptr(ws), _mk(gr[0::2]), _mk(gr[1::2]), s), "bwd")
                else:
                    check(lib.gsr_lbs_offset_mlp_backward_nb(24, P, ptr(x), ptr(new_pk), ptr(g), ptr(ws), _mk(gr[0::2]), _mk(gr[1::2]), s),
                          "bwd_nb")
                grads[tag] = gr
            for a, b in zip(grads["old"], grads["new"]):
                assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max()), mode
    finally:
        nets.set_precision("bf16x3")


def _silence_fragile_points(mod, inp, out):
    """forward hook: dL/dout of the points _fragile_points names is zeroed (the same points in both runs: float64 on the same
    inputs) -- a pre-activation within 1e-6 of a ReLU kink takes either side in two f32 evaluations, and one such point moves a row
    of a weight gradient by O(1) (6,000 points x 512 units: a few per run)"""
    frag = base._fragile_points(mod, inp[0].detach(), 1e-4)
    assert int(frag.sum()) <= max(1, frag.numel() // 5)
    if out.requires_grad:
        keep = (~frag).to(out.dtype)[None, None, :]
        out.register_hook(lambda g: g * keep)


def test_render_smplx_with_the_fused_offset_network_equals_render_with_its_torch_ops():
    """render() with motion_offset_flag on an SMPL-X body: the 55-bone network on the fused kernels against the same module in torch
    ops, as test_gpu_nets.py checks at 24 bones -- images on both instructions, gradients on the f32 one, with the network's
    fragile points silenced in all three runs (_silence_fragile_points).  Seed 4: at seed 3 this body has one pixel whose alpha
    cut-off sits within the offsets' 1e-6 of the threshold, the same pixel on both instructions (a rasterizer fragile pixel)."""
    import types
    from mygauhuman_amd import human_synth, nets
    from mygauhuman_amd.gaussian_renderer import render
    res = {}
    try:
        for mode in ("torch", "f32", "bf16x3"):
            nets.set_precision("bf16x3" if mode == "bf16x3" else "f32")
            model, body = human_synth.build(6000, 1500, "cuda", seed=4, motion=True, decoder="reference_size", body="smplx")
            dec = model.lweight_offset_decoder
            assert dec.total_bones == NB and dec.use_fused
            dec.use_fused = mode != "torch"
            dec.register_forward_hook(_silence_fragile_points)
            cam = human_synth.view_camera(body, 160, 128, 0, n_views=8, device="cuda")
            pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
            o = render(1, cam, model, pipe, torch.zeros(3, device="cuda"))
            (o["render"].mean() + 0.5 * o["render_alpha"].mean() + o["normal"].mean()).backward()
            net = list(dec.parameters())
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net)
            res[mode] = ([o[k].detach() for k in ("render", "render_alpha", "normal")],
                         [p.grad.clone() for p in net] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    finally:
        nets.set_precision("bf16x3")
    for mode in ("f32", "bf16x3"):
        for a, b in zip(res[mode][0], res["torch"][0]):
            d = (a - b).abs()
            if mode == "f32":
                assert float(d.max()) <= 2e-5
            else:
                assert int((d > 1e-4).sum()) <= 8 and float(d.max()) <= 2e-2, (int((d > 1e-4).sum()), float(d.max()))
    for a, b in zip(res["f32"][1], res["torch"][1]):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-4 * scale + 1e-12, float((a - b).abs().max()) / max(scale, 1e-30)
