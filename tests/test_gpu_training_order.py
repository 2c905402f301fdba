"""The pieces in the order training runs them: evaluate under no_grad, train with the project's own writers (optim.FusedAdam, eager
and recorded into a graph; a captured torch update), evaluate again, freeze the geometry and go on.  A forward that follows a writer
must run on the weights the writer left, whoever the writer was:

  * nets.FusedLBSOffsetDecoder (the one module that derives a device buffer -- the packed MFMA fragments -- from its parameters)
    against the float64 restatement of tests/test_gpu_nets.py on the LIVE parameters, at that module's bounds;
  * render() with the fused network against the same call on the module's torch ops (they read the live parameters), f32 instruction;
  * nets_pose.FusedBodyPoseRefiner (no derived buffer) through the same sequences, at the bounds of tests/test_gpu_pose_refiner.py;
  * FusedAdam writes like an in-place op: version counters, and autograd's saved-tensor guard.

Every sequence asserts that its writer moved the reference by at least 100 x the bound the forward is held to, so that a forward on
stale weights cannot pass inside a tolerance."""
import copy
import types

import pytest
import torch

from tests import pose_refiner_reference as pose_ref
from tests.test_gpu_nets import _randomise, _ref64, precision  # noqa: F401  (precision: the fixture of both instruction choices)

pytestmark = pytest.mark.gpu

LR, STEPS, P = 1e-2, 3, 300          # 300 points: one 256-point workgroup and a tail
WRITERS = ("fused_adam", "graphed_fused_adam", "captured_torch_add", "fused_adam_then_frozen")


def _make_writer(kind, params, iteration, seed):
    """A function that changes `params` in place the way `kind` says (STEPS times).  Whatever has to be built first -- the
    optimizer's state, the capture with its eager warm-up -- is built HERE, before the caller's first evaluation: everything the
    returned function does to the parameters after that evaluation is the writer's own doing.
    iteration(): zero-argument forward + loss, returns the loss (the grad-enabled fused forward of the module under test)."""
    from mygauhuman_amd.graph import GraphedFrame
    from mygauhuman_amd.optim import FusedAdam
    if kind in ("fused_adam", "fused_adam_then_frozen"):
        opt = FusedAdam(params, lr=LR)

        def write():
            for _ in range(STEPS):
                opt.zero_grad(set_to_none=True)
                iteration().backward()
                opt.step()
            if kind == "fused_adam_then_frozen":      # what update_learning_rate leaves behind for the PBR phase
                for p in params:
                    p.requires_grad_(False)
        return write
    if kind == "graphed_fused_adam":
        opt = FusedAdam(params, lr=LR).init_state()
        opt.sync_lr()

        def step():
            loss = iteration()
            loss.backward()
            opt.step()
            return loss.detach()
        frame = GraphedFrame(step, warmup=1, zero_grads=params, verify=False)

        def write():
            for _ in range(STEPS):
                opt.sync_lr()
                frame.replay()
            torch.cuda.synchronize()
        write.keep = frame
        return write
    assert kind == "captured_torch_add"      # not our writer: plain torch ops, recorded once -- a replay runs no host code at all
    gen = torch.Generator(device="cuda").manual_seed(seed)
    grads = [torch.randn(p.shape, device="cuda", generator=gen) * p.detach().abs().max() for p in params]
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.graph(graph, stream=side):
        for p, g in zip(params, grads):
            p.add_(g, alpha=-10.0 * LR)
    torch.cuda.synchronize()

    def write():
        for _ in range(STEPS):
            graph.replay()
        torch.cuda.synchronize()
    write.keep = (graph, grads)
    return write


def _graph_nodes(out, depth=4):
    """names of the autograd nodes within `depth` steps of `out`"""
    names, level = set(), [out.grad_fn]
    for _ in range(depth):
        level = [f for f in level if f is not None]
        names |= {type(f).__name__ for f in level}
        level = [g for f in level for g, _ in f.next_functions]
    return names


def _evaluate(module, run, frozen):
    """The cached path: under no_grad, or -- frozen -- with grad enabled and no parameter that requires grad."""
    if frozen:
        assert torch.is_grad_enabled() and not any(p.requires_grad for p in module.parameters())
        out = run()
        assert out.grad_fn is None and not out.requires_grad
        return out
    with torch.no_grad():
        return run()


# ---------------------------------------------------------------------------------------------------------------- (a) decoder
@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("total_bones", [24, 55])
def test_offset_decoder_evaluates_on_the_weights_its_writer_left(total_bones, writer, precision):  # noqa: F811
    from mygauhuman_amd.nets import FusedLBSOffsetDecoder
    dec = FusedLBSOffsetDecoder(total_bones).cuda()
    dec.use_fused = True
    _randomise(dec, 11 + total_bones)
    gen = torch.Generator(device="cuda").manual_seed(total_bones)
    pts = (torch.rand(1, P, 3, device="cuda", generator=gen) * 2 - 1) * torch.tensor([0.45, 0.9, 0.15], device="cuda")
    target = torch.randn(1, total_bones, P, device="cuda", generator=gen)
    params = list(dec.parameters())
    rel = 2e-6 if precision == "f32" else 2e-5          # tests/test_gpu_nets.py: the bounds of the two instructions against float64

    def iteration():
        out = dec(pts)
        assert "_FusedOffsetNetBackward" in _graph_nodes(out)      # (the fused forward, not the torch ops)
        return (out - target).square().mean()
    write = _make_writer(writer, params, iteration, seed=total_bones)

    def held(got, want, tag):
        scale = float(want.abs().max())
        err = float((got.double() - want).abs().max())
        print(f"{tag}: max |fused - float64| = {err / scale:.3e} of the largest output (bound {rel:.0e})")
        assert got.shape == (1, total_bones, P)
        assert err <= rel * scale, (tag, err / scale)
    before = _ref64(dec, pts).detach()
    held(_evaluate(dec, lambda: dec(pts), False), before, "first evaluation")          # (fills whatever the module caches)
    write()
    after = _ref64(dec, pts).detach()
    moved = float((after - before).abs().max())
    print(f"{writer}: the float64 reference moved by {moved / float(after.abs().max()):.3e} of its largest output")
    assert moved >= 100 * rel * max(float(before.abs().max()), float(after.abs().max()))
    held(_evaluate(dec, lambda: dec(pts), writer == "fused_adam_then_frozen"), after, "evaluation after " + writer)


# ---------------------------------------------------------------------------------------------------------------- (c) pose net
@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("J", [24, 55])
def test_pose_refiner_evaluates_on_the_weights_its_writer_left(J, writer):
    from tests.test_gpu_pose_refiner import _build, _params
    m = _build(J, "large", seed=J)
    gen = torch.Generator(device="cuda").manual_seed(J + 1)
    x = torch.randn(5, 3 * (J - 1), device="cuda", generator=gen) * 0.5
    target = torch.randn(5, J - 1, 3, 3, device="cuda", generator=gen) * 0.5
    params = _params(m)

    def iteration():
        out = m(x)["Rs"]
        assert "_FusedPoseRefinerBackward" in _graph_nodes(out)
        return (out - target).square().mean()
    write = _make_writer(writer, params, iteration, seed=J)

    def reference():
        with torch.no_grad():
            want = pose_ref.forward(x.double(), [p.detach().double() for p in params])
            return want, float((m.forward_torch(x)["Rs"].double() - want).abs().max())

    def held(got, want, e_torch, tag):
        err = float((got.double() - want).abs().max())
        print(f"{tag}: max |fused - float64| = {err:.3e}, torch f32 ops {e_torch:.3e}")
        assert got.shape == (5, J - 1, 3, 3)
        assert err <= 2 * e_torch + 1e-6, (tag, err, e_torch)       # tests/test_gpu_pose_refiner.py: twice the torch ops' error
    before, e0 = reference()
    held(_evaluate(m, lambda: m(x)["Rs"], False), before, e0, "first evaluation")
    write()
    after, e1 = reference()
    moved = float((after - before).abs().max())
    print(f"{writer}: the float64 reference moved by {moved:.3e}")
    assert moved >= 100 * (2 * max(e0, e1) + 1e-6)
    held(_evaluate(m, lambda: m(x)["Rs"], writer == "fused_adam_then_frozen"), after, e1, "evaluation after " + writer)


# ---------------------------------------------------------------------------------------------------------------- (b) render()
IMAGES = ("render", "render_alpha", "normal")
RENDER_BOUND = 2e-5        # test_render_with_the_fused_offset_network_equals_render_with_its_torch_ops, f32 instruction


@pytest.mark.parametrize("body", ["smpl", "smplx"])
def test_render_after_fused_adam_steps_sees_the_new_offset_network(body):
    from mygauhuman_amd import densify, human_synth, nets
    from mygauhuman_amd.gaussian_renderer import GEOMETRY_LEAVES, geometry_frozen, render
    nets.set_precision("f32")
    try:
        model, arrays = human_synth.build(2000, None, "cuda", seed=3, motion=True, decoder="reference_size", body=body)
        dec = model.lweight_offset_decoder
        assert dec.use_fused and dec.total_bones == (24 if body == "smpl" else 55)
        cam = human_synth.view_camera(arrays, 160, 128, 0, n_views=8, device="cuda")
        pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
        bg = torch.zeros(3, device="cuda")
        opt = densify.training_setup(model, dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=0.05, scaling=5e-3, rotation=1e-3,
                                                 normal=1e-3, albedo=0.05, roughness=0.05), fused_step=True)
        opt.add_param_group({"params": list(model.pose_decoder.parameters()), "lr": 1e-3, "name": "pose_decoder"})
        opt.add_param_group({"params": list(dec.parameters()), "lr": LR, "name": "lweight_offset_decoder"})

        def images(fused, **kw):
            dec.use_fused = fused
            try:
                o = render(1, cam, model, pipe, bg, **kw)
            finally:
                dec.use_fused = True
            return [o[k].detach().clone() for k in IMAGES]

        def worst(a, b):
            return max(float((x - y).abs().max()) for x, y in zip(a, b))
        with torch.no_grad():
            first = images(True)                                    # the evaluation before the steps (fills the module's cache)
            assert worst(first, images(False)) <= RENDER_BOUND
        old_dec = copy.deepcopy(dec)       # the network of the first evaluation, on its torch ops (the live one is not touched)
        old_dec.use_fused = False
        for _ in range(STEPS):
            opt.zero_grad(set_to_none=True)
            o = render(1, cam, model, pipe, bg)
            (o["render"].mean() + 0.5 * o["render_alpha"].mean() + o["normal"].mean()).backward()
            opt.step()
        assert all(p.grad is not None and bool(p.grad.abs().max() > 0) for p in dec.parameters())
        with torch.no_grad():
            got = images(True)
            want = images(False)                                    # the torch ops read the live parameters: the reference
            model.lweight_offset_decoder = old_dec
            try:
                stale = [render(1, cam, model, pipe, bg)[k].detach().clone() for k in IMAGES]
            finally:
                model.lweight_offset_decoder = dec
            moved, net_moved = worst(want, first), worst(want, stale)
            print(f"{body}: three steps moved the images by {moved:.3e}, the offset network alone by {net_moved:.3e} "
                  f"(bound {RENDER_BOUND:.0e})")
            assert moved >= 100 * RENDER_BOUND and net_moved >= 100 * RENDER_BOUND
            err_eval = worst(got, want)
            print(f"{body}: no_grad render after the steps, max |fused - torch ops| = {err_eval:.3e}")
        # the frozen-geometry PBR phase: no geometry leaf and no decoder parameter requires grad; grad stays enabled
        for name in GEOMETRY_LEAVES:
            getattr(model, name).requires_grad_(False)
        for net in (model.pose_decoder, dec):
            for p in net.parameters():
                p.requires_grad_(False)
        assert geometry_frozen(model) and torch.is_grad_enabled()
        want = images(False, geometry_grad=False)
        assert worst(want, first) >= 100 * RENDER_BOUND
        err_frozen = worst(images(True, geometry_grad=False), want)
        print(f"{body}: frozen render(geometry_grad=False) after the steps, max |fused - torch ops| = {err_frozen:.3e}")
        assert err_eval <= RENDER_BOUND and err_frozen <= RENDER_BOUND, (err_eval, err_frozen)
    finally:
        nets.set_precision("bf16x3")


# ---------------------------------------------------------------------------------------------------------------- (d) versions
def _versions(ts):
    return [t._version for t in ts]


def _stat_inputs(n, gen):
    m = types.SimpleNamespace(xyz_gradient_accum=torch.rand((n, 1), device="cuda", generator=gen),
                              denom=torch.zeros((n, 1), device="cuda"), max_radii2D=torch.zeros((n,), device="cuda"))
    vpt = torch.zeros((n, 3), device="cuda", requires_grad=True)
    vpt.grad = torch.randn((n, 3), device="cuda", generator=gen) * 1e-3
    radii = torch.randint(0, 60, (n,), device="cuda", generator=gen, dtype=torch.int32)
    return m, vpt, radii > 20, radii


def test_fused_adam_step_bumps_the_version_of_what_it_wrote_and_of_nothing_else():
    from mygauhuman_amd import optim
    gen = torch.Generator(device="cuda").manual_seed(5)
    n = 1000
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen)) for s in ((n, 3), (n, 1), (7,), (n, 4))]
    opt = optim.FusedAdam([{"params": [p], "lr": 1e-3} for p in ps], lr=0.0).init_state()
    for p in ps[:3]:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen)       # ps[3] has no gradient: step() leaves it out entirely
    moments = [opt.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq")]
    model, vpt, vis, radii = _stat_inputs(n, gen)
    stats = [model.xyz_gradient_accum, model.denom, model.max_radii2D]
    inputs = [vpt.grad, vis, radii] + [p.grad for p in ps[:3]]

    def grown(before, ts):
        return [b < t._version for b, t in zip(before, ts)]
    v_p, v_m, v_s, v_i = _versions(ps), _versions(moments), _versions(stats), _versions(inputs)
    opt.step()
    assert grown(v_p, ps) == [True, True, True, False]
    assert grown(v_m, moments) == [True] * 6 + [False] * 2
    assert grown(v_s, stats) == [False] * 3 and _versions(inputs) == v_i
    v_p, v_m, v_s = _versions(ps), _versions(moments), _versions(stats)
    opt.step(stats=(vpt, vis, radii, model))
    assert grown(v_p, ps) == [True, True, True, False] and grown(v_m, moments) == [True] * 6 + [False] * 2
    assert grown(v_s, stats) == [True] * 3
    v_p, v_s = _versions(ps), _versions(stats)
    optim.update_stats(model, vpt, vis, radii)
    assert grown(v_s, stats) == [True] * 3 and _versions(ps) == v_p
    for p in ps:                                                       # no gradient anywhere: the statistics launch alone
        p.grad = None
    v_p, v_m, v_s = _versions(ps), _versions(moments), _versions(stats)
    opt.step(stats=(vpt, vis, radii, model))
    assert grown(v_s, stats) == [True] * 3 and _versions(ps) == v_p and _versions(moments) == v_m
    assert _versions(inputs[:3]) == v_i[:3]
    torch.cuda.synchronize()
    assert float(model.denom.max()) == 3.0                             # (three statistics launches ran)


def test_a_recorded_fused_adam_step_bumps_versions_at_record_time_only():
    """A replay runs no host code: whatever it writes, no version moves -- the reason why nothing derived from the parameters may be
    keyed on it (the offset network's packed weights above)."""
    from mygauhuman_amd.optim import FusedAdam
    gen = torch.Generator(device="cuda").manual_seed(6)
    p = torch.nn.Parameter(torch.randn((1000, 3), device="cuda", generator=gen))
    p.grad = torch.randn(p.shape, device="cuda", generator=gen)
    opt = FusedAdam([p], lr=1e-2).init_state()
    opt.sync_lr()
    written = [p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]]
    start, v0 = p.detach().clone(), _versions(written)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        opt.step()
    torch.cuda.synchronize()
    v1 = _versions(written)
    assert all(b > a for a, b in zip(v0, v1)) and torch.equal(p.detach(), start)      # recorded, not run
    graph.replay()
    torch.cuda.synchronize()
    assert _versions(written) == v1 and not torch.equal(p.detach(), start)            # run, and no version moved


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
def test_a_step_between_forward_and_backward_raises_as_with_torch_adam(optimizer):
    from mygauhuman_amd.optim import FusedAdam
    gen = torch.Generator(device="cuda").manual_seed(7)
    p = torch.nn.Parameter(torch.randn((1000,), device="cuda", generator=gen))
    opt = (torch.optim.Adam if optimizer == "torch" else FusedAdam)([p], lr=1e-2)
    y = (p * p).sum()                            # saves p for its backward
    p.grad = torch.ones_like(p)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()
    y = (p * p).sum()                            # ... and a forward after the step is as good as ever
    p.grad = None
    y.backward()
    assert torch.equal(p.grad, 2 * p.detach())
