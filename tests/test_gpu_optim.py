"""The fused Adam step (mygauhuman_amd.optim.FusedAdam, csrc/adam.hip) on the GPU.

The yardstick is adam64 below: Adam restated in float64 from the formula in torch's documentation (it calls nothing under test).
torch's own float32 Adam (the default implementation, not fused=True) and FusedAdam run on identical inputs; FusedAdam's
parameters and moments may be off by twice torch-float32's own maximum error in that tensor plus one float32 ulp of the tensor's
largest parameter magnitude (two correct float32 evaluation orders differ by up to the sum of their errors; the ulp covers the
final p - update rounding) -- the rule of tests/test_gpu_pose_refiner.py.  Every figure is printed before it is asserted."""
import copy
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = ((1,), (3,), (4,), (15, 3), (0, 3))      # row shapes: 1, 3, 4, 45 floats and a zero-width one
LRS = (1.6e-4, 2.5e-3, 1e-3, 1.25e-4, 5e-3)
BETAS, EPS = (0.9, 0.999), 1e-15


# ---------------------------------------------------------------------------------------------------------------- helpers
def adam64(p, m, v, g, t, lr, beta1=BETAS[0], beta2=BETAS[1], eps=EPS):
    """One step t (1-based) of Adam on float64 tensors, in place: torch.optim.Adam's documented algorithm with weight_decay = 0,
    amsgrad = False, maximize = False."""
    m.mul_(beta1).add_(g, alpha=1.0 - beta1)
    v.mul_(beta2).add_(g * g, alpha=1.0 - beta2)
    m_hat = m / (1.0 - beta1 ** t)
    v_hat = v / (1.0 - beta2 ** t)
    p.sub_(lr * m_hat / (v_hat.sqrt() + eps))


def ulp32(x):
    """Spacing of float32 at magnitude x."""
    x = float(x)
    if x == 0.0 or not math.isfinite(x):
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


def make_grad(shape, gen, zero_rows=None):
    """Magnitudes log-uniform in [1e-12, 1e2], random sign, a quarter of the entries exactly zero; rows in zero_rows all zero."""
    e = torch.rand(shape, device="cuda", generator=gen) * 14.0 - 12.0
    g = torch.pow(10.0, e).clamp_(1e-12, 1e2)
    g = g * (torch.rand(shape, device="cuda", generator=gen) < 0.5).float().mul_(2).sub_(1)
    g = g * (torch.rand(shape, device="cuda", generator=gen) >= 0.25).float()
    if zero_rows is not None and g.shape[0]:
        g[zero_rows] = 0.0
    return g.contiguous()


def make_params(P, gen, shapes=WIDTHS):
    return [torch.randn((P,) + s, device="cuda", generator=gen) for s in shapes]


def groups_of(tensors, lrs=LRS):
    return [{"params": [torch.nn.Parameter(t.clone())], "lr": lr, "name": f"g{i}"} for i, (t, lr) in enumerate(zip(tensors, lrs))]


def state64(tensors):
    return [dict(p=t.double().clone(), m=torch.zeros_like(t, dtype=torch.float64), v=torch.zeros_like(t, dtype=torch.float64))
            for t in tensors]


def check_allowance(tag, ours, theirs, ref, own_ulp=False):
    """ours / theirs: lists of (p, m, v) float32 tensors; ref: list of dicts of float64.  Prints, then asserts the allowance.
    own_ulp: the ulp term of a moment is taken at that moment tensor's own largest magnitude instead of the parameter's."""
    worst = 0.0
    for i, ((po, mo, vo), (pt, mt, vt), r) in enumerate(zip(ours, theirs, ref)):
        if po.numel() == 0:
            assert po.shape == pt.shape
            continue
        ulp = ulp32(pt.detach().abs().max())
        for name, o, t, x in (("param", po, pt, r["p"]), ("exp_avg", mo, mt, r["m"]), ("exp_avg_sq", vo, vt, r["v"])):
            e_t = float((t.detach().double() - x).abs().max())
            e_o = float((o.detach().double() - x).abs().max())
            allow = 2.0 * e_t + (ulp32(t.detach().abs().max()) if own_ulp else ulp)
            print(f"{tag} tensor {i} {name}: torch-f32 error {e_t:.3e}, FusedAdam error {e_o:.3e}, allowance {allow:.3e}")
            assert torch.isfinite(o).all()
            assert e_o <= allow, f"{tag} tensor {i} {name}: {e_o:.3e} > {allow:.3e} (torch-f32 {e_t:.3e}, ulp {ulp:.3e})"
            worst = max(worst, e_o / allow)
    return worst


def triples(opt):
    out = []
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state[p]
            out.append((p.detach(), st["exp_avg"], st["exp_avg_sq"]))
    return out


def run_three(tensors, lrs, grads_of_step, K, fused_kwargs=None):
    """K steps of FusedAdam, torch's default float32 Adam and adam64 on the same start and the same gradients."""
    from mygauhuman_amd.optim import FusedAdam
    ours = FusedAdam(groups_of(tensors, lrs), lr=0.0, betas=BETAS, eps=EPS, **(fused_kwargs or {}))
    theirs = torch.optim.Adam(groups_of(tensors, lrs), lr=0.0, betas=BETAS, eps=EPS)
    ref = state64(tensors)
    for t in range(1, K + 1):
        grads = grads_of_step(t)
        for opt in (ours, theirs):
            for group, g in zip(opt.param_groups, grads):
                group["params"][0].grad = None if g is None else g.clone()
            opt.step()
        for r, g, lr in zip(ref, grads, lrs):
            if g is not None:
                adam64(r["p"], r["m"], r["v"], g.double(), t, lr)
    torch.cuda.synchronize()
    return ours, theirs, ref


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("K", [1, 2, 10, 200])
@pytest.mark.parametrize("P", [0, 1, 1000, 50_003])
def test_parity_with_float64_adam_on_model_shaped_groups(P, K):
    gen = torch.Generator(device="cuda").manual_seed(1000 * K + P)
    tensors = make_params(P, gen)
    zero_rows = torch.arange(P, device="cuda")[3::7]           # rows whose gradient is zero from step 0 on
    ours, theirs, ref = run_three(tensors, LRS, lambda t: [make_grad(x.shape, gen, zero_rows) for x in tensors], K)
    check_allowance(f"P={P} K={K}", triples(ours), triples(theirs), ref)
    for group, start in zip(ours.param_groups, tensors):
        p = group["params"][0]
        st = ours.state[p]
        assert float(st["step"]) == K and st["step"].dtype == torch.float32 and st["step"].dim() == 0
        if P and p.numel():
            # untouched means untouched: 0 / (0 + 1e-15) = 0, so the row keeps its bits and its moments stay +0
            assert torch.equal(p.detach()[zero_rows], start[zero_rows])
            assert not st["exp_avg"][zero_rows].any() and not st["exp_avg_sq"][zero_rows].any()
            assert not torch.equal(p.detach(), start)


def test_parity_at_smplx_decoder_shapes():
    """The two motion networks' parameter lists as two multi-tensor groups (more than a dozen small tensors each launch)."""
    from mygauhuman_amd import nets, nets_pose
    from mygauhuman_amd.optim import FusedAdam
    torch.manual_seed(3)
    mods = [nets.FusedLBSOffsetDecoder(total_bones=55).cuda(),
            nets_pose.FusedBodyPoseRefiner(total_bones=55, embedding_size=162, mlp_width=128, mlp_depth=2).cuda()]
    lists = [[p.detach().clone() for p in m.parameters()] for m in mods]
    assert sum(len(x) for x in lists) >= 6
    lrs = (5e-5, 5e-4)

    def build(cls, **kw):
        return cls([{"params": [torch.nn.Parameter(t.clone()) for t in lst], "lr": lr} for lst, lr in zip(lists, lrs)], lr=0.0,
                   betas=BETAS, eps=EPS, **kw)
    ours, theirs = build(FusedAdam), build(torch.optim.Adam)
    flat = [t for lst in lists for t in lst]
    flat_lr = [lr for lst, lr in zip(lists, lrs) for _ in lst]
    ref = state64(flat)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for t in range(1, 11):
        grads = [make_grad(x.shape, gen) for x in flat]
        for opt in (ours, theirs):
            ps = [p for group in opt.param_groups for p in group["params"]]
            for p, g in zip(ps, grads):
                p.grad = g.clone()
            opt.step()
        for r, g, lr in zip(ref, grads, flat_lr):
            adam64(r["p"], r["m"], r["v"], g.double(), t, lr)
    check_allowance("decoders", triples(ours), triples(theirs), ref)
    assert all(float(ours.state[p]["step"]) == 10 for group in ours.param_groups for p in group["params"])


def test_more_tensors_than_one_launch_holds():
    """150 small tensors in 19 groups: the host splits them into launches of <= 64 tensors and <= 16 groups.
    These tensors have 1 to 300 elements and gradients of up to 1e2 against parameters of order 1.  A float32 moment cannot be
    stored closer to its exact value than half an ulp of ITS OWN magnitude, and over a handful of elements torch's maximum error is
    often well below that, so the ulp term of a moment is taken at the moment's magnitude here (own_ulp); for the parameters the
    rule is the module's."""
    gen = torch.Generator(device="cuda").manual_seed(8)
    shapes = [((i * 37) % 300 + 1,) for i in range(150)]
    tensors = [torch.randn(s, device="cuda", generator=gen) for s in shapes]
    from mygauhuman_amd.optim import FusedAdam

    def build(cls):
        groups = [{"params": [torch.nn.Parameter(t.clone()) for t in tensors[8 * k: 8 * k + 8]], "lr": 1e-3 * (k + 1)} for k in range(19)]
        return cls(groups, lr=0.0, betas=BETAS, eps=EPS)
    ours, theirs = build(FusedAdam), build(torch.optim.Adam)
    ref = state64(tensors)
    for t in range(1, 4):
        grads = [make_grad(x.shape, gen) for x in tensors]
        for opt in (ours, theirs):
            for p, g in zip([p for group in opt.param_groups for p in group["params"]], grads):
                p.grad = g.clone()
            opt.step()
        for i, (r, g) in enumerate(zip(ref, grads)):
            adam64(r["p"], r["m"], r["v"], g.double(), t, 1e-3 * (i // 8 + 1))
    assert len(ours._launches) >= 3
    check_allowance("150 tensors", triples(ours), triples(theirs), ref, own_ulp=True)


def test_a_parameter_without_gradient_is_left_out_entirely():
    gen = torch.Generator(device="cuda").manual_seed(2)
    tensors = make_params(1000, gen)
    frozen = 1

    def grads(t):
        # the frozen group takes part in step 1 only (then requires_grad_(False) + zero_grad(set_to_none=True), as the reference
        # freezes the geometry after pbr_iteration)
        return [None if (i == frozen and t > 1) else make_grad(x.shape, gen) for i, x in enumerate(tensors)]
    from mygauhuman_amd.optim import FusedAdam
    ours = FusedAdam(groups_of(tensors), lr=0.0, betas=BETAS, eps=EPS)
    snap = None
    for t in range(1, 5):
        for group, g in zip(ours.param_groups, grads(t)):
            group["params"][0].grad = g
        ours.step()
        if t == 1:
            p = ours.param_groups[frozen]["params"][0]
            snap = [x.clone() for x in (p.detach(), ours.state[p]["exp_avg"], ours.state[p]["exp_avg_sq"], ours.state[p]["step"])]
    torch.cuda.synchronize()
    for i, group in enumerate(ours.param_groups):
        p = group["params"][0]
        st = ours.state[p]
        if i == frozen:
            for a, b in zip(snap, (p.detach(), st["exp_avg"], st["exp_avg_sq"], st["step"])):
                assert torch.equal(a, b)
            assert float(st["step"]) == 1
        else:
            assert float(st["step"]) == 4
    # a parameter that never had a gradient has no state at all, as in torch
    q = torch.nn.Parameter(torch.zeros(5, device="cuda"))
    ours.add_param_group({"params": [q], "lr": 1e-3})
    ours.step()
    assert len(ours.state[q]) == 0 and not q.detach().any()


# ---------------------------------------------------------------------------------------------------------------- alignment
GUARD, SENTINEL = 4096, -7.75


class Guarded:
    """A float32 buffer with GUARD sentinel floats either side of a payload that starts `offset` floats past a 16-byte boundary."""

    def __init__(self, values, offset):
        n = values.numel()
        self.whole = torch.full((GUARD + 4 + (n + 3) // 4 * 4 + 4 + GUARD,), SENTINEL, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.lo = GUARD + offset
        self.view = self.whole[self.lo:self.lo + n].view(values.shape)
        self.view.copy_(values)
        assert n == 0 or ((self.view.data_ptr() % 16) // 4 == offset % 4 and self.view.is_contiguous())

    def intact(self):
        n = self.view.numel()
        return bool((self.whole[:self.lo] == SENTINEL).all()) and bool((self.whole[self.lo + n:] == SENTINEL).all())


@pytest.mark.parametrize("offsets", [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 2, 3), (0, 0, 0, 2), (4, 0, 0, 0)])
def test_unaligned_views_give_the_aligned_bits_and_stay_inside_their_buffers(offsets):
    from mygauhuman_amd.optim import FusedAdam
    gen = torch.Generator(device="cuda").manual_seed(4)
    shapes = [(1,), (3,), (2 * 4096 + 5,), (1001, 3), (333, 15, 3), (4096,), (4095,), (0, 3)]
    start = [torch.randn(s, device="cuda", generator=gen) for s in shapes]
    grads = [[make_grad(s, gen) for s in shapes] for _ in range(3)]

    def run(offs):
        op, og, om, ov = offs
        bufs = []
        groups = []
        for t in start:
            bp = Guarded(t, op)
            bufs.append(bp)
            groups.append({"params": [torch.nn.Parameter(bp.view)], "lr": 1e-2})
            assert groups[-1]["params"][0].data_ptr() == bp.view.data_ptr()
        opt = FusedAdam(groups, lr=0.0, betas=BETAS, eps=EPS).init_state()
        for group in opt.param_groups:                  # moments carved out of guarded buffers as well
            p = group["params"][0]
            for key, o in (("exp_avg", om), ("exp_avg_sq", ov)):
                b = Guarded(torch.zeros_like(p), o)
                bufs.append(b)
                opt.state[p][key] = b.view
        for gs in grads:
            for group, g in zip(opt.param_groups, gs):
                b = Guarded(g, og)
                bufs.append(b)
                group["params"][0].grad = b.view
            opt.step()
        torch.cuda.synchronize()
        assert all(b.intact() for b in bufs), offs
        return [tuple(x.clone() for x in tr) for tr in triples(opt)]
    want, got = run((0, 0, 0, 0)), run(offsets)
    for a, b in zip(want, got):
        for x, y in zip(a, b):
            assert torch.equal(x, y), offsets
    assert not torch.equal(want[2][0], start[2])


# ---------------------------------------------------------------------------------------------------------------- statistics
def _stat_model(P, gen):
    m = types.SimpleNamespace()
    m.xyz_gradient_accum = torch.rand((P, 1), device="cuda", generator=gen)
    m.denom = torch.randint(0, 5, (P, 1), device="cuda", generator=gen).float()
    m.max_radii2D = torch.randint(0, 40, (P,), device="cuda", generator=gen).float()
    return m


@pytest.mark.parametrize("P", [0, 1, 1000, 50_003])
def test_statistics_equal_the_torch_ops(P):
    from mygauhuman_amd import densify, optim
    gen = torch.Generator(device="cuda").manual_seed(P + 6)
    base = _stat_model(P, gen)
    vpt = torch.zeros((P, 3), device="cuda", requires_grad=True)
    vpt.grad = torch.randn((P, 3), device="cuda", generator=gen) * 1e-3
    radii = torch.randint(0, 60, (P,), device="cuda", generator=gen, dtype=torch.int32)
    vis = radii > 20
    want = copy.deepcopy(base)
    densify.update_max_radii(want, radii, vis)
    densify.add_densification_stats(want, vpt, vis)
    tensors = make_params(P, gen)
    grads = [make_grad(t.shape, gen) for t in tensors]
    results = {}
    for mode in ("step", "alone", "none"):
        m = copy.deepcopy(base)
        opt = optim.FusedAdam(groups_of(tensors), lr=0.0, betas=BETAS, eps=EPS)
        for group, g in zip(opt.param_groups, grads):
            group["params"][0].grad = g.clone()
        if mode == "step":
            opt.step(stats=(vpt, vis, radii, m))
        elif mode == "alone":
            optim.update_stats(m, vpt, vis, radii)
            opt.step()
        else:
            opt.step()
        torch.cuda.synchronize()
        results[mode] = (m, triples(opt))
    for mode in ("step", "alone"):
        m = results[mode][0]
        assert torch.equal(m.denom, want.denom) and torch.equal(m.max_radii2D, want.max_radii2D), mode
        if P:
            rel = float(((m.xyz_gradient_accum - want.xyz_gradient_accum).abs() / want.xyz_gradient_accum.abs().clamp_min(1e-30)).max())
            print(f"P={P} {mode}: xyz_gradient_accum max relative difference {rel:.3e}")
            assert rel <= 1e-6
            out = ~vis
            for name in ("xyz_gradient_accum", "denom", "max_radii2D"):     # rows outside the filter: bitwise unchanged
                assert torch.equal(getattr(m, name)[out], getattr(base, name)[out]), (mode, name)
            assert bool(vis.any()) == (not torch.equal(m.denom, base.denom))
    m = results["none"][0]
    assert torch.equal(m.denom, base.denom) and torch.equal(m.xyz_gradient_accum, base.xyz_gradient_accum)
    for a, b in zip(results["step"][1], results["none"][1]):     # the parameters do not care whether stats was passed
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # a wider screen-space gradient row (stride 4) and the missing-gradient refusal
    if P:
        m = copy.deepcopy(base)
        wide = torch.zeros((P, 4), device="cuda", requires_grad=True)
        wide.grad = torch.cat([vpt.grad, torch.full((P, 1), 1e9, device="cuda")], 1)
        optim.update_stats(m, wide, vis, radii)
        assert torch.equal(m.xyz_gradient_accum, results["alone"][0].xyz_gradient_accum)
    with pytest.raises(RuntimeError, match="viewspace_point_tensor.grad is None"):
        optim.update_stats(copy.deepcopy(base), torch.zeros((P, 3), device="cuda", requires_grad=True), vis, radii)


# ---------------------------------------------------------------------------------------------------------------- surgery
def _surgery_model(fused, P=3000, seed=31):
    from mygauhuman_amd import densify
    from mygauhuman_amd.scene_model import HumanGaussianModel
    from tests.test_densify_cpu import make_state
    st = make_state(P, seed)
    m = HumanGaussianModel(3, device="cuda")
    for g in densify.GROUPS:
        setattr(m, densify.ATTR[g], torch.nn.Parameter(torch.from_numpy(st["params"][g]).cuda()))
    densify.training_setup(m, {g: 1e-3 * (i + 1) for i, g in enumerate(densify.GROUPS)}, fused_step=fused)
    return m


@pytest.mark.parametrize("op", ["clone", "prune", "prune_all"])
def test_steps_around_densify_surgery_match_torch_adam(op):
    from mygauhuman_amd import densify, optim
    P0 = 3000
    gen = torch.Generator(device="cuda").manual_seed(17)
    sel_grads = torch.rand((P0, 1), device="cuda", generator=gen)
    mask = torch.rand((P0,), device="cuda", generator=gen) < (0.4 if op == "prune" else 2.0)
    models = {fused: _surgery_model(fused) for fused in (True, False)}
    assert type(models[True].optimizer) is optim.FusedAdam and type(models[False].optimizer) is torch.optim.Adam
    params0 = {g: getattr(models[True], densify.ATTR[g]).detach().clone() for g in densify.GROUPS}
    ref = {g: r for g, r in zip(densify.GROUPS, state64([params0[g] for g in densify.GROUPS]))}
    lrs = {g: 1e-3 * (i + 1) for i, g in enumerate(densify.GROUPS)}

    def steps(first):
        for t in range(first, first + 3):
            grads = {g: make_grad(getattr(models[True], densify.ATTR[g]).shape, gen) for g in densify.GROUPS}
            for m in models.values():
                for g in densify.GROUPS:
                    getattr(m, densify.ATTR[g]).grad = grads[g].clone()
                m.optimizer.step()
                m.optimizer.zero_grad(set_to_none=True)
            for g in densify.GROUPS:
                adam64(ref[g]["p"], ref[g]["m"], ref[g]["v"], grads[g].double(), t, lrs[g])
    steps(1)
    for fused, m in models.items():
        if op == "clone":
            sel = densify.densify_and_clone(m, sel_grads, 0.5, 1e9)
            assert torch.equal(sel, sel_grads.squeeze(1) >= 0.5)
        else:
            densify.prune_points(m, mask)
    if op == "clone":
        sel = sel_grads.squeeze(1) >= 0.5
        for r in ref.values():
            n_new = int(sel.sum())
            r["p"] = torch.cat([r["p"], r["p"][sel]])
            r["m"] = torch.cat([r["m"], torch.zeros((n_new,) + tuple(r["m"].shape[1:]), dtype=torch.float64, device="cuda")])
            r["v"] = torch.cat([r["v"], torch.zeros((n_new,) + tuple(r["v"].shape[1:]), dtype=torch.float64, device="cuda")])
        P1 = P0 + int(sel.sum())
    else:
        for r in ref.values():
            for k in ("p", "m", "v"):
                r[k] = r[k][~mask]
        P1 = int((~mask).sum())
    assert (P1 == 0) == (op == "prune_all") and P1 != P0
    for fused, m in models.items():
        for g in densify.GROUPS:
            p = getattr(m, densify.ATTR[g])
            st = m.optimizer.state[p]
            assert p.shape[0] == P1 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
            assert float(st["step"]) == 3                                   # the counter the state entry carried over
            if op == "clone":                                               # new rows start from zero moments
                assert not st["exp_avg"][P0:].any() and not st["exp_avg_sq"][P0:].any() and st["exp_avg"][:P0].any()
    steps(4)
    torch.cuda.synchronize()

    def tri(m):
        out = []
        for g in densify.GROUPS:
            p = getattr(m, densify.ATTR[g])
            st = m.optimizer.state[p]
            assert float(st["step"]) == 6 and st["exp_avg"].shape == p.shape
            out.append((p.detach(), st["exp_avg"], st["exp_avg_sq"]))
        return out
    check_allowance(f"surgery {op}", tri(models[True]), tri(models[False]), [ref[g] for g in densify.GROUPS])
    assert models[True].optimizer.state[models[True]._xyz]["exp_avg"].shape == (P1, 3)


def test_reset_opacity_keeps_the_counter_and_zeroes_the_moments():
    from mygauhuman_amd import densify
    m = _surgery_model(True, P=500)
    for g in densify.GROUPS:
        getattr(m, densify.ATTR[g]).grad = torch.ones_like(getattr(m, densify.ATTR[g]))
    m.optimizer.step()
    densify.reset_opacity(m)
    st = m.optimizer.state[m._opacity]
    assert float(st["step"]) == 1 and not st["exp_avg"].any()
    m._opacity.grad = torch.ones_like(m._opacity)
    before = m._opacity.detach().clone()
    m.optimizer.step()
    assert float(st["step"]) == 2 and not torch.equal(before, m._opacity.detach())


# ---------------------------------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_checkpoint_moves_between_torch_adam_and_fused_adam(direction):
    from mygauhuman_amd.optim import FusedAdam
    gen = torch.Generator(device="cuda").manual_seed(23)
    tensors = make_params(1000, gen)
    grads = [[make_grad(t.shape, gen) for t in tensors] for _ in range(5)]
    classes = (torch.optim.Adam, FusedAdam) if direction == "torch_to_fused" else (FusedAdam, torch.optim.Adam)

    def drive(opt, gs):
        for step_grads in gs:
            for group, g in zip(opt.param_groups, step_grads):
                group["params"][0].grad = g.clone()
            opt.step()
    first = classes[0](groups_of(tensors), lr=0.0, betas=BETAS, eps=EPS)
    drive(first, grads[:3])
    sd = copy.deepcopy(first.state_dict())
    if direction == "torch_to_fused":   # as the reference stores it: step on the CPU
        assert all(st["step"].device.type == "cpu" for st in sd["state"].values())
    second = classes[1]([{"params": [torch.nn.Parameter(g["params"][0].detach().clone())], "lr": g["lr"], "name": g["name"]}
                         for g in first.param_groups], lr=0.0, betas=BETAS, eps=EPS)
    second.load_state_dict(sd)
    drive(second, grads[3:])
    whole = torch.optim.Adam(groups_of(tensors), lr=0.0, betas=BETAS, eps=EPS)
    drive(whole, grads)
    ref = state64(tensors)
    for t, step_grads in enumerate(grads, 1):
        for r, g, lr in zip(ref, step_grads, LRS):
            adam64(r["p"], r["m"], r["v"], g.double(), t, lr)
    torch.cuda.synchronize()
    check_allowance(direction, triples(second), triples(whole), ref)
    assert all(float(second.state[g["params"][0]]["step"]) == 5 for g in second.param_groups)


# ---------------------------------------------------------------------------------------------------------------- clamp_min
def test_clamp_min_equals_step_then_clamp():
    from mygauhuman_amd.optim import FusedAdam
    gen = torch.Generator(device="cuda").manual_seed(29)
    cube = torch.rand((6, 32, 32, 3), device="cuda", generator=gen) * 0.05      # a small cube map close to zero
    other = torch.randn((1000, 3), device="cuda", generator=gen)
    grads = [(make_grad(cube.shape, gen).clamp_(-1, 1), make_grad(other.shape, gen)) for _ in range(4)]

    def run(clamped):
        groups = [{"params": [torch.nn.Parameter(cube.clone())], "lr": 0.01, "name": "cubemap"},
                  {"params": [torch.nn.Parameter(other.clone())], "lr": 0.01, "name": "other"}]
        if clamped:
            groups[0]["clamp_min"] = 0.0
        opt = FusedAdam(groups, lr=0.0, betas=BETAS, eps=EPS)
        for gc, go in grads:
            opt.param_groups[0]["params"][0].grad, opt.param_groups[1]["params"][0].grad = gc.clone(), go.clone()
            opt.step()
            if not clamped:
                with torch.no_grad():
                    opt.param_groups[0]["params"][0].clamp_(min=0.0)
        return triples(opt)
    a, b = run(True), run(False)
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    assert float(a[0][0].min()) == 0.0 and float(a[1][0].min()) < 0.0     # the clamp bit, and only in its group


# ---------------------------------------------------------------------------------------------------------------- capture
def _capture_setup(gen):
    from mygauhuman_amd.optim import FusedAdam
    tensors = make_params(1000, gen)
    names = ("xyz", "f_dc", "opacity", "f_rest", "none")
    mk = lambda: FusedAdam([dict(g, name=n) for g, n in zip(groups_of(tensors), names)], lr=0.0, betas=BETAS, eps=EPS)  # noqa: E731
    return tensors, mk


def test_captured_step_replays_like_eager_steps_and_follows_sync_lr():
    gen = torch.Generator(device="cuda").manual_seed(37)
    tensors, mk = _capture_setup(gen)
    grads = [[make_grad(t.shape, gen) for t in tensors] for _ in range(5)]
    xyz_lr = [1.6e-4 * 0.8 ** k for k in range(5)]          # update_learning_rate: a new `xyz` rate every iteration
    eager = mk()
    for k in range(5):
        eager.param_groups[0]["lr"] = xyz_lr[k]
        for group, g in zip(eager.param_groups, grads[k]):
            group["params"][0].grad = g.clone()
        eager.step()
    graphed = mk().init_state()
    static = [torch.zeros_like(t) for t in tensors]
    for group, g in zip(graphed.param_groups, static):
        group["params"][0].grad = g
    graphed.sync_lr()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        graphed.step()
    torch.cuda.synchronize()
    assert all(float(graphed.state[g["params"][0]]["step"]) == 0 for g in graphed.param_groups)   # a capture runs nothing
    for k in range(5):
        for s, g in zip(static, grads[k]):
            s.copy_(g)                                    # gradient buffers rewritten in place
        graphed.param_groups[0]["lr"] = xyz_lr[k]
        graphed.sync_lr()
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(triples(eager), triples(graphed)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(float(graphed.state[g["params"][0]]["step"]) == 5 for g in graphed.param_groups)


def test_captured_step_without_sync_lr_keeps_the_old_rate():
    """The contract, pinned: a replay reads lr_tensor(), not param_groups -- a changed Python rate without sync_lr() has no effect."""
    gen = torch.Generator(device="cuda").manual_seed(41)
    tensors, mk = _capture_setup(gen)
    grads = [[make_grad(t.shape, gen) for t in tensors] for _ in range(2)]

    def eager(second_rate):
        opt = mk()
        for k in range(2):
            if k == 1:
                opt.param_groups[0]["lr"] = second_rate
            for group, g in zip(opt.param_groups, grads[k]):
                group["params"][0].grad = g.clone()
            opt.step()
        return triples(opt)
    old_rate, new_rate = LRS[0], 10.0 * LRS[0]
    graphed = mk().init_state()
    static = [torch.zeros_like(t) for t in tensors]
    for group, g in zip(graphed.param_groups, static):
        group["params"][0].grad = g
    graphed.sync_lr()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        graphed.step()
    for k in range(2):
        for s, g in zip(static, grads[k]):
            s.copy_(g)
        if k == 1:
            graphed.param_groups[0]["lr"] = new_rate      # ... and no sync_lr()
        graph.replay()
    torch.cuda.synchronize()
    got = triples(graphed)
    for a, b in zip(eager(old_rate), got):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(eager(new_rate)[0][0], got[0][0])

# ---------------------------------------------------------------------------------------------------------------- whole iteration
def test_whole_training_iteration_as_one_graph():
    """render(fused_loss) -> backward -> statistics -> step in ONE GraphedFrame(verify=False); five replays against five eager
    iterations from the same start.  One Adam update moves a parameter by at most lr (1 - beta1) / sqrt(1 - beta2) ~ 3.2 lr, and
    the backward's float atomics may flip the sign of a near-zero gradient, so the two runs may differ by 5 * 3.2 * lr and no
    tighter bound is derivable."""
    from mygauhuman_amd import densify, human_synth
    from mygauhuman_amd.diff_gaussian_rasterization._C import Phase1Loss
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.graph import GraphedFrame
    W, H, K = 160, 128, 5
    lrs = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=0.05, scaling=5e-3, rotation=1e-3, normal=1e-3, albedo=0.05,
               roughness=0.05)
    gen = torch.Generator(device="cuda").manual_seed(43)
    gt, gt_n = torch.rand((3, H, W), device="cuda", generator=gen), torch.rand((3, H, W), device="cuda", generator=gen)
    bkgd = (torch.rand((1, H, W), device="cuda", generator=gen) > 0.4).float()
    bound = torch.zeros((1, H, W), device="cuda")
    bound[:, H // 6:H - H // 8, W // 5:W - W // 7] = 1.0
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")

    def setup():
        model, body = human_synth.build(4000, None, "cuda", seed=6)
        cam = human_synth.view_camera(body, W, H, 1, n_views=8, device="cuda")
        opt = densify.training_setup(model, lrs, fused_step=True)
        spec = Phase1Loss(gt, gt_n, bkgd, bound)

        def iteration():
            o = render(1, cam, model, pipe, bg, fused_loss=spec)
            o["loss"].backward()
            opt.step(stats=(o["viewspace_points"], o["visibility_filter"], o["radii"], model))
            return o["loss"].detach()
        return model, opt, iteration
    # eager
    model_e, opt_e, it_e = setup()
    for k in range(K):
        opt_e.param_groups[0]["lr"] = lrs["xyz"] * 0.9 ** k
        it_e()
        opt_e.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    # graphed: the constructor's warm-up runs the iteration eagerly, so the start is put back (in place) before the replays
    model_g, opt_g, it_g = setup()
    params = [getattr(model_g, densify.ATTR[g]) for g in densify.GROUPS]
    start = [p.detach().clone() for p in params]
    opt_g.sync_lr()
    frame = GraphedFrame(it_g, warmup=1, zero_grads=params, verify=False)
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
            if p in opt_g.state:
                for key in ("exp_avg", "exp_avg_sq", "step"):
                    opt_g.state[p][key].zero_()
        for t in (model_g.xyz_gradient_accum, model_g.denom, model_g.max_radii2D):
            t.zero_()
    for k in range(K):
        opt_g.param_groups[0]["lr"] = lrs["xyz"] * 0.9 ** k
        opt_g.sync_lr()
        frame.replay()
    torch.cuda.synchronize()
    frame.check()
    identical, stepped = True, 0
    for g in densify.GROUPS:
        pe, pg = getattr(model_e, densify.ATTR[g]).detach(), getattr(model_g, densify.ATTR[g]).detach()
        has_e, has_g = getattr(model_e, densify.ATTR[g]) in opt_e.state, getattr(model_g, densify.ATTR[g]) in opt_g.state
        assert has_e == has_g, g
        if not has_g:      # a group this loss gives no gradient: left out entirely, in both runs
            print(f"whole iteration, {g}: no gradient, not stepped")
            assert torch.equal(pg, start[densify.GROUPS.index(g)]) and torch.equal(pe, pg)
            continue
        stepped += 1
        assert float(opt_g.state[getattr(model_g, densify.ATTR[g])]["step"]) == K
        assert float(opt_e.state[getattr(model_e, densify.ATTR[g])]["step"]) == K
        assert torch.isfinite(pg).all()
        diff = float((pe - pg).abs().max())
        print(f"whole iteration, {g}: max |graph - eager| = {diff:.3e} (bound {K * 3.2 * lrs[g]:.3e})")
        assert diff <= K * 3.2 * lrs[g], g
        identical = identical and torch.equal(pe, pg)
    print("whole iteration: graph and eager parameters bit-identical:", identical)
    assert stepped >= 6
    assert float(model_g.denom.sum()) > 0 and float(model_g.denom.max()) == K
    assert not torch.equal(getattr(model_g, "_xyz").detach(), start[0])
