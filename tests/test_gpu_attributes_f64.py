"""csrc/attributes.hip and csrc/activations.hip against the float64 CPU evaluation of the torch chain they replace
(tests/torch_reference.frame_attributes_torch, the property getters of the model), at the sizes where the kernels branch, on
the edges of the activations, with guard bands around everything the bindings allocate.

The bound is measured (tests/attributes_cases.py): for every tensor the float32 CPU evaluation of the same chain is compared
with the float64 one by the measure of util.assert_close (e32), and the kernel must stay within 2 x e32 + 4 float32 ulps of the
tensor's scale.  Gaussians whose non-differentiable selections lie within attributes_cases.MARGIN of switching (float64 margins;
at most 0.5 % per case, asserted without a GPU in test_attributes_inputs_host.py) are left out of the comparisons that depend on
the selection.

Measured on one MI355X, by that measure.  Per tensor, worst over the cases: e32 = the float32 checker against float64, kernel =
the kernel against float64, k/e32 = the worst ratio of the two within one case, /bound = the worst kernel / (2 e32 + 4 ulp):

    part A (96 shape cases)   e32      kernel   k/e32  /bound     part B (filler rows)   e32      kernel   k/e32  /bound
    cov3D                     7.2e-07  6.9e-07  3.66   0.63       opacity                7.3e-08  7.3e-08  1.00   0.12
    features[:15]             9.8e-08  9.8e-08  1.58   0.16       albedo                 7.9e-08  7.9e-08  1.00   0.12
    axis feature              7.8e-07  8.4e-07  2.38   0.41       scaling                4.5e-08  4.6e-08  1.01   0.08
    colors                    1.7e-07  1.7e-07  1.46   0.21       rotation               9.4e-08  9.4e-08  1.00   0.14
    d_means3D                 5.6e-07  3.3e-07  1.97   0.35       normal                 8.6e-08  9.3e-08  1.07   0.14
    d_transforms              9.6e-07  7.6e-07  3.10   0.79       occlusion              7.3e-08  7.3e-08  1.00   0.12
    d_world_normals           3.6e-07  2.8e-07  3.53   0.28       d_opacity_raw          1.0e-07  7.5e-08  0.75   0.11
    d_scales                  6.3e-07  7.5e-07  2.62   0.50       d_albedo_raw           1.4e-07  1.4e-07  1.00   0.18
    d_rot_cov                 2.6e-06  1.7e-06  2.07   0.77       d_scaling_raw          3.3e-08  3.3e-08  1.00   0.06
    d_rot_axis                3.2e-06  3.5e-06  2.92   0.56       d_rotation_raw         1.1e-07  1.0e-07  0.89   0.15
    d_albedo, d_occlusion     0        0        -      0          d_normal_raw           8.4e-08  9.9e-08  1.18   0.15
    d_roughness               1.0e-07  1.0e-07  1.00   0.15       hand rows, per row: k/e32 <= 4.1 (d_normal_raw, norm
    d_shs                     2.9e-07  4.1e-07  2.03   0.44       1e-10: 8.7e-08 against 2.1e-08), /bound <= 0.27

No tensor needs more than 0.79 of its bound.  Where k/e32 exceeds two, the checker's own error in that case is below two ulps
(P = 1 and P = 63: a handful of elements, the float32 chain happens to round well) and the kernel's error is within the 4-ulp
floor; at the sizes where e32 is at its worst the kernel's error is 0.6 to 1.3 times e32.

Activation edges (part B).  Rows laid out by hand are compared one row at a time (each row has one magnitude; a tensor-wide
scale would be set by exp(88) or by the 1e15 gradients and hide every other row), except the sigmoid rows, which share the
scale of their tensor (about 1).  A row's scale is floored at the smallest normal float32 (1.18e-38): below it float32 has no
relative precision, so a subnormal result (exp(-90) = 8.2e-40) is held to 4 ulps of that floor, i.e. to 4 subnormal steps
(5.6e-45) -- the kernel has to produce the subnormal, as torch's float32 exp does; a result flushed to zero fails.  Rows whose float64 result is not a normal float32 are compared
with that result ROUNDED to float32: sigmoid and its gradient at raw -90 and -104 (8e-40 / 7e-46: subnormal / zero), exp(-90)
and its gradient (subnormal), and the gradient g * exp(88) where |g| > 2.06 (infinite in float32: must be the same infinity).
"""
import numpy as np
import pytest
import torch

from tests import attributes_cases as ac
from tests import util
from tests.test_gpu_guardband import GuardedTorch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def _attr_args(d, sh, cam, view, deg):
    return (d["means3D"], d["transforms"], d["world_normals"], d["scales"], ac.MOD, d["rot_cov"], d["rot_axis"], d["albedo"],
            d["roughness"], d["occlusion"], sh, deg, cam, view)


def _leaves(dnp, layout):
    """Device leaves of the numpy inputs; returns (dict without shs, the shs argument, the SH leaves in order)."""
    t = lambda a: torch.from_numpy(a).to(DEV).requires_grad_(True)  # noqa: E731
    d = {k: t(v) for k, v in dnp.items() if k != "shs"}
    if "shs" not in dnp:
        return d, None, []
    shs = dnp["shs"]
    if layout == "pair":
        dc, rest = t(np.ascontiguousarray(shs[:, :1])), t(np.ascontiguousarray(shs[:, 1:]))
        return d, (dc, rest), [dc, rest]
    if layout == "misaligned":
        P = shs.shape[0]
        flat = torch.zeros(P * 48 + 8, device=DEV)
        leaf = flat[1:1 + P * 48].view(P, 16, 3)
        leaf.copy_(torch.from_numpy(shs))
        leaf = leaf.detach().requires_grad_(True)
        assert leaf.is_contiguous() and leaf.data_ptr() % 16 == 4
        return d, leaf, [leaf]
    leaf = t(shs)
    assert leaf.data_ptr() % 16 == 0
    return d, leaf, [leaf]


def _run_kernel(r, layout, deg):
    from mygauhuman_amd.attributes import frame_attributes
    d, sh, sh_leaves = _leaves(r["d"], layout)
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    cov, col, feat = frame_attributes(*_attr_args(d, sh, dev(r["cam"]), dev(r["view"]), deg))
    loss = (cov * dev(r["ups"]["cov"])).sum() + (feat * dev(r["ups"]["features"])).sum()
    if col is not None:
        loss = loss + (col * dev(r["ups"]["colors"])).sum()
    loss.backward()
    n = lambda x: x.detach().cpu().numpy()  # noqa: E731
    outs = dict(cov3D=n(cov), features=n(feat))
    if col is not None:
        outs["colors"] = n(col)
    grads = {k: n(v.grad) for k, v in d.items()}
    if sh_leaves:
        grads["shs"] = np.concatenate([n(x.grad) for x in sh_leaves], axis=1)
    return outs, grads


@pytest.mark.parametrize("P,layout,M,deg", ac.CASES, ids=[f"P{c[0]}-{c[1]}-M{c[2]}-deg{c[3]}" for c in ac.CASES])
def test_frame_attributes_match_float64(P, layout, M, deg):
    """Every output and every input gradient, measured rule.  Staged (M = 16, aligned or pair) and per-row (other M, misaligned)
    kernels, one thread, one short of / exactly / one past a wave and a 256-thread workgroup, two full workgroups plus one row."""
    r = ac.reference(P, layout, M, deg)
    outs, grads = _run_kernel(r, layout, deg)
    keep = ~r["excluded"]
    ratios = {}
    chk = lambda name, got, w64, w32, rows=None: ac.check_measured(name, got, w64, w32, rows, ratios)  # noqa: E731
    chk("cov3D", outs["cov3D"], r["out64"]["cov3D"], r["out32"]["cov3D"])
    chk("features[:15]", outs["features"][:, :15], r["out64"]["features"][:, :15], r["out32"]["features"][:, :15])
    chk("axis feature", outs["features"][:, 15:], r["out64"]["features"][:, 15:], r["out32"]["features"][:, 15:], keep)
    if M:
        chk("colors", outs["colors"], r["out64"]["colors"], r["out32"]["colors"], keep)
    else:
        assert "colors" not in outs
    for k in r["grad64"]:
        assert np.isfinite(grads[k]).all(), k
        chk("d_" + k, grads[k], r["grad64"][k], r["grad32"][k], keep)
    if M:
        active = (deg + 1) ** 2
        assert not grads["shs"][:, active:].any(), "gradient columns of inactive SH bands must be exactly zero"
        assert not r["grad64"]["shs"][:, active:].any()


def test_degenerate_rows_do_not_disturb_their_neighbours():
    """One launch at P = 257 in which a few rows carry a zero world normal, a position equal to the camera's, or a zero rot_axis
    quaternion: every OTHER row, outputs and gradients, has the bits of the launch in which those rows are ordinary.  (What the
    degenerate rows hold -- NaN from 0/0, as in the torch chain -- is printed, not asserted.)"""
    P, layout, M, deg = 257, "one", 16, 3
    r = ac.reference(P, layout, M, deg)
    bad = {"world_normals": [3, 130], "means3D": [64, 255], "rot_axis": [7, 256]}
    dnp = {k: v.copy() for k, v in r["d"].items()}
    dnp["world_normals"][bad["world_normals"]] = 0.0
    dnp["means3D"][bad["means3D"]] = r["cam"]
    dnp["rot_axis"][bad["rot_axis"]] = 0.0
    base = _run_kernel(r, layout, deg)
    degen = _run_kernel(dict(r, d=dnp), layout, deg)
    rows = sorted(sum(bad.values(), []))
    others = np.ones(P, bool)
    others[rows] = False
    for which, (a, b) in (("output", (base[0], degen[0])), ("gradient", (base[1], degen[1]))):
        for k in a:
            assert np.array_equal(a[k][others].view(np.uint32), b[k][others].view(np.uint32)), f"{which} {k}: an ordinary row changed"
            print(f"{which} {k} of the degenerate rows {rows}:\n{b[k][rows].reshape(len(rows), -1)}")


# ------------------------------------------------------------------------------------------------------ activation edges
SIG_RAW = [0.0, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0]
EXP_RAW = [-90.0, -20.0, 0.0, 20.0, 88.0]
QUAT_NORMS = [1e-20, 1e-15, 1e-13, 1e-10, 1.0, 1e15]        # the first three are below F.normalize's eps = 1e-12: x / eps, g / eps
NORMAL_NORMS = [1e-15, 1e-10, 1e-5, 1.0, 1e5, 1e10, 1e15]
N_HAND = 7


def _edge_inputs(P=257, seed=3):
    rng = np.random.default_rng(seed)
    raw = [rng.normal(0, 1.5, s).astype(np.float32) for s in ((P, 1), (P, 3), (P, 3), (P, 4), (P, 3))]
    raw[0][:7, 0] = SIG_RAW
    raw[1][:7] = np.array(SIG_RAW, np.float32)[:, None]
    raw[2][:5] = np.array(EXP_RAW, np.float32)[:, None]
    for t, norms in ((raw[3], QUAT_NORMS), (raw[4], NORMAL_NORMS)):
        for i, nrm in enumerate(norms):
            u = t[i].astype(np.float64)
            t[i] = (u / np.linalg.norm(u) * nrm).astype(np.float32)
    ups = [rng.normal(0, 1, s).astype(np.float32) for s in ((P, 1), (P, 3), (P, 3), (P, 4), (P, 3), (P, 3))]
    return raw, ups


def _getters(o, a, s, r, n):
    import torch.nn.functional as F
    op = torch.sigmoid(o)
    return op, torch.sigmoid(a), torch.exp(s), F.normalize(r), n / n.norm(dim=1, keepdim=True), op.repeat(1, 3)


def _activations(fn, raw, ups, dtype, dev):
    leaves = [torch.from_numpy(t).to(dev).to(dtype).requires_grad_(True) for t in raw]
    outs = fn(*leaves)
    sum((o * torch.from_numpy(u).to(dev).to(dtype)).sum() for o, u in zip(outs, ups)).backward()
    n64 = lambda x: x.detach().cpu().to(torch.float64).numpy()  # noqa: E731
    return [n64(o) for o in outs], [n64(t.grad) for t in leaves]


def _as_float32_where_not_normal(w64):
    """The float64 result, rounded to float32 where it is no normal float32 (subnormal, zero after rounding, infinite)."""
    w = w64.copy()
    odd = (np.abs(w64) < FLT_MIN) | (np.abs(w64) > FLT_MAX)
    with np.errstate(over="ignore"):
        w[odd] = w64[odd].astype(np.float32).astype(np.float64)
    return w


def _row_measure(got, want):
    scale = max(float(np.abs(want).max()), FLT_MIN)
    return float((np.abs(got - want) / np.maximum(np.abs(want), scale)).max())


def _check_edge_tensor(name, got, w64, w32, per_row):
    want = _as_float32_where_not_normal(w64)
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf]), f"{name}: an overflowing element is not the same infinity"
    assert np.isfinite(got[~inf]).all(), f"{name}: not finite: {got[:N_HAND]}"
    got, want, w32 = (np.where(inf, 0.0, x) for x in (got, want, w32))
    ac.check_measured(name + " (filler rows)", got[N_HAND:], want[N_HAND:], w32[N_HAND:])
    if not per_row:
        ac.check_measured(name + " (hand rows)", got[:N_HAND], want[:N_HAND], w32[:N_HAND])
        return
    for i in range(N_HAND):
        e32, ek = _row_measure(w32[i], want[i]), _row_measure(got[i], want[i])
        tol = 2.0 * e32 + 4.0 * ac.ULP
        print(f"{name} row {i}: want {want[i]}  got {got[i]}  float32 checker {e32:.3e}  kernel {ek:.3e}  bound {tol:.3e}")
        assert ek <= tol, f"{name} row {i}: kernel {ek:.3e} > 2 x {e32:.3e} + 4 ulp; got {got[i]} want {want[i]}"


def test_activation_edges_match_float64():
    """Saturated sigmoid / exp, quaternions on both sides of F.normalize's eps, normals from 1e-15 to 1e15: values and the five
    raw gradients, measured rule (module docstring: which rows are compared per row / with the rounded float64 result)."""
    from mygauhuman_amd.activations import frame_activations
    raw, ups = _edge_inputs()
    o64, g64 = _activations(_getters, raw, ups, torch.float64, "cpu")
    o32, g32 = _activations(_getters, raw, ups, torch.float32, "cpu")
    ok, gk = _activations(frame_activations, raw, ups, torch.float32, DEV)
    names = ("opacity", "albedo", "scaling", "rotation", "normal", "occlusion")
    per_row = (False, False, True, True, True, False)
    for k, name in enumerate(names):
        _check_edge_tensor(name, ok[k], o64[k], o32[k], per_row[k])
    for k, name in enumerate(names[:5]):
        _check_edge_tensor("d_" + name + "_raw", gk[k], g64[k], g32[k], per_row[k])
    # below eps the normalised quaternion is x / eps and its gradient g / eps (the projection term is gone)
    g_rot = ups[3].astype(np.float64)
    for i in range(3):
        np.testing.assert_allclose(ok[3][i], raw[3][i].astype(np.float64) / 1e-12, rtol=4 * ac.ULP)
        np.testing.assert_allclose(gk[3][i], g_rot[i] / 1e-12, rtol=4 * ac.ULP)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("P", [1, 257])
def test_activations_backward_accumulation_input(P):
    """gsr_model_activations_backward_acc called directly: with `acc` given, d_rotation_raw = fl(fl(d) + acc) bit for bit and every
    other output has the bits of the call without it."""
    from mygauhuman_amd._lib import call, ptr
    g = torch.Generator(device="cpu").manual_seed(P)
    rn = lambda *s: torch.randn(s, generator=g).to(DEV)  # noqa: E731
    rot, nrm, op, al, sc = rn(P, 4), rn(P, 3), torch.sigmoid(rn(P, 1)), torch.sigmoid(rn(P, 3)), torch.exp(rn(P, 3))
    gs = [rn(P, 1), rn(P, 3), rn(P, 3), rn(P, 4), rn(P, 3), rn(P, 3)]
    acc = rn(P, 4) * 3.0
    res = {}
    for with_acc in (False, True):
        outs = [torch.full(s, float("nan"), device=DEV) for s in ((P, 1), (P, 3), (P, 3), (P, 4), (P, 3))]
        call("gsr_model_activations_backward_acc", torch.device(DEV, 0), P, ptr(rot), ptr(nrm), ptr(op), ptr(al), ptr(sc),
             *[ptr(x) for x in gs], *[ptr(o) for o in outs], ptr(acc) if with_acc else None)
        res[with_acc] = outs
    assert _bits_equal(res[True][3], res[False][3] + acc)
    assert not _bits_equal(res[True][3], res[False][3])
    for k in (0, 1, 2, 4):
        assert _bits_equal(res[True][k], res[False][k]), k


@pytest.mark.parametrize("P", [1, 257])
@pytest.mark.parametrize("layout", ["one", "pair", "misaligned"])
def test_attributes_backward_accumulation_input(P, layout):
    """gsr_frame_attributes_backward_acc called directly: with acc_dmeans3D given, d_means = fl(fl(d) + acc) bit for bit and every
    other gradient has the bits of the call without it (staged single-array, staged pair and per-row kernels)."""
    from mygauhuman_amd._lib import call, ptr
    r = ac.reference(P, layout, 16, 3)
    d, sh, sh_leaves = _leaves(r["d"], layout)
    x = {k: v.detach() for k, v in d.items()}
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    cam, view, ups = dev(r["cam"]), dev(r["view"]), {k: dev(v) for k, v in r["ups"].items()}
    shs, rest = (sh_leaves[0].detach(), sh_leaves[1].detach() if layout == "pair" else None)
    acc = torch.randn((P, 3), generator=torch.Generator(device="cpu").manual_seed(P)).to(DEV)
    res = {}
    for with_acc in (False, True):
        shapes = [(P, 3), (P, 9), (P, 3), (P, 3), (P, 4), (P, 4), (P, 3), (P, 3), (P, 3), tuple(shs.shape)] + ([tuple(rest.shape)] if rest is not None else [])
        outs = [torch.full(s, float("nan"), device=DEV) for s in shapes]
        call("gsr_frame_attributes_backward_acc", torch.device(DEV, 0), P, 3, 16, ptr(x["means3D"]), ptr(x["transforms"]),
             ptr(x["world_normals"]), ptr(x["scales"]), ac.MOD, ptr(x["rot_cov"]), ptr(x["rot_axis"]), ptr(x["albedo"]),
             ptr(x["roughness"]), ptr(x["occlusion"]), ptr(shs), ptr(rest), ptr(cam), ptr(view), ptr(ups["cov"]), ptr(ups["colors"]),
             ptr(ups["features"]), *[ptr(o) for o in outs[:10]], ptr(outs[10]) if rest is not None else None,
             ptr(acc) if with_acc else None)
        res[with_acc] = outs
    assert _bits_equal(res[True][0], res[False][0] + acc)
    assert not _bits_equal(res[True][0], res[False][0])
    for k in range(1, len(res[True])):
        assert not torch.isnan(res[False][k]).any(), k
        assert _bits_equal(res[True][k], res[False][k]), k


# ------------------------------------------------------------------------------------------------------ guard bands
@pytest.fixture()
def guarded_attr(monkeypatch):
    from mygauhuman_amd import activations, attributes
    g = GuardedTorch()
    monkeypatch.setattr(attributes, "torch", g)
    monkeypatch.setattr(activations, "torch", g)
    return g


class _Sink:
    def __init__(self):
        self.n = 0

    def collect(self, colors, g_colors, means3D):
        self.n += 1


@pytest.mark.parametrize("P", [1, 255, 257, 777])
@pytest.mark.parametrize("layout,M,sink", [("one", 16, False), ("pair", 16, False), ("one", 4, False), ("one", 16, True), ("pair", 16, True)],
                         ids=["M16", "M16pair", "M4", "M16-no-sh-grad", "M16pair-no-sh-grad"])
def test_attribute_and_activation_writes_stay_inside_their_arrays(guarded_attr, P, layout, M, sink):
    """4 KB margins around every output and gradient tensor of frame_attributes and frame_activations stay intact: the ragged last
    workgroup of the staged backward leaves d_shs / d_rest through float4 block stores plus a scalar tail.  `sink`: the SH
    gradient is not wanted (detached SH tensors under an installed sh_gradient_sink)."""
    from mygauhuman_amd import attributes
    from mygauhuman_amd.activations import frame_activations
    deg = 3 if M == 16 else 1
    dnp, cam, view, ups = ac.make_inputs(P, M, 50 + P)
    d, sh, sh_leaves = _leaves(dnp, layout)
    if sink:
        sh = tuple(x.detach() for x in sh) if layout == "pair" else sh.detach()
    dev = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    the_sink = _Sink()
    with attributes.sh_gradient_sink(the_sink if sink else None):
        cov, col, feat = attributes.frame_attributes(*_attr_args(d, sh, dev(cam), dev(view), deg))
    assert guarded_attr.check("attributes forward") == 3
    ((cov * dev(ups["cov"])).sum() + (col * dev(ups["colors"])).sum() + (feat * dev(ups["features"])).sum()).backward()
    assert guarded_attr.check("attributes backward") == 9 + (0 if sink else len(sh_leaves))
    assert the_sink.n == int(sink)
    for x in sh_leaves:
        assert (x.grad is None) == sink
    raw = [torch.randn(P, k, device=DEV, requires_grad=True) for k in (1, 3, 3, 4, 3)]
    outs = frame_activations(*raw)
    assert guarded_attr.check("activations forward") == 6
    sum((o * torch.randn_like(o)).sum() for o in outs).backward()
    assert guarded_attr.check("activations backward") == 5


def test_misaligned_rest_of_an_sh_pair_raises():
    """(dc, rest) with a `rest` that is not 16-byte aligned: the library's error, not a misaligned float4 read."""
    from mygauhuman_amd._lib import GsrError
    from mygauhuman_amd.attributes import frame_attributes
    P = 65
    dnp, cam, view, _ = ac.make_inputs(P, 16, 1)
    d, _, _ = _leaves(dnp, "one")
    dc = torch.from_numpy(np.ascontiguousarray(dnp["shs"][:, :1])).to(DEV)
    flat = torch.zeros(P * 45 + 8, device=DEV)
    rest = flat[1:1 + P * 45].view(P, 15, 3)
    rest.copy_(torch.from_numpy(dnp["shs"][:, 1:]))
    assert rest.is_contiguous() and rest.data_ptr() % 16 == 4
    with pytest.raises(GsrError, match="16-byte aligned"):
        frame_attributes(*_attr_args(d, (dc, rest), torch.from_numpy(cam).to(DEV), torch.from_numpy(view).to(DEV), 3))
