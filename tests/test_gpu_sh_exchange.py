"""The six kernels of csrc/sh_exchange.hip, called through the C ABI on synthetic blocks (no rasterizer session, no process
group), against the float64 / bit-exact CPU references of tests/sh_exchange_reference.py (pinned without a GPU by
test_sh_exchange_reference_host.py):

  gsr_sh_grad_from_views         <STAGE, SPLIT> = <true, false> (M = 16, aligned) and <false, false> (misaligned or M != 16)
  gsr_sh_grad_from_views_posed   <true, true>: dc [P,1,3] + rest [P,15,3], float4 stores with a scalar tail of nrows * 45 % 4
  gsr_sh_view_pack_posed, gsr_step_finish, gsr_step_status: bit for bit

P runs over sh_exchange_reference.P_LIST: one thread, a wave and a 256-row block +- 1, and 257 .. 260 / 513 / 1027 so that the
last block holds 1, 2, 3, 4 rows (nrows * 45 % 4 = 1, 2, 3, 0); 1, 2 and 8 views; degrees 0 to 3.  Every output is a slice of a
larger allocation filled with a sentinel, checked after the call (as in test_gpu_guardband.py); floats of a view block that
belong to no part hold NaN.

The bound of the reconstruction is measured (sh_exchange_reference.check_measured): per case e32 = the worst error of the same
formula in numpy float32 against float64, relative to the largest magnitude of the Gaussian's row; every element of the kernel's
result has to lie within (2 e32 + 4 ulp) x its row's largest magnitude of the float64 value.  Nothing is excluded: these kernels
have no discontinuity (the clamp mask is an input).

The three instantiations share one arithmetic body and, fed the same numbers, agree bit for bit
(test_three_instantiations_agree_bit_for_bit); so do the two strides and the two posed layouts.

Measured on one MI355X.  Per group of cases, worst over the cases: e32 = the float32 twin against float64, kernel = the kernel
against float64 (both relative to the row's largest magnitude), share = the worst |error| / bound of any element:

    group                                             cases   e32      kernel   share
    static <true,false> (two strides each)            180     7.0e-06  3.2e-06  0.35
    static <false,false>, M = 16 misaligned           180     7.0e-06  3.2e-06  0.35
    static <false,false>, M = 9 / 4 / 1               135/90/45  7.0e-06  3.2e-06  0.35 / 0.33 / 0.33
    posed <true,true> (two layouts each)              180     7.0e-06  3.2e-06  0.39
    posed <true,true>, shared positions               180     7.0e-06  3.2e-06  0.35
    scale_h, scale_h x dev_scale, degenerate rows     22      4.7e-07  3.9e-07  0.31
    test_gpu_parallel.py, rasterizer-made blocks      4       2.1e-06  1.8e-06  0.46 (plain path: 0.45)

No kernel needs more than 0.46 of its bound.  The largest e32 (58 ulp of the row: P = 513, degree 0, two views) belongs to a
row whose two packed gradients almost cancel: the float32 sum is accurate relative to its terms, not to the cancelled result, and
the kernel's error in that row is half the twin's; in the typical case e32 is 2 to 4 ulp (degree 3), the bound 8 to 12 ulp of the
row.
"""
import numpy as np
import pytest
import torch

from tests import sh_exchange_reference as xr

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096   # bytes in front of and behind every output
GSR_EINVAL = -1
NAN = float("nan")
GRID = [(P, deg, v) for P in xr.P_LIST for deg in range(4) for v in xr.VIEWS_LIST]
GRID_IDS = [f"P{P}-deg{d}-views{v}" for P, d, v in GRID]


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


def _to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Guarded:
    """n floats `offset` floats past a 16-byte boundary, inside an allocation whose every other float holds the sentinel.  The
    payload starts as `fill` (NaN: an element the kernel does not write shows)."""

    def __init__(self, n, offset=0, fill=NAN):
        self.first, self.n = GUARD // 4 + offset, n
        self.whole = torch.full((self.first + n + GUARD // 4,), xr.SENTINEL_BITS - (1 << 32), dtype=torch.int32, device=DEV).view(torch.float32)
        self.t = self.whole[self.first:self.first + n]
        if fill is not None:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 4 * (offset % 4)

    def ptr(self):
        return self.t.data_ptr()

    def numpy(self, what):
        """The payload, after checking that the sentinels in front of and behind it are intact."""
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy().view(np.uint32)
        front, back = w[:self.first] != xr.SENTINEL_BITS, w[self.first + self.n:] != xr.SENTINEL_BITS
        assert not front.any(), f"{what}: write {4 * (self.first - int(np.flatnonzero(front).max()))} bytes IN FRONT of the {self.n}-float output"
        assert not back.any(), f"{what}: write {4 * int(np.flatnonzero(back).min())} bytes BEHIND the {self.n}-float output"
        return w[self.first:self.first + self.n].view(np.float32).copy()


def _dev_scalar(x):
    return None if x is None else torch.tensor([x], dtype=torch.float32, device=DEV)


def run_static(P, deg, M, views, stride, means, scale_h, dev_scale=None, offset=0):
    """gsr_sh_grad_from_views -> [P, M, 3]; offset: floats the output sits past a 16-byte boundary."""
    from mygauhuman_amd._lib import call
    out = Guarded(P * M * 3, offset)
    v, m, ds = _to_dev(views), _to_dev(means), _dev_scalar(dev_scale)
    call("gsr_sh_grad_from_views", _dev(), P, deg, M, v.numel() // stride, m.data_ptr(), v.data_ptr(), stride, scale_h,
         None if ds is None else ds.data_ptr(), out.ptr())
    return out.numpy(f"gsr_sh_grad_from_views P={P} M={M} offset={offset}").reshape(P, M, 3)


def run_posed(P, deg, views, stride, means_off, cam_off, scale_h, dev_scale=None):
    """gsr_sh_grad_from_views_posed -> cat(dc, rest) [P, 16, 3]."""
    from mygauhuman_amd._lib import call
    dc, rest = Guarded(P * 3), Guarded(P * 45)
    v, ds = _to_dev(views), _dev_scalar(dev_scale)
    call("gsr_sh_grad_from_views_posed", _dev(), P, deg, v.numel() // stride, v.data_ptr(), stride, means_off, cam_off, scale_h,
         None if ds is None else ds.data_ptr(), dc.ptr(), rest.ptr())
    what = f"gsr_sh_grad_from_views_posed P={P}"
    return np.concatenate([dc.numpy(what + " dc").reshape(P, 1, 3), rest.numpy(what + " rest").reshape(P, 15, 3)], axis=1)


def _static_views(P, n_views, kind):
    g, means, _, cams = xr.make_inputs(P, n_views)
    stride, mo, co = xr.static_layout(P, kind)
    return xr.build_views(g, None, cams, stride, mo, co), stride, means


def _posed_views(P, n_views, kind, shared=False):
    g, means, per_view, cams = xr.make_inputs(P, n_views)
    stride, mo, co = xr.posed_layout(P, kind)
    return xr.build_views(g, np.broadcast_to(means, per_view.shape) if shared else per_view, cams, stride, mo, co), stride, mo, co


def _inactive_bands_are_zero(got, deg):
    assert not _bits(got[:, (deg + 1) ** 2:]).any(), "bands above the active degree must be exactly +0"


# ------------------------------------------------------------------------------------------------------ reconstruction
@pytest.mark.parametrize("P,deg,n_views", GRID, ids=GRID_IDS)
def test_static_entry_staged_matches_float64(P, deg, n_views):
    """M = 16, aligned output: <true, false>, with CompactShExchange's stride (a multiple of 64 floats) and with the smallest
    the ABI accepts (3 P + 3)."""
    want, twin = xr.reference(P, deg, n_views, False)
    scale = float(np.float32(1.0 / n_views))
    got = {}
    for kind in ("padded", "tight"):
        views, stride, means = _static_views(P, n_views, kind)
        assert (stride % 64 == 0) == (kind == "padded")
        got[kind] = run_static(P, deg, 16, views, stride, means, scale)
        xr.check_measured(f"static <true,false> {kind}", got[kind], want, twin)
        _inactive_bands_are_zero(got[kind], deg)
    assert np.array_equal(_bits(got["padded"]), _bits(got["tight"]))


@pytest.mark.parametrize("P,deg,n_views", GRID, ids=GRID_IDS)
def test_static_entry_per_row_matches_float64(P, deg, n_views):
    """<false, false>: M = 16 with the output one float past a 16-byte boundary, and every M in {1, 4, 9} that holds the degree."""
    want, twin = xr.reference(P, deg, n_views, False)
    scale = float(np.float32(1.0 / n_views))
    views, stride, means = _static_views(P, n_views, "tight")
    got = run_static(P, deg, 16, views, stride, means, scale, offset=1)
    xr.check_measured("static <false,false> misaligned", got, want, twin)
    _inactive_bands_are_zero(got, deg)
    views, stride, means = _static_views(P, n_views, "padded")
    for M in (1, 4, 9):
        if M >= (deg + 1) ** 2:
            got = run_static(P, deg, M, views, stride, means, scale, offset=M % 4)
            xr.check_measured(f"static <false,false> M={M}", got, want[:, :M], twin[:, :M])
            _inactive_bands_are_zero(got, deg)


@pytest.mark.parametrize("P,deg,n_views", GRID, ids=GRID_IDS)
def test_posed_entry_matches_float64(P, deg, n_views):
    """<true, true>: positions that differ per view, in CompactShExchange(posed=True)'s layout and in one with gaps between the
    parts; cat(dc, rest) against the reference."""
    want, twin = xr.reference(P, deg, n_views, True)
    scale = float(np.float32(1.0 / n_views))
    got = {}
    for kind in ("compact", "gap"):
        views, stride, mo, co = _posed_views(P, n_views, kind)
        got[kind] = run_posed(P, deg, views, stride, mo, co, scale)
        xr.check_measured(f"posed <true,true> {kind}", got[kind], want, twin)
        _inactive_bands_are_zero(got[kind], deg)
    assert np.array_equal(_bits(got["compact"]), _bits(got["gap"]))


def test_posed_layout_is_the_one_of_the_exchange_object():
    from mygauhuman_amd.parallel import CompactShExchange
    for P in (1, 257, 1027):
        ex = CompactShExchange(P, 16, DEV, posed=True)
        assert (ex.stride, ex.means_off, ex.cam_off) == xr.posed_layout(P, "compact")
        ex = CompactShExchange(P, 16, DEV)
        assert (ex.stride, 0, 3 * P) == xr.static_layout(P, "padded")


@pytest.mark.parametrize("P,deg,n_views", GRID, ids=GRID_IDS)
def test_three_instantiations_agree_bit_for_bit(P, deg, n_views):
    """The same numbers -- the shared positions copied into every posed block -- through <true,true>, <true,false> and
    <false,false>: one arithmetic body, identical bits (and each within the float64 bound, by the tests above)."""
    scale = float(np.float32(1.0 / n_views))
    views, stride, means = _static_views(P, n_views, "padded")
    staged = run_static(P, deg, 16, views, stride, means, scale)
    per_row = run_static(P, deg, 16, views, stride, means, scale, offset=1)
    pviews, pstride, mo, co = _posed_views(P, n_views, "compact", shared=True)
    split = run_posed(P, deg, pviews, pstride, mo, co, scale)
    assert np.array_equal(_bits(staged), _bits(per_row)), "<true,false> and <false,false> differ"
    assert np.array_equal(_bits(staged), _bits(split)), "<true,false> and <true,true> differ"
    xr.check_measured("posed <true,true> shared positions", split, *xr.reference(P, deg, n_views, False))


VARIANTS = ("static-staged", "static-per-row", "posed")


def _run_variant(variant, P, deg, n_views, scale_h, dev_scale, nan_blocks=False):
    if variant == "posed":
        views, stride, mo, co = _posed_views(P, n_views, "compact")
        views = np.full_like(views, np.nan) if nan_blocks else views
        return run_posed(P, deg, views, stride, mo, co, scale_h, dev_scale)
    views, stride, means = _static_views(P, n_views, "padded")
    views = np.full_like(views, np.nan) if nan_blocks else views
    return run_static(P, deg, 16, views, stride, means, scale_h, dev_scale, offset=int(variant == "static-per-row"))


@pytest.mark.parametrize("P", [3, 257, 260])
@pytest.mark.parametrize("variant", VARIANTS)
def test_scale_and_device_scale(variant, P):
    """dev_scale = None: scale_h alone; a device scalar multiplies it (one float32 product); a device scalar of 0 gives exact,
    finite zeros whatever the blocks hold -- they are filled with NaN here."""
    deg, n_views = 3, 2
    posed = variant == "posed"
    h = float(np.float32(0.6))
    got = _run_variant(variant, P, deg, n_views, h, None)
    xr.check_measured(f"{variant} scale_h", got, *xr.reference(P, deg, n_views, posed, scale=h))
    d = float(np.float32(0.37))
    got = _run_variant(variant, P, deg, n_views, h, d)
    xr.check_measured(f"{variant} scale_h x dev_scale", got, *xr.reference(P, deg, n_views, posed, scale=h * d))
    for nan_blocks in (False, True):
        got = _run_variant(variant, P, deg, n_views, h, 0.0, nan_blocks)
        assert not _bits(got).any(), f"dev_scale = 0 must give +0 everywhere (NaN blocks: {nan_blocks})"
    got = _run_variant(variant, P, deg, n_views, 0.0, None, True)
    assert not _bits(got).any(), "scale = 0 must give +0 everywhere"


@pytest.mark.parametrize("variant,case", [(v, "at-camera") for v in VARIANTS] + [("posed", "nan-position")])
def test_degenerate_positions_of_a_dead_view_do_not_reach_the_sum(variant, case):
    """A Gaussian exactly AT one view's camera position (direction 0 / 0), or with a NaN position riding in a posed block, whose
    packed gradient in that view is all zero (culled / invisible there): the view contributes nothing and the row is the finite
    float64 value of the other views, as in the all-reduced path, which never forms a direction for an invisible Gaussian."""
    P, deg, n_views = 257, 3, 3
    posed = variant == "posed"
    g, means, per_view, cams = (np.array(a) for a in xr.make_inputs(P, n_views))
    rows = [0, 63, 64, 255, 256]
    for j, i in enumerate(rows):
        v = j % n_views
        g[:, i] = [[1.0, -0.5, 0.25], [0.0, 2.0, 0.0], [-1.5, 0.0, 0.75]]
        g[v, i] = 0.0
        if posed:
            per_view[v, i] = cams[v] if case == "at-camera" else np.nan
        else:
            means[i] = cams[v]
    if posed:
        stride, mo, co = xr.posed_layout(P, "compact")
        views = xr.build_views(g, per_view, cams, stride, mo, co)
        args = (P, deg, 16, views, stride, None, mo, co, 0.5)
        got = run_posed(P, deg, views, stride, mo, co, 0.5)
    else:
        stride, mo, co = xr.static_layout(P, "padded")
        views = xr.build_views(g, None, cams, stride, mo, co)
        args = (P, deg, 16, views, stride, means, mo, co, 0.5)
        got = run_static(P, deg, 16, views, stride, means, 0.5, offset=int(variant == "static-per-row"))
    want, twin = xr.grad_from_views64(*args), xr.grad_from_views32(*args)
    assert np.isfinite(want).all() and (np.abs(want[rows]).max(axis=(1, 2)) > 0).all()
    print("degenerate rows:", got[rows, :2].reshape(len(rows), -1))
    xr.check_measured(f"{variant} {case}", got, want, twin)


# ------------------------------------------------------------------------------------------------------ the posed pack
def _pack_layouts(P):
    return [xr.posed_layout(P, "compact"), xr.posed_layout(P, "gap")]


@pytest.mark.parametrize("P", [1, 2, 85, 86, 257])
def test_view_pack_posed_is_bit_exact(P):
    """packed = colour > 0 ? gradient : +0 with colours that are positive, +0, -0, the smallest denormal and negative; positions
    and camera copied bit for bit; every other float of the block (radii, padding, gaps) and of the allocation keeps its
    sentinel.  3 P = 255 / 258 floats: one short of / past the first 256-thread block."""
    from mygauhuman_amd._lib import call
    rng = np.random.default_rng(P)
    colors = np.abs(rng.normal(0, 1, (P, 3))).astype(np.float32)
    plant = np.array([0.0, -0.0, 1e-45, -1.0, -1e-45, 2.0], np.float32)
    colors.reshape(-1)[:min(3 * P, 6)] = plant[:min(3 * P, 6)]
    colors.reshape(-1)[-3:] = plant[:3] if P > 2 else colors.reshape(-1)[-3:]
    g = rng.normal(0, 1, (P, 3)).astype(np.float32)
    g.reshape(-1)[0] = -0.0 if P > 1 else g.reshape(-1)[0]
    means = rng.normal(0, 1, (P, 3)).astype(np.float32)
    campos = rng.normal(0, 4, 3).astype(np.float32)
    assert _bits(colors.reshape(-1)[:3]).tolist() == [0, 0x80000000, 1]
    for stride, mo, co in _pack_layouts(P):
        blk = Guarded(stride, fill=None)
        d = [_to_dev(a) for a in (colors, g, means, campos)]
        call("gsr_sh_view_pack_posed", _dev(), P, *[t.data_ptr() for t in d], blk.ptr(), mo, co)
        got = blk.numpy(f"gsr_sh_view_pack_posed P={P}")
        want = xr.pack_posed_ref(colors, g, means, campos, xr.sentinel(stride), mo, co)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, f"stride {stride}: floats {bad[:8]} differ: got {got[bad[:8]]} want {want[bad[:8]]}"
        assert int((_bits(want) == xr.SENTINEL_BITS).sum()) == stride - 6 * P - 3


def test_view_pack_posed_with_no_gaussians_writes_the_camera_only():
    from mygauhuman_amd._lib import call
    campos = np.array([1.5, -2.5, 3.5], np.float32)
    blk, cam = Guarded(64, fill=None), _to_dev(campos)
    call("gsr_sh_view_pack_posed", _dev(), 0, None, None, None, cam.data_ptr(), blk.ptr(), 0, 5)
    want = xr.sentinel(64).copy()
    want[5:8] = campos
    assert np.array_equal(_bits(blk.numpy("gsr_sh_view_pack_posed P=0")), _bits(want))


def test_exchange_entry_points_refuse_bad_arguments():
    from mygauhuman_amd._lib import lib
    s = torch.cuda.current_stream().cuda_stream
    buf = Guarded(4096, fill=0.0)
    p = buf.ptr()
    P = 8
    bad_posed_pack = [(-1, p, p, p, p, p, 24, 48), (P, None, p, p, p, p, 24, 48), (P, p, p, p, None, p, 24, 48), (P, p, p, p, p, None, 24, 48),
                      (P, p, p, p, p, p, 23, 48), (P, p, p, p, p, p, 24, 47)]
    for a in bad_posed_pack:
        assert lib.gsr_sh_view_pack_posed(*a, s) == GSR_EINVAL, a
    bad_static = [(P, 4, 16, 1, p, p, 64, 1.0, None, p), (P, 2, 4, 1, p, p, 64, 1.0, None, p), (P, 1, 17, 1, p, p, 64, 1.0, None, p),
                  (P, 1, 16, 0, p, p, 64, 1.0, None, p), (P, 1, 16, 1, p, p, 26, 1.0, None, p), (P, 1, 16, 1, None, p, 64, 1.0, None, p),
                  (P, 1, 16, 1, p, None, 64, 1.0, None, p), (P, 1, 16, 1, p, p, 64, 1.0, None, None)]
    for a in bad_static:
        assert lib.gsr_sh_grad_from_views(*a, s) == GSR_EINVAL, a
    bad_posed = [(P, 3, 1, p, 64, 23, 48, 1.0, None, p, p), (P, 3, 1, p, 64, 24, 62, 1.0, None, p, p), (P, 3, 1, p, 64, 48, 56, 1.0, None, p, p),
                 (P, 3, 1, p, 64, 24, 48, 1.0, None, p, p + 4), (P, 3, 1, None, 64, 24, 48, 1.0, None, p, p)]
    for a in bad_posed:
        assert lib.gsr_sh_grad_from_views_posed(*a, s) == GSR_EINVAL, a
    assert not buf.numpy("refused calls").any(), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------ gsr_step_finish
FINISH_N = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 1024 * 1024 + 3]
SLOTS = (0.0, 1.0, 3.0)
INV_WORLDS = (1.0, 0.5, 0.125)


def _slot_positions(n):
    """0, n - 1, each residue mod 4 inside a middle group of four and inside the tail group."""
    mid, tail = (n // 4) // 2 * 4, n // 4 * 4
    return sorted({0, n - 1} | {mid + r for r in range(4) if mid + r < n} | {tail + r for r in range(n % 4)})


@pytest.mark.parametrize("n", FINISH_N)
def test_step_finish_is_bit_exact(n):
    """Every element but the slot times (slot > 0 ? 0 : inv_world), the slot's bits unchanged, scale and the report words, guard
    bands around the bucket.  n <= 7: scalar paths only; 1023 .. 1025: the last float4 / the tail next to a block edge;
    4 Mi + 3 floats: more than 1024 workgroups of 1024 floats, the strided loop."""
    from mygauhuman_amd._lib import call
    rng = np.random.default_rng(n % 1000)
    base = rng.normal(0, 1, n).astype(np.float32)
    base[rng.uniform(0, 1, n) < 0.05] = 0.0
    pristine = _to_dev(base)
    status = torch.tensor([123456, 7], dtype=torch.int32, device=DEV)
    k = 0
    for idx in _slot_positions(n):
        for slot in SLOTS:
            for inv in INV_WORLDS:
                k += 1
                with_status = k % 2 == 0
                bucket = Guarded(n, fill=None)
                bucket.t.copy_(pristine)
                bucket.t[idx] = slot
                scale = Guarded(1)
                report = torch.full((5,), -1, dtype=torch.int32, device=DEV)
                call("gsr_step_finish", _dev(), status.data_ptr() if with_status else None, bucket.ptr(), n, idx, inv, scale.ptr(),
                     report.data_ptr() + 4)
                flat = base.copy()
                flat[idx] = slot
                want, want_scale, ranks = xr.step_finish_ref(flat, idx, inv)
                what = f"n={n} slot {slot} at {idx}, inv_world {inv}"
                got = bucket.numpy(what)
                assert _bits(got[idx:idx + 1])[0] == _bits(np.float32(slot).reshape(1))[0], f"{what}: the slot changed to {got[idx]}"
                bad = np.flatnonzero(_bits(got) != _bits(want))
                assert bad.size == 0, f"{what}: {bad.size} floats differ, first at {bad[:4]}: got {got[bad[:4]]} want {want[bad[:4]]}"
                assert _bits(scale.numpy(what)).tolist() == _bits(want_scale.reshape(1)).tolist()
                assert report.cpu().tolist() == [-1, ranks, 123456 if with_status else 0, 7 if with_status else 0, -1], what


@pytest.mark.parametrize("n", [5, 1025])
def test_step_finish_accepts_null_scale_and_report(n):
    from mygauhuman_amd._lib import call
    base = np.random.default_rng(n).normal(0, 1, n).astype(np.float32)
    base[n - 2] = 0.0
    for scale_given, report_given in ((False, False), (True, False), (False, True)):
        bucket = Guarded(n, fill=None)
        bucket.t.copy_(_to_dev(base))
        scale, report = Guarded(1), torch.full((3,), -1, dtype=torch.int32, device=DEV)
        call("gsr_step_finish", _dev(), None, bucket.ptr(), n, n - 2, 0.25, scale.ptr() if scale_given else None,
             report.data_ptr() if report_given else None)
        assert np.array_equal(_bits(bucket.numpy("null scale / report")), _bits(xr.step_finish_ref(base, n - 2, 0.25)[0]))
        assert report.cpu().tolist() == ([0, 0, 0] if report_given else [-1, -1, -1])
        assert np.isnan(scale.numpy("scale")[0]) != scale_given


def test_step_finish_refusals_launch_nothing():
    from mygauhuman_amd._lib import lib
    s = torch.cuda.current_stream().cuda_stream
    n = 16
    bucket = Guarded(n + 1, fill=2.0)
    scale, report = Guarded(1), torch.full((3,), -1, dtype=torch.int32, device=DEV)
    rp = report.data_ptr()
    assert lib.gsr_step_finish(None, bucket.ptr(), n, n, 0.5, scale.ptr(), rp, s) == GSR_EINVAL          # overflow_index >= n
    assert lib.gsr_step_finish(None, bucket.ptr(), n, n + 7, 0.5, scale.ptr(), rp, s) == GSR_EINVAL
    assert lib.gsr_step_finish(None, bucket.ptr(), 0, 0, 0.5, scale.ptr(), rp, s) == GSR_EINVAL          # an empty bucket has no slot
    assert lib.gsr_step_finish(None, bucket.ptr() + 4, n, 3, 0.5, scale.ptr(), rp, s) == GSR_EINVAL      # not 16-byte aligned
    assert lib.gsr_step_finish(None, None, n, 3, 0.5, scale.ptr(), rp, s) == GSR_EINVAL                  # null bucket
    assert b"gsr_step_finish" in lib.gsr_last_error()
    assert (bucket.numpy("refused gsr_step_finish") == 2.0).all() and np.isnan(scale.numpy("scale")[0])
    assert report.cpu().tolist() == [-1, -1, -1]


# ------------------------------------------------------------------------------------------------------ gsr_step_status
@pytest.mark.parametrize("phase", [0, 1, 2])
@pytest.mark.parametrize("flag", [0, 1, 7])
def test_step_status_truth_table(phase, flag):
    """phase 0: slot = flag != 0; phase 1: scale and report from the (reduced) slot, which stays; phase 2: both."""
    from mygauhuman_amd._lib import call
    for slot0 in (0.0, 2.0):
        for inv in (1.0, 0.25):
            status = torch.tensor([4321, flag], dtype=torch.int32, device=DEV)
            slot, scale = Guarded(1, fill=slot0), Guarded(1)
            report = torch.full((5,), -1, dtype=torch.int32, device=DEV)
            call("gsr_step_status", _dev(), phase, status.data_ptr(), slot.ptr(), inv, scale.ptr(), report.data_ptr() + 4)
            want_slot, want_scale, want_report = xr.step_status_ref(phase, (4321, flag), np.float32(slot0), inv)
            what = f"phase {phase} flag {flag} slot {slot0} inv_world {inv}"
            assert slot.numpy(what)[0] == want_slot, what
            if phase == 0:
                assert np.isnan(scale.numpy(what)[0]) and report.cpu().tolist() == [-1] * 5, what
            else:
                assert _bits(scale.numpy(what)).tolist() == _bits(want_scale.reshape(1)).tolist(), what
                assert report.cpu().tolist() == [-1] + want_report + [-1], what
            assert status.cpu().tolist() == [4321, flag]


def test_step_status_phase_0_takes_null_scale_and_report_and_refusals_launch_nothing():
    from mygauhuman_amd._lib import call, lib
    s = torch.cuda.current_stream().cuda_stream
    status = torch.tensor([1, 1], dtype=torch.int32, device=DEV)
    slot, scale = Guarded(1, fill=5.0), Guarded(1)
    report = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    sp, rp = status.data_ptr(), report.data_ptr()
    for a in ((-1, sp, slot.ptr(), 0.5, scale.ptr(), rp), (3, sp, slot.ptr(), 0.5, scale.ptr(), rp), (0, None, slot.ptr(), 0.5, scale.ptr(), rp),
              (0, sp, None, 0.5, scale.ptr(), rp), (1, sp, slot.ptr(), 0.5, None, rp), (1, sp, slot.ptr(), 0.5, scale.ptr(), None),
              (2, sp, slot.ptr(), 0.5, None, rp), (2, sp, slot.ptr(), 0.5, scale.ptr(), None)):
        assert lib.gsr_step_status(*a, s) == GSR_EINVAL, a
    assert slot.numpy("refused gsr_step_status")[0] == 5.0 and np.isnan(scale.numpy("scale")[0]) and report.cpu().tolist() == [-1] * 3
    call("gsr_step_status", _dev(), 0, sp, slot.ptr(), 0.5, None, None)
    assert slot.numpy("phase 0")[0] == 1.0
