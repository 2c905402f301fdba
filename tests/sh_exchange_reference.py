"""CPU references of csrc/sh_exchange.hip (the compact SH-gradient exchange of the view-parallel ranks and the step's
bookkeeping kernels), float64 / bit-exact numpy, no GPU: shared by test_gpu_sh_exchange.py, test_gpu_parallel.py and
test_sh_exchange_reference_host.py (which pins this file against autograd).

  basis64            the 16 SH weights of a direction, from the project's own polynomial (sh_utils.eval_sh applied to the unit
                     coefficient vectors -- nothing is restated here)
  grad_from_views64  what gsr_sh_grad_from_views / _posed compute, float64
  grad_from_views32  the same formula in numpy float32 throughout: the checker's own arithmetic, used ONLY to size the bound
  pack_posed_ref     gsr_sh_view_pack_posed, bit-exact
  step_finish_ref    gsr_step_finish, bit-exact (one float32 multiply per element)
  step_status_ref    gsr_step_status

The bound (bound_for) is measured, not chosen, after tests/attributes_cases.py: per case e32 = the float32 twin's worst error
against float64, and the kernel may be off by 2 x e32 (another association, fused multiply-adds) + 4 float32 ulps.  Both terms
are RELATIVE TO THE ROW: the 48 values of one Gaussian share its packed gradients and its directions, so an element is held to
the largest magnitude of its own row, never to the tensor's (a Gaussian with a small gradient is held to its own size), and a row
whose reference is all zero has to be all zero.
"""
import functools

import numpy as np

from mygauhuman_amd import sh_utils

ULP = 2.0 ** -23
SENTINEL_BITS = 0xA5A5A5A5   # the fill of every guard band and of every float of a block nobody should write (a negative normal)
P_LIST = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 258, 259, 260, 513, 1027)
VIEWS_LIST = (1, 2, 8)


def _basis(deg, dirs):
    """[..., 3] unit directions -> [..., 16] weights in the dtype of `dirs`: channel c of eval_sh on the 16 x 16 unit matrix."""
    dirs = np.asarray(dirs)
    sh = np.broadcast_to(np.eye(16, dtype=dirs.dtype), dirs.shape[:-1] + (16, 16))
    w = np.asarray(sh_utils.eval_sh(deg, sh, dirs), dtype=dirs.dtype)
    assert w.dtype == dirs.dtype and w.shape == dirs.shape[:-1] + (16,)
    return w + dirs.dtype.type(0)   # (-0 from a negative constant times a zero coefficient -> +0)


def basis64(deg, dirs):
    return _basis(deg, np.asarray(dirs, np.float64))


def _grad_from_views(dtype, P, deg, M, views, stride, means, means_off, cam_off, scale):
    n = (deg + 1) ** 2
    assert 0 <= deg <= 3 and n <= M <= 16
    views = np.asarray(views, np.float32).reshape(-1)
    n_views, rem = divmod(views.size, stride)
    assert rem == 0 and n_views >= 1 and cam_off + 3 <= stride and cam_off >= 3 * P
    out = np.zeros((P, M, 3), dtype)
    scale = dtype(scale)
    if scale == 0 or P == 0:
        return out
    acc = np.zeros((P, 16, 3), dtype)
    for v in range(n_views):
        blk = views[v * stride:(v + 1) * stride]
        g = blk[:3 * P].reshape(P, 3).astype(dtype)
        m = means if means is not None else blk[means_off:means_off + 3 * P]
        m = np.asarray(m, np.float32).reshape(P, 3).astype(dtype)
        cam = blk[cam_off:cam_off + 3].astype(dtype)
        live = (g != 0).any(axis=1)   # an all-zero packed triple: the view contributes nothing, whatever its direction is
        d = m[live] - cam
        length = np.sqrt(d[:, 0:1] * d[:, 0:1] + d[:, 1:2] * d[:, 1:2] + d[:, 2:3] * d[:, 2:3])
        w = _basis(deg, d / length)
        acc[live] += w[:, :, None] * g[live][:, None, :]
    out[:, :n] = acc[:, :n] * scale
    return out


def grad_from_views64(P, deg, M, views, stride, means, means_off, cam_off, scale):
    """[P, M, 3] float64: scale * sum_v w_k(normalise(mean_v(i) - cam_v)) * g_v[i, c].  views: n_views blocks of `stride` floats,
    [3P packed | ...] with the camera at cam_off; means: the shared [P, 3] positions, or None = the view's own at means_off.
    Bands >= (deg + 1)^2 are exactly 0, everything is exactly 0 for scale == 0 (whatever the blocks hold)."""
    return _grad_from_views(np.float64, P, deg, M, views, stride, means, means_off, cam_off, scale)


def grad_from_views32(P, deg, M, views, stride, means, means_off, cam_off, scale):
    return _grad_from_views(np.float32, P, deg, M, views, stride, means, means_off, cam_off, scale)


def pack_posed_ref(colors, g, means, campos, block, means_off, cam_off):
    """The block after gsr_sh_view_pack_posed: packed = colour > 0 ? g : +0, the positions and the camera copied, every other
    float as it was."""
    out = np.array(block, np.float32, copy=True)
    n = np.asarray(colors).size
    c, g = np.asarray(colors, np.float32).reshape(-1), np.asarray(g, np.float32).reshape(-1)
    out[:n] = np.where(c > 0, g, np.float32(0.0))
    out[means_off:means_off + n] = np.asarray(means, np.float32).reshape(-1)
    out[cam_off:cam_off + 3] = np.asarray(campos, np.float32).reshape(3)
    return out


def step_finish_ref(flat, overflow_index, inv_world):
    """(bucket, scale, ranks) after gsr_step_finish: every element but the slot times scale = (slot > 0 ? 0 : inv_world)."""
    flat = np.asarray(flat, np.float32)
    slot = flat[overflow_index]
    scale = np.float32(0.0) if slot > 0 else np.float32(inv_world)
    out = flat * scale
    assert out.dtype == np.float32
    out[overflow_index] = slot
    return out, scale, int(np.uint32(np.float32(slot + np.float32(0.5))))


def step_status_ref(phase, status, slot, inv_world):
    """(slot, scale or None, report or None) after gsr_step_status."""
    if phase in (0, 2):
        slot = np.float32(1.0 if status[1] else 0.0)
    if phase == 0:
        return slot, None, None
    scale = np.float32(0.0) if slot > 0 else np.float32(inv_world)
    return np.float32(slot), scale, [int(np.uint32(np.float32(slot) + np.float32(0.5))), int(status[0]), int(status[1])]


# ------------------------------------------------------------------------------------------------------ the bound
def row_scale(want64):
    """[P, 1, 1]: the largest magnitude of every Gaussian's row."""
    return np.abs(want64).reshape(want64.shape[0], -1).max(axis=1).reshape(-1, 1, 1)


def twin_error(twin32, want64):
    """e32: the float32 twin's worst |error| / (largest magnitude of the row), over the rows that are not all zero."""
    rs = row_scale(want64)
    err = np.abs(np.asarray(twin32, np.float64) - want64)
    assert not err[np.broadcast_to(rs == 0, err.shape)].any(), "the twin is non-zero in a row the float64 reference has all zero"
    return float((err / np.where(rs > 0, rs, 1.0)).max()) if err.size else 0.0


def bound_for(want64, e32):
    """Elementwise bound [P, 1, 1] of the measured rule: (2 e32 + 4 ulp) x the row's largest magnitude."""
    return (2.0 * e32 + 4.0 * ULP) * row_scale(want64)


def check_measured(name, got, want64, twin32, shares=None):
    """Asserts |got - want64| <= bound elementwise, nothing excluded; prints the figures first and returns the share of the bound
    the worst element used (recorded in `shares` under `name` if given)."""
    got = np.asarray(got, np.float64)
    assert got.shape == want64.shape, (name, got.shape, want64.shape)
    assert np.isfinite(got).all(), f"{name}: {np.count_nonzero(~np.isfinite(got))} non-finite values, first row {np.argwhere(~np.isfinite(got))[0][0]}"
    e32 = twin_error(twin32, want64)
    bound = np.broadcast_to(bound_for(want64, e32), want64.shape)
    err = np.abs(got - want64)
    dead = bound == 0
    assert not err[dead].any(), f"{name}: non-zero values in rows whose reference is all zero"
    share = float((err[~dead] / bound[~dead]).max()) if (~dead).any() else 0.0
    ek = float((err / np.where(row_scale(want64) > 0, row_scale(want64), 1.0)).max()) if err.size else 0.0
    print(f"{name}: float32 twin {e32:.3e}  kernel {ek:.3e}  bound {2 * e32 + 4 * ULP:.3e}  share of the bound {share:.3f}")
    if shares is not None:
        shares[name] = max(shares.get(name, 0.0), share)
    worst = np.unravel_index(np.argmax(np.where(dead, 0.0, err / np.where(dead, 1.0, bound))), err.shape)
    assert share <= 1.0, f"{name}: element {worst} got {got[worst]!r} want {want64[worst]!r}: {share:.2f} x the bound (2 x {e32:.3e} + 4 ulp of the row)"
    return share


# ------------------------------------------------------------------------------------------------------ seeded inputs
@functools.lru_cache(maxsize=None)
def make_inputs(P, n_views, seed=0):
    """float32: g [V, P, 3] packed gradients ~ N(0, 1) with ~30 % of the entries exactly 0 (clamped channels) and ~10 % of the
    rows all zero (invisible in that view); shared positions [P, 3] ~ N(0, 1); per-view positions [V, P, 3] (the shared ones
    moved by N(0, 0.3): every view poses the Gaussians differently); cameras [V, 3] 3 to 5 units from the origin.  Read-only."""
    rng = np.random.default_rng(100003 * P + 101 * n_views + seed)
    g = rng.normal(0, 1, (n_views, P, 3)).astype(np.float32)
    g[rng.uniform(0, 1, g.shape) < 0.3] = 0.0
    g[rng.uniform(0, 1, (n_views, P)) < 0.1] = 0.0
    means = rng.normal(0, 1, (P, 3)).astype(np.float32)
    posed = (means[None] + rng.normal(0, 0.3, (n_views, P, 3))).astype(np.float32)
    d = rng.normal(0, 1, (n_views, 3))
    cams = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3, 5, (n_views, 1))).astype(np.float32)
    for a in (g, means, posed, cams):
        a.setflags(write=False)
    return g, means, posed, cams


def static_layout(P, stride_kind):
    """(stride, means_off, cam_off) of a static block [3P packed | campos | padding]: "padded" = CompactShExchange's stride (a
    multiple of 64 floats), "tight" = 3P + 3, the smallest the ABI accepts -- two floats more where that is itself a multiple of
    64 (P = 63, 255), so that "tight" is never one."""
    used = 3 * P + 3
    if stride_kind == "padded":
        return (used + 63) // 64 * 64, 0, 3 * P
    return (used + 2 if used % 64 == 0 else used), 0, 3 * P


def posed_layout(P, kind):
    """(stride, means_off, cam_off): "compact" = CompactShExchange(posed=True): [3P | 3P positions | campos 3, one pad | P radii],
    padded to 64 floats; "gap" = other legal offsets: 5 floats between the packed part and the positions, 7 between the
    positions and the camera, a stride that is no multiple of 4."""
    if kind == "compact":
        return (6 * P + 4 + P + 63) // 64 * 64, 3 * P, 6 * P
    return 6 * P + 5 + 7 + 3 + 6, 3 * P + 5, 6 * P + 12


def sentinel(n):
    return np.full(n, SENTINEL_BITS, np.uint32).view(np.float32)


def build_views(g, means_per_view, cams, stride, means_off, cam_off, fill=None):
    """[V * stride] float32 blocks; floats that belong to no part hold `fill` (default NaN: a kernel that reads one shows it)."""
    V, P = g.shape[0], g.shape[1]
    views = np.full((V, stride), np.nan if fill is None else fill, np.float32)
    views[:, :3 * P] = g.reshape(V, -1)
    if means_per_view is not None:
        views[:, means_off:means_off + 3 * P] = np.asarray(means_per_view, np.float32).reshape(V, -1)
    views[:, cam_off:cam_off + 3] = cams
    return views.reshape(-1)


@functools.lru_cache(maxsize=None)
def reference(P, deg, n_views, posed, scale=None):
    """(want64, twin32) [P, 16, 3] of the seeded case; scale: float32(1 / n_views) unless given -- the EXACT product of the
    kernel's float32 factors scale_h and dev_scale[0] (the twin rounds it to float32, as the kernel's one multiply does); posed:
    per-view positions.  Shared by the tests, read-only."""
    g, means, per_view, cams = make_inputs(P, n_views)
    scale = float(np.float32(1.0 / n_views)) if scale is None else float(scale)
    if posed:
        stride, mo, co = posed_layout(P, "compact")
        args = (P, deg, 16, build_views(g, per_view, cams, stride, mo, co), stride, None, mo, co, scale)
    else:
        stride, mo, co = static_layout(P, "tight")
        args = (P, deg, 16, build_views(g, None, cams, stride, mo, co), stride, means, mo, co, scale)
    want, twin = grad_from_views64(*args), grad_from_views32(*args)
    want.setflags(write=False)
    twin.setflags(write=False)
    return want, twin
