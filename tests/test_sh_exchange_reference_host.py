"""Pins tests/sh_exchange_reference.py, the float64 / bit-exact CPU references the GPU tests of csrc/sh_exchange.hip are held to,
without a GPU: the basis against autograd's Jacobian of eval_sh, the rank-one structure of one view, the two position layouts
against each other, the bookkeeping references on hand-made buckets, and that the float32 twin the bound is sized by really
measures an error."""
import numpy as np
import pytest
import torch

from mygauhuman_amd import sh_utils
from tests import sh_exchange_reference as xr


def _unit_dirs(n, seed):
    d = np.random.default_rng(seed).normal(0, 1, (n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _jacobian(deg, dirs):
    """d eval_sh / d sh [N, 16] by autograd, float64 (eval_sh is linear in sh: one backward of the sum gives every row)."""
    sh = torch.zeros((dirs.shape[0], 1, 16), dtype=torch.float64, requires_grad=True)
    sh_utils.eval_sh(deg, sh, torch.from_numpy(dirs)).sum().backward()
    return sh.grad[:, 0].numpy()


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_basis_is_the_jacobian_of_eval_sh(deg):
    dirs = _unit_dirs(200, deg)
    w = xr.basis64(deg, dirs)
    assert w.dtype == np.float64 and w.shape == (200, 16)
    np.testing.assert_allclose(w, _jacobian(deg, dirs), rtol=0, atol=1e-15)
    n = (deg + 1) ** 2
    assert not w[:, n:].any() and not np.signbit(w[:, n:]).any()
    assert (np.abs(w[:, :n]).max(axis=0) > 0).all()


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_one_view_is_rank_one(deg):
    """grad_from_views64 with one view = the Jacobian at that view's directions, contracted with the packed gradient."""
    P = 37
    g, means, _, cams = xr.make_inputs(P, 1)
    stride, mo, co = xr.static_layout(P, "tight")
    views = xr.build_views(g, None, cams, stride, mo, co)
    got = xr.grad_from_views64(P, deg, 16, views, stride, means, mo, co, 0.75)
    d = means.astype(np.float64) - cams[0].astype(np.float64)
    jac = _jacobian(deg, d / np.linalg.norm(d, axis=1, keepdims=True))
    np.testing.assert_allclose(got, 0.75 * jac[:, :, None] * g[0].astype(np.float64)[:, None, :], rtol=0, atol=1e-15)
    assert not got[:, (deg + 1) ** 2:].any()
    assert (g[0] == 0).all(axis=1).any() and not got[(g[0] == 0).all(axis=1)].any()


def test_shared_positions_equal_the_same_positions_in_every_block():
    P, V, deg = 65, 3, 3
    g, means, _, cams = xr.make_inputs(P, V)
    s0, m0, c0 = xr.static_layout(P, "padded")
    a = xr.grad_from_views64(P, deg, 16, xr.build_views(g, None, cams, s0, m0, c0), s0, means, m0, c0, 1 / 3)
    for kind in ("compact", "gap"):
        s1, m1, c1 = xr.posed_layout(P, kind)
        views = xr.build_views(g, np.broadcast_to(means, (V, P, 3)), cams, s1, m1, c1)
        b = xr.grad_from_views64(P, deg, 16, views, s1, None, m1, c1, 1 / 3)
        assert np.array_equal(a, b), kind
    assert np.abs(a).max() > 0


def test_a_zero_scale_and_dead_views_give_exact_zeros():
    """scale == 0: zeros whatever the blocks hold; an all-zero packed triple: that view's direction (here 0 / 0 and NaN) is never
    formed."""
    P, V = 9, 2
    g, means, per_view, cams = (np.array(a) for a in xr.make_inputs(P, V))
    stride, mo, co = xr.posed_layout(P, "compact")
    nan_views = np.full(V * stride, np.nan, np.float32)
    z = xr.grad_from_views64(P, 3, 16, nan_views, stride, None, mo, co, 0.0)
    assert z.shape == (P, 16, 3) and not z.any() and np.isfinite(z).all()
    g[0, 2], g[1, 2] = 0.0, (1.0, -2.0, 0.5)
    g[0, 5], g[1, 5] = 0.0, (0.0, 0.0, 3.0)
    plain = xr.grad_from_views64(P, 3, 16, xr.build_views(g, per_view, cams, stride, mo, co), stride, None, mo, co, 0.5)
    per_view[0, 2] = cams[0]
    per_view[0, 5] = np.nan
    degen = xr.grad_from_views64(P, 3, 16, xr.build_views(g, per_view, cams, stride, mo, co), stride, None, mo, co, 0.5)
    assert np.isfinite(degen).all() and np.array_equal(plain, degen) and np.abs(degen[[2, 5]]).max() > 0


def test_pack_posed_ref_mask_rule():
    colors = np.array([[0.5, 0.0, -0.0], [1e-45, -1.0, 2.0]], np.float32)
    g = np.arange(1, 7, dtype=np.float32).reshape(2, 3)
    means = -np.arange(1, 7, dtype=np.float32).reshape(2, 3)
    block = xr.sentinel(24)
    out = xr.pack_posed_ref(colors, g, means, np.array([7, 8, 9], np.float32), block, 8, 16)
    assert out[:6].tolist() == [1.0, 0.0, 0.0, 4.0, 0.0, 6.0] and not np.signbit(out[:6]).any()
    assert out[8:14].tolist() == means.reshape(-1).tolist() and out[16:19].tolist() == [7.0, 8.0, 9.0]
    untouched = np.r_[6:8, 14:16, 19:24]
    assert (out.view(np.uint32)[untouched] == xr.SENTINEL_BITS).all() and (block.view(np.uint32) == xr.SENTINEL_BITS).all()


def test_step_finish_ref_keeps_the_slot_and_zeroes_a_failed_step():
    flat = np.array([1.5, -2.0, 3.0, 0.25, 8.0], np.float32)
    out, scale, ranks = xr.step_finish_ref(flat, 2, 0.5)            # slot 3 > 0: some rank overflowed
    assert scale == 0 and ranks == 3 and out[2] == 3.0 and not out[[0, 1, 3, 4]].any()
    flat[2] = 0.0
    out, scale, ranks = xr.step_finish_ref(flat, 2, 0.5)
    assert scale == np.float32(0.5) and ranks == 0 and out.tolist() == [0.75, -1.0, 0.0, 0.125, 4.0]
    assert out.dtype == np.float32 and flat.tolist() == [1.5, -2.0, 0.0, 0.25, 8.0]
    out, _, _ = xr.step_finish_ref(np.array([2.0], np.float32), 0, 0.125)
    assert out.tolist() == [2.0]


def test_step_status_ref_truth_table():
    assert xr.step_status_ref(0, (9, 7), np.float32(5.0), 0.5) == (1.0, None, None)
    assert xr.step_status_ref(0, (9, 0), np.float32(5.0), 0.5) == (0.0, None, None)
    assert xr.step_status_ref(1, (9, 1), np.float32(0.0), 0.5) == (0.0, 0.5, [0, 9, 1])
    assert xr.step_status_ref(1, (9, 0), np.float32(2.0), 0.5) == (2.0, 0.0, [2, 9, 0])
    assert xr.step_status_ref(2, (9, 7), np.float32(0.0), 0.25) == (1.0, 0.0, [1, 9, 7])
    assert xr.step_status_ref(2, (9, 0), np.float32(4.0), 0.25) == (0.0, 0.25, [0, 9, 0])


@pytest.mark.parametrize("P,deg,n_views", [(1, 0, 1), (4, 1, 2), (65, 2, 8), (257, 3, 8), (1027, 3, 2)])
@pytest.mark.parametrize("posed", [False, True], ids=["static", "posed"])
def test_the_float32_twin_measures_an_error(P, deg, n_views, posed):
    """The bound of the GPU tests is 2 x (this error) + 4 ulp: printed, and asserted only to be a finite non-zero number (so the
    recipe cannot silently collapse to the floor)."""
    want, twin = xr.reference(P, deg, n_views, posed)
    e32 = xr.twin_error(twin, want)
    print(f"P={P} deg={deg} views={n_views} {'posed' if posed else 'static'}: float32 twin {e32:.3e} = {e32 / xr.ULP:.2f} ulp of the row")
    assert twin.dtype == np.float32 and want.dtype == np.float64 and np.isfinite(e32)
    assert np.abs(want).max() > 0
    assert e32 > 0
    assert not want[:, (deg + 1) ** 2:].any() and not twin[:, (deg + 1) ** 2:].any()
