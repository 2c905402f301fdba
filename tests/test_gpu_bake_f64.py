"""The occlusion bake (csrc/bake.hip behind mygauhuman_amd.baking) against the float64 restatement of the reference rasterizer aimed at
the cube (tests/bake_cases.py; its inputs are proven on the CPU in tests/test_bake_cases_host.py): whole cube faces, so that all
four pixel slots of every lane of the blend are used; tile lists of pinned lengths around the 64-entry walk batches and the three
sort back-ends; direction subsets against the full cube bit for bit, with the rule for a direction without a texel; expand and
the per-frame reduction at their block tails."""
import numpy as np
import pytest
import torch

from tests import bake_cases as bc
from tests import util

pytestmark = pytest.mark.gpu

F32 = np.float32
FACE = bc.N * bc.N
GUARD, SENTINEL = 4096, -1234.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bake(s, dirs):
    from mygauhuman_amd import baking
    vis = baking.bake_visibility(_dev(s.means), _dev(s.scales), _dev(s.rots), _dev(s.opac), _dev(s.cell), _dev(s.centres), dirs.cuda())
    return vis.cpu().numpy()


def _against_float64(name, got, r):
    """`got` [K, 6144] of full_cube_dirs() against the reference `r`, outside its margin mask: the tolerance of the rasterizer's own
    float64 comparison of this blend (tests/test_gpu_cameras.py)."""
    assert got.shape == r.vis.shape and got.dtype == F32
    assert np.isfinite(got).all()
    keep = ~r.margin
    print(f"{name}: max |vis - float64| outside the margin mask {np.abs(got - r.vis)[keep].max():.3e} "
          f"({keep.mean():.4f} of the texels compared)")
    util.assert_close(name + " vis vs float64", got, r.vis, tol=1e-4, mask=keep, max_bad_frac=1e-4)
    unreached = (r.n_contrib == 0) & keep
    assert (got[unreached] == 1.0).all(), f"{name}: {(got[unreached] != 1.0).sum()} texels that nothing reaches are not 1.0f"
    for (i, f), d in r.faces.items():
        if not (d["radii"] > 0).any():
            assert (got[i, f * FACE:(f + 1) * FACE] == 1.0).all(), f"{name}: cell {i} face {f} sees nothing and is not all ones"


# ---- 1. whole cubes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["body", "box", "planted"])
def test_whole_cube_against_float64(name):
    """Every tile needs 256 pixels: all four pixel slots of every lane of the blend.  Measured on an MI355X (the printed maximum):
    body 1.0e-6, box 3.1e-6, planted 4.2e-7 (and 5.4e-7 for the scene of test_pinned_list_lengths)."""
    _against_float64(name, _bake(bc.SCENES[name](), bc.full_cube_dirs()), bc.reference(name))


# ---- 2. list lengths ---------------------------------------------------------------------------------------------------------
def test_pinned_list_lengths():
    from mygauhuman_amd import _lib, baking
    s, r = bc.lengths(), bc.reference("lengths")
    got = _bake(s, bc.full_cube_dirs())
    # the tight cull keeps an instance whose centre is inside its tile; the host test showed one tile per Gaussian
    assert baking.LAST_STATS["instances"] == sum(bc.LENGTHS)
    assert baking.LAST_STATS["batches"] == 1
    _against_float64("lengths", got, r)
    assert (got[1] == 1.0).all()
    _lib.set_tuning("bake_batch_cells", 1)
    try:
        again = _bake(s, bc.full_cube_dirs())
        assert baking.LAST_STATS["batches"] == 2 and baking.LAST_STATS["instances"] == sum(bc.LENGTHS)
    finally:
        _lib.set_tuning("bake_batch_cells", 0)
    np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))


# ---- 3. direction subsets ----------------------------------------------------------------------------------------------------
def test_direction_subsets_give_the_full_cube_bits():
    """A pixel's arithmetic does not depend on which other pixels are needed, and neither the tile lists nor their order depend
    on the direction set: bit-identical.  Rule: a direction without a texel (zero or non-finite) is NaN in every row."""
    s = bc.box_three_cells()
    full = _bake(s, bc.full_cube_dirs())
    assert np.isfinite(full).all() and (full < 1.0).any() and (full == 1.0).any()
    # the cells are baked independently: the same rows as in the five-cell bake
    np.testing.assert_array_equal(full.view(np.uint32), _bake(bc.box(), bc.full_cube_dirs())[:3].view(np.uint32))
    for name, make in bc.DIRECTION_SETS.items():
        dirs, texel = make()
        got = _bake(s, dirs)
        valid = texel >= 0
        assert got.shape == (3, len(texel))
        np.testing.assert_array_equal(got[:, valid].view(np.uint32), full[:, texel[valid]].view(np.uint32), err_msg=name)
        assert np.isnan(got[:, ~valid]).all(), name
        if not valid.all():  # the invalid directions change no other column
            alone = _bake(s, dirs[torch.from_numpy(valid)])
            np.testing.assert_array_equal(got[:, valid].view(np.uint32), alone.view(np.uint32), err_msg=name)


# ---- 4. expand and the per-frame reduction at their tails -------------------------------------------------------------------
def _guarded(n):
    return torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")


def _bands_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("P", [1, 3, 257])
@pytest.mark.parametrize("ndir", [1, 512, 513])
def test_expand_bits_at_the_tails(P, ndir):
    """occ = ((d0 n0 + d1 n1) + d2 n2 > 0) * vis[cell]: exact IEEE arithmetic in the order the kernel documents, so the numpy float32
    expression gives the same bits (a NaN vis gives the default NaN either way)."""
    from mygauhuman_amd import _lib, baking
    rng = np.random.default_rng(1000 * P + ndir)
    cells = 3
    d = rng.normal(0, 1, (ndir, 3)).astype(F32)
    n = rng.normal(0, 1, (P, 3)).astype(F32)
    # exactly orthogonal pairs: the first and last normal against an axis (0 + 0 + 0) and against 0.5 * 0.25 - 0.25 * 0.5
    n[0] = n[-1] = (0.5, 0.25, 0)
    d[0], d[-1] = (0, 0, 1), (0.25, -0.5, 0)
    vis = rng.normal(0.5, 0.6, (cells, ndir)).astype(F32)
    vis[:, ndir // 2] = np.nan
    cell = rng.integers(0, cells, P).astype(np.int32)
    cell[0] = cells - 1
    dot = (d[None, :, 0] * n[:, None, 0] + d[None, :, 1] * n[:, None, 1]) + d[None, :, 2] * n[:, None, 2]
    assert dot.dtype == F32 and dot[0, 0] == 0 and dot[0, -1] == 0 and dot[-1, -1] == 0
    want = (dot > 0).astype(F32) * vis[cell]
    got = baking.expand(_dev(cell), _dev(n), _dev(d), _dev(vis), H=1, W=ndir)
    assert got.shape == (P, 1, ndir, 1)
    got = got.cpu().numpy().reshape(P, ndir)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    buf = _guarded(P * ndir)
    t = [_dev(cell), _dev(n), _dev(d), _dev(vis)]
    _lib.check(_lib.lib.gsr_bake_expand(P, ndir, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                        buf[GUARD:].data_ptr(), None), "expand")
    torch.cuda.synchronize()
    assert _bands_intact(buf, P * ndir)
    np.testing.assert_array_equal(buf[GUARD:GUARD + P * ndir].cpu().numpy().view(np.uint32), want.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 1023])
def test_env_reduction_at_the_workgroup_tail(P):
    """Four Gaussians per workgroup: P around that tail, against a float64 sum at the tolerance of the 200k test."""
    from mygauhuman_amd import _lib, baking
    rng = np.random.default_rng(P)
    occ = rng.normal(0.5, 0.7, (P, 512)).astype(F32)
    for k, v in enumerate((0.0, 1.0, -0.3, 1.6)):  # exactly 0 and 1, below 0, above 1
        occ[:, k::7] = v
    assert (occ < 0).any() and (occ > 1).any() and (occ == 0).any() and (occ == 1).any()
    env = rng.uniform(0, 0.004, 512).astype(F32)

    def want_of(e):
        return np.repeat(np.clip((np.clip(occ.astype(np.float64), 0, 1) * e.astype(np.float64)).sum(1), 0, 1)[:, None], 3, 1)

    want = want_of(env)
    assert 0.1 < want.min() and want.max() < 0.9  # neither outer clamp is active
    got = baking.env_occlusion(_dev(occ).reshape(P, 16, 32, 1), _dev(env).reshape(1, 16, 32))
    assert got.shape == (P, 3)
    util.assert_close("env occlusion", got.cpu().numpy(), want, tol=1e-5)
    # the outer clamp, both ends: exactly 1 and exactly 0
    assert (baking.env_occlusion(_dev(occ).reshape(P, 16, 32, 1), _dev(env * 100).reshape(1, 16, 32)) == 1.0).all()
    assert (baking.env_occlusion(_dev(occ).reshape(P, 16, 32, 1), _dev(-env).reshape(1, 16, 32)) == 0.0).all()
    buf = _guarded(P * 3)
    o, e = _dev(occ), _dev(env)
    _lib.check(_lib.lib.gsr_bake_env_reduce(P, o.data_ptr(), e.data_ptr(), buf[GUARD:].data_ptr(), None), "env_reduce")
    torch.cuda.synchronize()
    assert _bands_intact(buf, P * 3)
    assert torch.equal(buf[GUARD:GUARD + P * 3].reshape(P, 3), got)
