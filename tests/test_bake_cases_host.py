"""CPU tests of the inputs of tests/test_gpu_bake_f64.py (tests/bake_cases.py): with the float64 reference alone they show that
every scene and direction set is what the GPU tests assume, so that no GPU test can pass by leaving everything out."""
import numpy as np
import pytest
import torch

from tests import bake_cases as bc

# conditions on the scenes, not measurements: a scene that breaks them is changed (another seed), not the limits
MAX_MARGIN_FRAC, MAX_FACE_MARGIN_FRAC = 0.05, 0.20
FACE = bc.N * bc.N


@pytest.mark.parametrize("name", list(bc.SCENES))
def test_fragile_share(name):
    """Measured: body 2.3 % overall, 13 % in the worst (cell, face); box 3.7 %, 14 %; lengths 0.9 %, 5.8 %; planted 0.7 %, 1.1 %."""
    r = bc.reference(name)
    per_face = r.margin.reshape(-1, 6, FACE).mean(2)
    print(name, "margin share", r.margin.mean(), "worst (cell, face)", per_face.max())
    assert r.margin.mean() <= MAX_MARGIN_FRAC
    assert per_face.max() <= MAX_FACE_MARGIN_FRAC


@pytest.mark.parametrize("name", ["body", "box"])
def test_coverage(name):
    s, r = bc.SCENES[name](), bc.reference(name)
    assert s.centres.shape == (5, 3) and sorted(set(s.cell.tolist())) == [0, 1, 2, 3, 4, 5]
    assert len(set(s.chosen)) == 5 and s.chosen[0] == 0 and s.chosen[-1] == s.grid_cells - 1
    solid = ~r.margin
    assert (r.terminated & solid).sum() >= 100
    assert (r.clamped & solid).sum() >= 10
    unreached = (r.n_contrib == 0) & solid
    assert unreached.sum() >= 100 and (r.vis[unreached] == 1.0).all()
    reached = (r.n_contrib > 0) & solid
    assert reached.sum() >= 1000 and (r.vis[reached] < 1.0).all()
    empty = [(i, f) for (i, f), d in r.faces.items() if not (d["radii"] > 0).any()]
    assert empty
    for i, f in empty:
        assert (r.vis[i, f * FACE:(f + 1) * FACE] == 1.0).all() and not r.margin[i, f * FACE:(f + 1) * FACE].any()


def test_lengths_tile_lists():
    s = bc.lengths()
    assert len(s.means) == sum(bc.LENGTHS) and (s.cell == 1).all() and s.centres.shape == (2, 3)
    count = np.zeros(24, np.int64)
    tiles_of = np.zeros(len(s.means), np.int64)
    for f, (alive, x0, y0, x1, y1) in enumerate(bc.reference_rects(s.means, s.scales, s.rots, s.opac, s.centres[0])):
        for ty in range(2):
            for tx in range(2):
                inside = alive & (x0 <= tx) & (tx < x1) & (y0 <= ty) & (ty < y1)
                count[f * 4 + ty * 2 + tx] = inside.sum()
                tiles_of += inside
                assert (s.tile[inside] == f * 4 + ty * 2 + tx).all()
    assert count.tolist() == bc.LENGTHS
    assert (tiles_of == 1).all()
    # every centre lies inside its tile with an alpha above the cut-off there, so the tight cull keeps every instance
    assert s.opac.min() > 1.5 / 255.0
    r = bc.reference("lengths")
    assert (r.vis[1] == 1.0).all() and not r.margin[1].any()
    assert not r.terminated.any()  # the long lists are walked to their end
    assert r.n_contrib.max() > 128


def _solo_alpha(s, i, f):
    """The alpha image of face f with Gaussian i alone."""
    keep = np.zeros(len(s.means), bool)
    keep[i] = True
    r = bc.reference_visibility(s.means, s.scales, s.rots, s.opac, np.where(keep, 1, 0), s.centres, [0])
    return 1.0 - r.vis[0, f * FACE:(f + 1) * FACE].reshape(bc.N, bc.N)


def test_planted_decisions():
    s, r = bc.planted(), bc.reference("planted")
    rects = bc.reference_rects(s.means, s.scales, s.rots, s.opac, s.centres[0])
    assert s.centres.shape == (1, 3) and (s.cell == 1).all()
    for f in range(6):
        d = r.faces[(0, f)]
        assert np.array_equal(d["ids"], np.arange(len(s.means)))
        mine = lambda role: [int(i) for i in s.roles[role] if s.face_of[i] == f]  # noqa: E731
        (i,) = mine("near_culled")
        assert abs(d["z"][i] - 0.2 * 0.99) < 1e-6 and d["radii"][i] == 0
        (i,) = mine("near_kept")
        assert abs(d["z"][i] - 0.2 * 1.01) < 1e-6 and d["radii"][i] > 0 and _solo_alpha(s, i, f).max() > 0.5
        for i in mine("behind"):
            assert d["z"][i] < 0 and d["radii"][i] == 0
        (i,) = mine("outside_reaching_in")
        assert 1.0 < abs(d["txtz"][i]) < d["limx"] and d["radii"][i] > 0 and _solo_alpha(s, i, f).max() > 0.1
        (i,) = mine("clamped_x")
        assert abs(d["txtz"][i]) > d["limx"] and abs(d["tytz"][i]) < 1 and d["radii"][i] > 0 and _solo_alpha(s, i, f).max() > 0.1
        (i,) = mine("clamped_y")
        assert abs(d["tytz"][i]) > d["limy"] and abs(d["txtz"][i]) < 1 and d["radii"][i] > 0 and _solo_alpha(s, i, f).max() > 0.1
        alive, x0, y0, x1, y1 = rects[f]
        for role in ("seam_four_tiles", "four_tiles"):
            (i,) = mine(role)
            assert alive[i] and (x0[i], y0[i], x1[i], y1[i]) == (0, 0, 2, 2)
        (i,) = mine("seam_two_tiles")
        assert alive[i] and (x0[i], y0[i], x1[i], y1[i]) == (0, 0, 2, 1)
        a = _solo_alpha(s, mine("seam_four_tiles")[0], f)
        assert min(a[15, 15], a[15, 16], a[16, 15], a[16, 16]) > 0.1
        lo, hi = mine("corner")
        assert _solo_alpha(s, lo, f)[0, 0] > 0.1 and _solo_alpha(s, hi, f)[31, 31] > 0.1
        term = r.terminated[0, f * FACE:(f + 1) * FACE].reshape(bc.N, bc.N)
        assert term[19:29, 3:11].sum() >= 20 and not term[:, 16:].any()


def test_direction_sets():
    from mygauhuman_amd import baking
    full = bc.full_cube_dirs()
    assert full.shape == (bc.TEXELS, 3) and full.dtype == torch.float32
    np.testing.assert_array_equal(baking.cube_nearest_texel(full).numpy(), np.arange(bc.TEXELS))
    for name, make in bc.DIRECTION_SETS.items():
        dirs, texel = make()
        assert dirs.dtype == torch.float32 and dirs.shape == (len(texel), 3) and 1 <= len(texel) <= bc.TEXELS
        np.testing.assert_array_equal(baking.cube_nearest_texel(dirs).numpy(), texel, err_msg=name)
    # the plan: each (face, tile) needs the planned number of distinct pixels, every count of PLAN_COUNTS is there
    dirs, texel = bc.dirs_plan()
    counts = bc.plan_counts()
    assert set(bc.PLAN_COUNTS) <= set(counts) and len(counts) == 24
    assert len(np.unique(texel)) == len(texel) == sum(counts)
    assert np.bincount(bc.tile_of_texel(texel), minlength=24).tolist() == list(counts)
    assert (np.diff(texel) < 0).any()  # shuffled
    dirs, texel = bc.dirs_single()
    assert len(texel) == 1
    dirs, texel = bc.dirs_repeated()
    assert len(texel) == 513 and len(np.unique(texel)) <= 200
    dirs, texel = bc.dirs_production_and_invalid()
    assert len(texel) == 514 and texel[100] == -1 and texel[-1] == -1 and (np.delete(texel, [100, 513]) >= 0).all()
    assert not dirs[100].any() and torch.isnan(dirs[-1]).any()
    # what the production directions cover of a cube
    prod = np.delete(texel, [100, 513])
    assert len(np.unique(prod)) == 441
    assert np.bincount(bc.tile_of_texel(np.unique(prod)), minlength=24).max() == 27
