"""The reference side of the tests of an active SH degree below the stored one (tests/sh_degree_cases.py), without a GPU: the
CPU oracle against the float64 restatement at D < M with the inactive bands times 50, the coverage the scenes promise, the
inactive gradients, the NaN poison and the scale-modifier identity -- so that test_gpu_sh_degree.py cannot pass or fail
because of its yardstick.  Also HumanGaussianModel.oneupSHdegree()."""
import numpy as np
import pytest

from tests import raster_reference as rr
from tests import sh_degree_cases as sc
from tests import util
from tests.test_raster_reference_host import compare_to_float64, grad_names, rel_err, tolerance

CASES = [(name, M, D) for name in sc.SCENES for M, D in sc.LAYOUTS]
# what the issue's table states for the two scenes (measured with the float64 restatement and the oracle on the CPU)
VISIBLE = {"p600": 443, "p300": 258}
CLAMPED_P600_M16 = {0: 40, 1: 46, 2: 48}


@pytest.mark.parametrize("name,M,D", CASES)
def test_oracle_matches_float64_below_the_stored_degree(oracle, name, M, D):
    P = sc.SCENES[name][0]
    s = sc.reference(oracle, name, P, M, D)
    assert s.g["shs"].shape[1] == M and s.g["sh_degree"] == D and s.n_active < M
    # the inactive bands are fifty times what the scene was made with: reading one of them cannot hide inside a tolerance
    stored = sc.scene(name, P, M, sc.STORED_DEGREE[M])[1]["shs"]
    np.testing.assert_array_equal(s.g["shs"][:, :s.n_active], stored[:, :s.n_active])
    np.testing.assert_array_equal(s.g["shs"][:, s.n_active:], np.float32(50.0) * stored[:, s.n_active:])
    assert float(np.abs(s.g["shs"][:, s.n_active:]).min(axis=(1, 2)).max()) > 0
    np.testing.assert_array_equal(s.ref["pre"]["radii"], s.r64["radii"])
    assert int(s.visible.sum()) == VISIBLE[name]
    assert s.keep.mean() > 1 - sc.MAX_MARGIN_FRAC, s.keep.mean()
    n_clamped = int(s.ref["pre"]["clamped"][s.visible].sum())
    assert n_clamped > 0, "no clamped channel: the clamp mask of the SH backward is not exercised"
    if name == "p600" and M == 16:
        assert n_clamped == CLAMPED_P600_M16[D]
    errs = {}
    for k in ("color", "depth", "alpha"):
        errs[k] = compare_to_float64(k, s.ref["img"][k], s.r64[k], s.keep, tol=tolerance("identity", k))
    for n in grad_names("sh"):
        assert np.abs(s.want64[n]).max() > 0, n
        util.assert_close(n, s.want[n].reshape(s.want64[n].shape), s.want64[n], tol=tolerance("identity", n))
        errs[n] = rel_err(s.want[n], s.want64[n])
    print(f"{name} M={M} D={D} keep {s.keep.mean():.4f} clamped {n_clamped} worst " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    # inactive bands and culled rows: exactly zero on both sides
    sc.assert_inactive_zero("oracle", s.want["dL_dsh"], s.ref["pre"]["radii"], D)
    sc.assert_inactive_zero("float64", s.want64["dL_dsh"], s.r64["radii"], D)
    assert (s.ref["pre"]["radii"] == 0).sum() > 0
    # the active part is what the same scene gives when the inactive coefficients are not there at all
    assert float(np.abs(s.want["dL_dsh"][:, :s.n_active]).max()) > 0


@pytest.mark.parametrize("name,M,D", CASES)
def test_nan_in_the_inactive_bands_leaves_the_oracle_bit_identical(oracle, name, M, D):
    """The reference reads only the active bands: NaN (or zero) in the others changes no bit of any output."""
    P = sc.SCENES[name][0]
    s = sc.reference(oracle, name, P, M, D)
    for variant in (sc.poisoned(s.g), sc.zeroed(s.g)):
        ref = util.oracle_forward(oracle, s.cam, variant, sc.BG, "sh")
        for k in ("color", "depth", "alpha", "final_T", "n_contrib"):
            assert sc.bits_equal(ref["img"][k], s.ref["img"][k]), k
        for k in ("radii", "rgb", "clamped", "depths", "means2D", "conic_opacity", "tiles_touched"):
            assert sc.bits_equal(ref["pre"][k], s.ref["pre"][k]), k
        got = oracle.rasterize_backward(ref, *s.up)
        for n in grad_names("sh"):
            assert sc.bits_equal(got[n], s.want[n]), n


@pytest.mark.parametrize("name", list(sc.SCENES))
@pytest.mark.parametrize("m", sc.MODIFIERS + (2.0,))
def test_scale_modifier_identity_on_the_oracle_and_the_restatement(oracle, name, m):
    """The reference kernel's convention: the scale that enters is float32(m) * s and dL_dscales is taken with respect to THAT
    product (no factor of m).  So the rasterizer at modifier m with scales s equals the rasterizer at modifier 1 with scales
    float32(m) * s -- for the oracle in every bit, dL_dscales included; for the float64 restatement to the rounding of the float32
    product (2^-24 relative on the scales) -- and the oracle matches the restatement at modifier m."""
    P0 = sc.SCENES[name][0]
    cam, g = sc.scene(name, P0, 16, 3)
    s = sc.reference(oracle, name, P0, 16, 3, modifier=m)
    g1 = dict(g, scales=(np.float32(m) * g["scales"]).astype(np.float32))
    # ---- oracle: bit for bit
    ref1 = util.oracle_forward(oracle, cam, g1, sc.BG, "sh")
    for k in ("color", "depth", "alpha", "final_T", "n_contrib", "fragile"):
        assert sc.bits_equal(ref1["img"][k], s.ref["img"][k]), k
    for k in ("radii", "cov3D", "conic_opacity", "tiles_touched"):
        assert sc.bits_equal(ref1["pre"][k], s.ref["pre"][k]), k
    got1 = oracle.rasterize_backward(ref1, *s.up)
    for n in grad_names("sh"):
        assert sc.bits_equal(got1[n], s.want[n]), n
    assert float(np.abs(s.want["dL_dscales"]).max()) > 0
    # ---- the modifier changes the picture (the identity above is not vacuous)
    base = sc.reference(oracle, name, P0, 16, 3)
    assert float(np.abs(base.ref["img"]["color"] - s.ref["img"]["color"]).max()) > 1e-2
    # ---- restatement: the same identity to the rounding of the product, and the oracle against it at modifier m
    r1 = rr.forward(cam, g1, sc.BG, "sh")
    np.testing.assert_array_equal(r1["radii"], s.r64["radii"])
    both = ~r1["margin"] & ~s.r64["margin"]
    for k in ("color", "depth", "alpha"):
        compare_to_float64(k, s.r64[k], r1[k], both, tol=1e-5)
    w1 = rr.backward(cam, g1, sc.BG, "sh", *s.up)
    for n in grad_names("sh"):
        util.assert_close(n + " (restatement identity)", s.want64[n], w1[n], tol=1e-5)
    np.testing.assert_array_equal(s.ref["pre"]["radii"], s.r64["radii"])
    assert s.keep.mean() > 1 - sc.MAX_MARGIN_FRAC, s.keep.mean()
    for k in ("color", "depth", "alpha"):
        compare_to_float64(k, s.ref["img"][k], s.r64[k], s.keep, tol=tolerance("identity", k))
    for n in grad_names("sh"):
        util.assert_close(n, s.want[n].reshape(s.want64[n].shape), s.want64[n], tol=tolerance("identity", n))


@pytest.mark.parametrize("P", sc.TAILS)
def test_block_tail_scenes_are_cuts_of_the_full_scene(oracle, P):
    """The first P Gaussians of the 600-Gaussian scene: same camera, same rows; the restatement and the oracle still agree."""
    cam, g = sc.scene("p600", P, 16, 1)
    cam0, g0 = sc.scene("p600", 600, 16, 1)
    assert cam is not None and g["shs"].shape == (P, 16, 3) and g["sh_degree"] == 1
    for k in sc.PER_GAUSSIAN:
        np.testing.assert_array_equal(g[k], g0[k][:P])
    s = sc.reference(oracle, "p600", P, 16, 1)
    np.testing.assert_array_equal(s.ref["pre"]["radii"], s.r64["radii"])
    for n in grad_names("sh"):
        util.assert_close(n, s.want[n].reshape(s.want64[n].shape), s.want64[n], tol=tolerance("identity", n))
    sc.assert_inactive_zero("oracle", s.want["dL_dsh"], s.ref["pre"]["radii"], 1)


def test_oneup_sh_degree_stops_at_the_stored_degree():
    from mygauhuman_amd.scene_model import HumanGaussianModel
    m = HumanGaussianModel(3, device="cpu")
    assert m.active_sh_degree == m.max_sh_degree == 3
    m.active_sh_degree = 0
    seen = []
    for _ in range(5):
        m.oneupSHdegree()
        seen.append(m.active_sh_degree)
    assert seen == [1, 2, 3, 3, 3] and m.max_sh_degree == 3
    z = HumanGaussianModel(0, device="cpu")
    z.oneupSHdegree()
    assert z.active_sh_degree == 0
