"""CPU-only tests of the PBR-phase loss (mygauhuman_amd.pbr.loss): the float64 restatement (tests/pbr_loss_reference.py) is pinned
to the fixture the reference's own train.py / utils/loss_utils.py made (tests/golden/make_golden_pbr_loss.py), every term's value
and gradient at 1e-9; the reference's NaN gradient of a constant entropy column is shown next to the restatement's zero; the
library exports the new entry points and validates their arguments without a GPU; CPU tensors raise."""
import os

import numpy as np
import pytest
import torch

from tests import pbr_loss_reference as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbr_loss.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def _close(name, got, want, rtol=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, name
    scale = max(float(np.abs(want).max()) if want.size else 0.0, 1e-300)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= rtol * scale, f"{name}: max error {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_matches_reference_fixture(fx, case):
    vals, grads = R.terms_and_grads(R.case_inputs(case))
    for name, v in vals.items():
        want = float(fx[f"{case}/{name}"])
        if np.isnan(want):
            assert np.isnan(v), f"{case}/{name}"
        else:
            assert abs(v - want) <= 1e-9 * max(abs(want), 1e-30), f"{case}/{name}: {v} vs {want}"
        for inp, g in grads[name].items():
            key = f"{case}/{name}/d_{inp}"
            want_g = fx[key] if key in fx else np.zeros_like(g)
            nan = np.isnan(want_g)
            if nan.any():  # only the entropy of a constant column: the reference's 0 * inf (checked below)
                assert name.startswith("entropy") and case == "edges", key
                assert np.all(g[nan] == 0), key
            _close(key, g[~nan], want_g[~nan])


def test_constant_column_nan_in_the_reference_zero_in_the_restatement(fx):
    """Rule (a): albedo's column 0 and roughness's column 2 are constant (sigma = 0) in the "edges" case.  The reference's autograd
    gives NaN on every pixel of such a column (its neighbours take their branch); the restatement, like the fused path, gives 0."""
    _, grads = R.terms_and_grads(R.case_inputs("edges"))
    ref_a, ref_r = fx["edges/entropy_albedo/d_albedo"], fx["edges/entropy_roughness/d_roughness"]
    assert np.isnan(ref_a[:, :, 0]).all() and not np.isnan(ref_a[:, :, 1:]).any()
    assert np.isnan(ref_r[:, :, 2]).all() and not np.isnan(ref_r[:, :, :2]).any()
    ours_a, ours_r = grads["entropy_albedo"]["albedo"], grads["entropy_roughness"]["roughness"]
    assert (ours_a[:, :, 0] == 0).all() and (ours_r[:, :, 2] == 0).all()
    assert np.abs(ours_a[:, :, 1:3]).max() > 0  # the other columns keep their gradient
    assert (ours_a[:, :, 3:] == 0).all()  # only columns 0..2 enter


def test_empty_masks_give_nan_values_and_zero_gradients(fx):
    vals, grads = R.terms_and_grads(R.case_inputs("empty_bound"))
    assert np.isnan(vals["l1"]) and np.isnan(fx["empty_bound/l1"]) and (grads["l1"]["rgb"] == 0).all()
    vals, grads = R.terms_and_grads(R.case_inputs("zero_alpha"))
    assert np.isnan(vals["prior"]) and np.isnan(fx["zero_alpha/prior"]) and (grads["prior"]["roughness"] == 0).all()
    assert vals["tv"] == 0.0 and (grads["tv"]["alpha"] == 0).all()


def test_reference_raises_below_three_columns(fx):
    assert int(fx["w_lt_3_raises"]) == 1
    with pytest.raises(ValueError):
        R.entropy(torch.rand(3, 4, 2, dtype=torch.float64))


def test_library_validates_the_pbr_loss_struct_without_a_gpu():
    import ctypes as C

    from mygauhuman_amd import _lib
    assert _lib.lib.gsr_pbr_loss_workspace_floats() > 1024 * 8
    s = _lib.PbrLoss()
    assert _lib.lib.gsr_pbr_loss_forward(C.byref(s), None, None) == -1
    s.width, s.height = 2, 8
    s.ca, s.a, s.entropy[0], s.bins = 1, 16, 1, 15
    s.loss, s.terms = 16, 16
    assert _lib.lib.gsr_pbr_loss_forward(C.byref(s), 16, None) == -1
    assert b"width >= 3" in _lib.lib.gsr_last_error()
    s.width, s.bins = 4, 33
    assert _lib.lib.gsr_pbr_loss_forward(C.byref(s), 16, None) == -1
    s.bins, s.tv = 15, 1
    assert _lib.lib.gsr_pbr_loss_forward(C.byref(s), 16, None) == -1 and b"mask" in _lib.lib.gsr_last_error()
    s.tv, s.g[0], s.gc[0], s.P = 0, 16, 3, 10
    assert _lib.lib.gsr_pbr_loss_forward(C.byref(s), 16, None) == -1 and b"k1" in _lib.lib.gsr_last_error()
    s.k1 = s.k2 = 16
    s.d_g[0] = 16
    assert _lib.lib.gsr_pbr_loss_backward(C.byref(s), 16, None) == -1 and b"inverse" in _lib.lib.gsr_last_error()


def test_cpu_tensors_raise():
    from mygauhuman_amd.pbr import MaterialSmoothness, PbrPhaseLoss, gaussian_entropy, get_masked_tv_loss
    x = torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        get_masked_tv_loss(torch.rand(1, 8, 8), x)
    with pytest.raises(RuntimeError, match="HIP device"):
        gaussian_entropy(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        MaterialSmoothness(torch.zeros(4, 3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="HIP device"):
        PbrPhaseLoss(x, torch.ones(1, 8, 8))


def test_names_are_exported_by_the_package():
    import mygauhuman_amd.pbr as pbr
    for name in ("PbrPhaseLoss", "MaterialSmoothness", "gaussian_entropy", "get_masked_tv_loss"):
        assert name in pbr.__all__ and callable(getattr(pbr, name))
