"""CPU-only tests of the crop SSIM (loss_utils.bounding_rect / ssim_crop, csrc/ssim_crop.hip): the library exports the entry points
and validates their arguments without a device; CPU tensors raise; the numpy restatement of cv2.boundingRect reproduces the rects of
the fixture the reference's own ssim() made (tests/golden/make_golden_ssim_crop.py); and tests/torch_reference.ssim_torch on the
crop, in float64, reproduces the fixture's values and gradients -- the restatement the GPU tests also use is pinned to the
reference."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import ssim_crop_reference as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_crop.npz")
NEW_SYMBOLS = ("gsr_bounding_rect_workspace_ints", "gsr_bounding_rect", "gsr_ssim_crop_workspace_floats", "gsr_ssim_crop_forward",
               "gsr_ssim_crop_backward")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def test_symbols_are_exported_and_declared():
    from mygauhuman_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name), name
    assert _lib.lib.gsr_bounding_rect_workspace_ints() >= 4
    # one float per 16 x 16 tile and plane
    assert _lib.lib.gsr_ssim_crop_workspace_floats(6, 1024, 1024) == 6 * 64 * 64
    assert _lib.lib.gsr_ssim_crop_workspace_floats(3, 17, 33) == 3 * 2 * 3
    assert _lib.lib.gsr_ssim_crop_workspace_floats(0, 17, 33) == 0


def test_bounding_rect_validates_without_a_device():
    from mygauhuman_amd import _lib
    f = _lib.lib.gsr_bounding_rect
    assert f(0, 8, 16, _lib.MASK_F32, 16, 16, None) == -1 and b"positive" in _lib.lib.gsr_last_error()
    assert f(8, -1, 16, _lib.MASK_F32, 16, 16, None) == -1
    assert f(1 << 16, 1 << 15, 16, _lib.MASK_U8, 16, 16, None) == -1 and b"too large" in _lib.lib.gsr_last_error()
    for mask, rect, ws in ((None, 16, 16), (16, None, 16), (16, 16, None)):
        assert f(8, 8, mask, _lib.MASK_F32, rect, ws, None) == -1 and b"required" in _lib.lib.gsr_last_error()
    assert f(8, 8, 16, 2, 16, 16, None) == -1 and b"mask_dtype" in _lib.lib.gsr_last_error()


def _valid_spec(_lib):
    s = _lib.SsimCrop()
    s.groups, s.height, s.width, s.rect = 2, 32, 48, 16
    for g in range(2):
        s.planes[g] = 3
        s.img1[g] = s.img2[g] = s.value[g] = 16
        s.img1_stride[g][:] = [32 * 48, 48, 1]
    return s


def test_ssim_crop_validates_without_a_device():
    from mygauhuman_amd import _lib
    fwd, bwd, err = _lib.lib.gsr_ssim_crop_forward, _lib.lib.gsr_ssim_crop_backward, _lib.lib.gsr_last_error
    assert fwd(None, 16, None) == -1 and b"null" in err()
    assert bwd(None, None) == -1 and b"null" in err()
    s = _valid_spec(_lib)
    assert fwd(C.byref(s), None, None) == -1 and b"workspace" in err()
    for groups in (0, 5, -1):
        s = _valid_spec(_lib)
        s.groups = groups
        assert fwd(C.byref(s), 16, None) == -1 and b"groups" in err()
        assert bwd(C.byref(s), None) == -1 and b"groups" in err()
    for field in ("height", "width"):
        s = _valid_spec(_lib)
        setattr(s, field, 0)
        assert fwd(C.byref(s), 16, None) == -1 and b"positive" in err()
        assert bwd(C.byref(s), None) == -1 and b"positive" in err()
    s = _valid_spec(_lib)
    s.rect = None
    assert fwd(C.byref(s), 16, None) == -1 and b"rect" in err()
    assert bwd(C.byref(s), None) == -1 and b"rect" in err()
    s = _valid_spec(_lib)
    s.planes[1] = 0
    assert fwd(C.byref(s), 16, None) == -1 and b"planes" in err()
    s.planes[0], s.planes[1] = 65000, 536
    assert fwd(C.byref(s), 16, None) == -1 and b"65535" in err()
    assert bwd(C.byref(s), None) == -1 and b"65535" in err()
    for field in ("img1", "img2", "value"):
        s = _valid_spec(_lib)
        getattr(s, field)[1] = None
        assert fwd(C.byref(s), 16, None) == -1, field
    s = _valid_spec(_lib)
    s.dA[0] = 16  # the three maps come together
    assert fwd(C.byref(s), 16, None) == -1 and b"dA" in err()
    s = _valid_spec(_lib)
    s.d_img1[0] = 16  # a gradient needs the maps
    assert bwd(C.byref(s), None) == -1 and b"d_img1" in err()


def test_cpu_tensors_and_bad_arguments_raise():
    from mygauhuman_amd import loss_utils
    x, rect = torch.rand(3, 8, 8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss_utils.bounding_rect(torch.ones(8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss_utils.ssim_crop(x, x, rect)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss_utils.ssim_crop((x, x), (x, x), rect)
    with pytest.raises(ValueError):
        loss_utils.ssim_crop((x, x), x, rect)
    with pytest.raises(ValueError):
        loss_utils.ssim_crop((x,) * 5, (x,) * 5, rect)


def test_names_are_exported_next_to_the_pbr_loss():
    import mygauhuman_amd.pbr as pbr
    from mygauhuman_amd import loss_utils
    for name in ("bounding_rect", "ssim_crop"):
        assert name in pbr.__all__ and getattr(pbr, name) is getattr(loss_utils, name)


@pytest.mark.parametrize("case", list(R.CASES))
def test_bounding_rect_restatement_reproduces_the_fixture_rects(fx, case):
    rect = R.bounding_rect_np(R.case_inputs(case)["mask"])
    assert rect == tuple(int(v) for v in fx[f"{case}/rect"]) == R.CASES[case][4]


def test_bounding_rect_restatement_on_the_documented_corner_cases():
    assert R.bounding_rect_np(np.zeros((5, 7))) == (0, 0, 0, 0)
    m = np.zeros((5, 7), np.uint8)
    m[4, 6] = 1
    assert R.bounding_rect_np(m) == (6, 4, 1, 1)
    m[0, 0] = 3
    assert R.bounding_rect_np(m) == (0, 0, 7, 5)
    assert R.bounding_rect_np(np.array([[0, 0, 0], [0, 1, 1]], bool)) == (1, 1, 2, 1)


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_on_the_crop_matches_the_reference_fixture(fx, case):
    x = R.case_inputs(case)
    rx, ry, rw, rh = rect = tuple(int(v) for v in fx[f"{case}/rect"])
    for g in range(R.CASES[case][3]):
        v, grad = R.value_and_grad(x["img1"][g], x["img2"][g], rect)
        want_v, want_g = float(fx[f"{case}/{g}/value"]), fx[f"{case}/{g}/grad"]
        assert abs(v - want_v) <= 1e-9 * abs(want_v), f"{case}/{g}: {v} vs {want_v}"
        inside = grad[:, ry:ry + rh, rx:rx + rw]
        assert inside.shape == want_g.shape
        assert np.abs(inside - want_g).max() <= 1e-9 * np.abs(want_g).max(), f"{case}/{g}"
        outside = grad.copy()
        outside[:, ry:ry + rh, rx:rx + rw] = 0.0
        assert not outside.any()


def test_one_pixel_rect_is_a_real_value_with_a_gradient(fx):
    """A 1 x 1 crop is not a degenerate case: the window's centre tap alone gives a value strictly inside (0, 1)."""
    assert 0.0 < float(fx["one_pixel/0/value"]) < 1.0
    assert fx["one_pixel/0/grad"].shape == (3, 1, 1) and np.abs(fx["one_pixel/0/grad"]).min() > 0


def test_crop_equals_the_zeroed_full_frame_map_averaged_over_the_rect(fx):
    """The identity the kernels rest on (zero padding): SSIM of the crop = the full-frame SSIM map of the images zeroed outside the
    rect, averaged over the rect."""
    import torch.nn.functional as F

    from tests.torch_reference import _window_2d
    x = R.case_inputs("interior")
    rx, ry, rw, rh = (int(v) for v in fx["interior/rect"])
    keep = torch.zeros(x["img1"][0].shape[1:], dtype=torch.float64)
    keep[ry:ry + rh, rx:rx + rw] = 1.0
    a, b = (x["img1"][0] * keep)[None], (x["img2"][0] * keep)[None]
    win = _window_2d(11).to(torch.float64).expand(3, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t, win, padding=5, groups=3)  # noqa: E731
    m1, m2 = blur(a), blur(b)
    v1, v2, v12 = blur(a * a) - m1 * m1, blur(b * b) - m2 * m2, blur(a * b) - m1 * m2
    smap = ((2 * m1 * m2 + 1e-4) * (2 * v12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (v1 + v2 + 9e-4))
    got = float(smap[0, :, ry:ry + rh, rx:rx + rw].mean())
    assert abs(got - float(fx["interior/0/value"])) < 1e-12
