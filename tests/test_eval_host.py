"""CPU-only tests of the evaluation view finish (mygauhuman_amd.evaluate, csrc/eval.hip): the float64 numpy restatement of
tests/eval_reference.py reproduces the fixture the reference's own psnr() / ssim() made (tests/golden/make_golden_eval.py), so the
restatement the GPU tests lean on at other sizes is itself pinned to the reference; save_image's rounding rule; finish_view's refusals
raise before the library is touched; the two entry points are exported and validate their arguments without a device."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import eval_reference as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("case", list(R.CASES))
def test_numpy_restatement_reproduces_the_reference_fixture(fx, case):
    x = R.case_inputs(case)
    fin = R.finish_np(x["images"], x["mask"], x["background"])
    p, s = R.psnr_np(fin["render"], fin["gt"]), R.ssim_np(fin["render"], fin["gt"])
    want_p, want_s = float(fx[f"{case}/psnr_f64"]), float(fx[f"{case}/ssim_f64"])
    if math.isinf(want_p):
        assert p == want_p
    else:
        assert abs(p - want_p) <= 1e-9 * abs(want_p), (p, want_p)
    assert abs(s - want_s) <= 1e-9, (s, want_s)
    assert R.crc_of([R.quantise_np(fin[n]) for n in R.NAMES]) == int(fx[f"{case}/u8_crc"])


def test_fixture_covers_what_it_should(fx):
    assert math.isinf(float(fx["zeros_black_70x90_inf/psnr_f64"])) and float(fx["zeros_black_70x90_inf/psnr_f64"]) > 0
    x = R.case_inputs("inside_equal_256")  # render == gt inside: channel 1's mse is tiny
    fin = R.finish_np(x["images"], x["mask"], x["background"])
    assert 0.0 < float(((fin["render"][1].astype(np.float64) - fin["gt"][1]) ** 2).mean()) < 1e-6
    for case in R.CASES:  # the reference's own float32 error is the scale of the GPU tests' bound
        if not math.isinf(float(fx[f"{case}/psnr_f64"])):
            assert abs(float(fx[f"{case}/psnr_f32"]) - float(fx[f"{case}/psnr_f64"])) < 1e-4
        assert abs(float(fx[f"{case}/ssim_f32"]) - float(fx[f"{case}/ssim_f64"])) < 1e-5


def test_quantisation_rule_on_all_2_16_inputs():
    """uint8(min(max(x * 255 + 0.5, 0), 255)), truncating, two float32 roundings: numpy restatement against the torch chain."""
    x = (np.arange(65536, dtype=np.float64) / 65535 * 1.4 - 0.2).astype(np.float32).reshape(1, 256, 256)
    want = R.quantise_torch(torch.from_numpy(x.copy())).numpy()
    got = R.quantise_np(x)
    np.testing.assert_array_equal(got, want)
    assert got.min() == 0 and got.max() == 255 and len(np.unique(got)) == 256
    # the rule itself, spelled out in float32
    q = np.minimum(np.maximum(x * np.float32(255) + np.float32(0.5), np.float32(0)), np.float32(255))
    np.testing.assert_array_equal(got.reshape(-1), np.trunc(q).astype(np.uint8).reshape(-1))


def test_finish_view_refusals_raise_before_the_library():
    from mygauhuman_amd import evaluate
    x, m, bg = torch.rand(3, 8, 8), torch.ones(8, 8), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.finish_view({"render": x}, m, bg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.EvalMetrics(4, "cpu")
    with pytest.raises(ValueError):
        evaluate.finish_view({}, m, bg)
    table = object.__new__(evaluate.EvalMetrics)  # (never reached: the names are checked first)
    with pytest.raises(ValueError, match="metric = \\('render', 'gt'\\)"):
        evaluate.finish_view({"render": x}, m, bg, metrics=table)
    with pytest.raises(ValueError, match="metric"):
        evaluate.finish_view({"render": x, "gt": x}, m, bg, metrics=table, metric=("render_pbr", "gt"))
    assert len(evaluate.FILL_NAMES) == 11 and "gt" not in evaluate.FILL_NAMES and "gt_normal" not in evaluate.FILL_NAMES
    assert evaluate.FILL_NAMES == R.FILL_NAMES


def test_finish_view_shape_checks_name_the_tensor():
    """The checks that do not depend on where the tensor lives, exercised through the checker finish_view runs first."""
    from mygauhuman_amd import evaluate

    class FakeCuda(torch.Tensor):  # a CPU tensor that claims to be on the device: the shape checks come after the device check
        @property
        def is_cuda(self):
            return True

    def fake(t):
        return t.as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="'strided'.*not a dense permutation"):
        evaluate._check_image("strided", fake(torch.rand(3, 8, 16)[:, :, ::2]))
    with pytest.raises(ValueError, match="'two'.*2 channels"):
        evaluate._check_image("two", fake(torch.rand(2, 8, 8)))
    with pytest.raises(ValueError, match="'half'"):
        evaluate._check_image("half", fake(torch.rand(3, 8, 8).half()))
    evaluate._check_image("hwc", fake(torch.rand(8, 8, 3).permute(2, 0, 1)))
    evaluate._check_image("chw", fake(torch.rand(3, 8, 8)))
    evaluate._check_image("plane", fake(torch.rand(3, 8, 8)[0:1]))


def test_psnr_has_the_reference_signature_and_shape():
    from mygauhuman_amd import evaluate
    a, b = torch.rand(3, 5, 7), torch.rand(3, 5, 7)
    p = evaluate.psnr(a, b)
    assert tuple(p.shape) == (3, 1)
    torch.testing.assert_close(p, R.psnr_torch(a, b), rtol=0, atol=0)


def test_save_png_repeats_a_single_channel(tmp_path):
    from PIL import Image
    from mygauhuman_amd import evaluate
    rng = np.random.default_rng(0)
    a3, a1 = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (5, 7, 1), dtype=np.uint8)
    evaluate.save_png(str(tmp_path / "a3.png"), torch.from_numpy(a3))
    evaluate.save_png(str(tmp_path / "a1.png"), torch.from_numpy(a1))
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "a3.png")), a3)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "a1.png")), np.repeat(a1, 3, axis=2))
    with pytest.raises(ValueError):
        evaluate.save_png(str(tmp_path / "bad.png"), torch.zeros(5, 7, 2, dtype=torch.uint8))


def _valid_view(_lib):
    v = _lib.EvalView()
    v.slots, v.height, v.width = 2, 32, 48
    for k in range(2):
        v.slot[k].src, v.slot[k].channels = 16, 3
        v.slot[k].stride[:] = [32 * 48, 48, 1]
    v.slot[0].flags = _lib.EVAL_FILL
    v.mask, v.mask_dtype, v.background = 16, _lib.MASK_F32, 16
    v.metric_image, v.metric_gt = 0, 1
    v.counter = v.table = v.overflow = 16
    v.capacity = 4
    return v


def test_symbols_are_exported_and_validate_without_a_device():
    from mygauhuman_amd import _lib
    for name in ("gsr_eval_workspace_floats", "gsr_eval_view_finish"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name), name
    ws = _lib.lib.gsr_eval_workspace_floats
    # three doubles per workgroup of 256 threads x 4 pixels, one float per 16 x 16 tile and plane
    assert ws(1024, 1024) == 2 * 3 * 1024 + 3 * 64 * 64
    assert ws(70, 90) == 2 * 3 * 7 + 3 * 5 * 6
    assert ws(0, 8) == 0 and ws(8, -1) == 0 and ws(1 << 16, 1 << 15) == 0
    f, err = _lib.lib.gsr_eval_view_finish, _lib.lib.gsr_last_error
    assert f(None, 16, None) == -1 and b"null" in err()

    def bad(edit, word, workspace=16):
        v = _valid_view(_lib)
        edit(v)
        assert f(C.byref(v), workspace, None) == -1, word
        assert word in err(), (word, err())
    for n in (0, 17, -1):
        bad(lambda v, n=n: setattr(v, "slots", n), b"slots")
    bad(lambda v: setattr(v, "height", 0), b"positive")
    bad(lambda v: setattr(v, "width", -3), b"positive")

    def huge(v):
        v.height, v.width = 1 << 16, 1 << 15
    bad(huge, b"too large")
    bad(lambda v: setattr(v.slot[1], "src", None), b"src")
    for ch in (0, 2, 4):
        bad(lambda v, ch=ch: setattr(v.slot[0], "channels", ch), b"channels")
    bad(lambda v: setattr(v.slot[0], "flags", 8), b"flags")

    def flip_one(v):
        v.slot[0].channels, v.slot[0].flags = 1, _lib.EVAL_FLIP_Z
    bad(flip_one, b"FLIP_Z")

    def neg(v):
        v.slot[1].stride[1] = -48
    bad(neg, b"strides")
    bad(lambda v: setattr(v, "mask", None), b"mask")
    bad(lambda v: setattr(v, "background", None), b"background")
    bad(lambda v: setattr(v, "mask_dtype", 2), b"mask_dtype")
    bad(lambda v: setattr(v, "metric_gt", 0), b"metric pair")
    bad(lambda v: setattr(v, "metric_gt", 2), b"metric pair")
    bad(lambda v: setattr(v, "metric_image", -1), b"metric pair")
    bad(lambda v: setattr(v.slot[1], "channels", 1), b"3-channel")
    for field in ("counter", "table", "overflow"):
        bad(lambda v, field=field: setattr(v, field, None), b"required")
    bad(lambda v: setattr(v, "capacity", 0), b"capacity")
    bad(lambda v: None, b"workspace", workspace=None)
    bad(lambda v: None, b"aligned", workspace=20)
