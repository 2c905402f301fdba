"""CPU-only tests of the SMPL-X (55-joint) support: the host-side skinning formulation and the skinning-offset network at 55 bones
against vectors generated from the imported reference (tests/golden/make_golden_smplx.py), the joint-count entry points of the C ABI
(exported; unsupported joint counts refused before anything runs on a device) and the seeded SMPL-X-shaped synthetic body."""
import os

import numpy as np
import pytest
import torch

from mygauhuman_amd import human_synth, lbs, nets
from mygauhuman_amd._lib import lib

NJ = 55


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


def test_smplx_lbs_matches_reference_at_55_joints(golden_dir):
    g = _load(golden_dir, "lbs_smplx.npz")
    t = lambda k: torch.from_numpy(g[k].astype(np.float32))  # noqa: E731
    assert g["pose"].shape == (1, 3 * NJ) and g["betas"].shape == (1, 20) and g["smpl_posedirs"].shape == (9 * (NJ - 1), 900)
    verts, Jt, A, T = lbs.smplx_lbs(t("betas"), t("pose"), t("smpl_v_template"), t("smpl_shapedirs"), t("smpl_posedirs"),
                                    t("smpl_J_regressor"), torch.from_numpy(g["smpl_parents"]), t("smpl_weights"))
    assert A.shape == (1, NJ, 4, 4) and Jt.shape == (1, NJ, 3)
    for name, got in (("verts", verts), ("J_transformed", Jt), ("A", A), ("T", T)):
        assert _rel(got[0].numpy(), g[name]) < 1e-5, name
    rot = lbs.batch_rodrigues(t("pose").view(-1, 3))
    assert _rel(rot.numpy(), g["rot_mats"]) < 1e-6


def test_offset_decoder_55_bones_matches_reference(golden_dir):
    g = _load(golden_dir, "lbs_offset_decoder_55.npz")
    dec = nets.FusedLBSOffsetDecoder(total_bones=NJ)
    assert not dec.use_fused and dec.bw_fc.weight.shape == (NJ, 128, 1)
    dec.load_state_dict({k[len("param."):]: torch.from_numpy(g[k].astype(np.float32)) for k in g.files if k.startswith("param.")})
    pts, w = torch.from_numpy(g["pts"]), torch.from_numpy(g["w"])
    out = dec.forward_torch(pts)
    assert out.shape == (1, NJ, 256)
    assert _rel(out.detach().numpy(), g["out"]) < 1e-5
    (out * w).sum().backward()
    for name, p in dec.named_parameters():
        assert _rel(p.grad.numpy(), g["grad." + name]) < 1e-5, name
    # forward() at 55 bones is forward_torch (the fused kernels are built for 24 outputs): same values, also with use_fused set
    dec.use_fused = True
    with torch.no_grad():
        assert torch.equal(dec(pts), out.detach())


def test_offset_decoder_24_bones_unchanged():
    dec = nets.FusedLBSOffsetDecoder()
    assert dec.use_fused and dec.total_bones == 24 and dec.bw_fc.weight.shape == (24, 128, 1)
    with pytest.raises(ValueError):
        nets.FusedLBSOffsetDecoder(total_bones=0)


def test_joint_count_entry_points_exported_and_checked():
    names = ("gsr_lbs_forward_nj", "gsr_lbs_forward_grid_nj", "gsr_lbs_forward_cached_nj", "gsr_lbs_backward_nj",
             "gsr_body_pose_forward", "gsr_body_pose_backward")
    for n in names:
        assert hasattr(lib, n), n
    z = [None] * 19
    # LBS: J in {24, 55}; 30 is refused before anything else is looked at, with a message naming the supported counts
    rc = lib.gsr_lbs_forward_nj(30, 0, 1, *z, None)
    msg = lib.gsr_last_error()
    assert rc == -1 and b"30" in msg and b"24" in msg and b"55" in msg
    assert lib.gsr_lbs_forward_grid_nj(30, 0, 1, *z, None, 0, 0, None) == -1 and b"gsr_lbs_forward_grid_nj" in lib.gsr_last_error()
    assert lib.gsr_lbs_forward_cached_nj(30, 0, 1, *z, None, 0, None, 0, 0, None) == -1
    assert lib.gsr_lbs_backward_nj(30, 0, 1, *([None] * 20), None) == -1 and b"gsr_lbs_backward_nj" in lib.gsr_last_error()
    # P = 0 with a supported J: nothing to do, no device touched
    for J in (24, 55):
        assert lib.gsr_lbs_forward_nj(J, 0, 1, *z, None) == 0
        assert lib.gsr_lbs_backward_nj(J, 0, 1, *([None] * 20), None) == 0
    # pose chain: 2 <= J <= 64
    par = (lib.gsr_body_pose_forward.argtypes[4]._type_ * 65)(*([0] + list(range(64))))
    for J in (65, 1, 0):
        assert lib.gsr_body_pose_forward(J, None, None, None, par, None, None, None) == -1
        assert f"J = {J}".encode() in lib.gsr_last_error() and b"64" in lib.gsr_last_error()
        assert lib.gsr_body_pose_backward(J, None, None, None, par, None, None, None, None, None, None) == -1
    # a valid J gets as far as the argument checks
    assert lib.gsr_body_pose_forward(55, None, None, None, par, None, None, None) == -1
    assert b"null argument" in lib.gsr_last_error()
    # pose-blend GEMV: up to 512 columns
    assert lib.gsr_gemv_rows(0, 512, None, None, None, None) == 0
    assert lib.gsr_gemv_rows(0, 513, None, None, None, None) == -1 and b"512" in lib.gsr_last_error()


def test_synthetic_smplx_body():
    b = human_synth.body_arrays(body="smplx")
    V = 10475
    assert b["v_template"].shape == (V, 3) and b["weights"].shape == (V, NJ) and b["J_regressor"].shape == (NJ, V)
    assert b["shapedirs"].shape == (V, 3, 20) and b["posedirs"].shape == (V, 3, 486)
    np.testing.assert_allclose(b["weights"].sum(1), 1.0, rtol=1e-5)
    kt = human_synth.kintree_table("smplx")
    assert kt.shape == (2, NJ) and kt[0, 0] == -1
    assert all(0 <= kt[0, i] < i for i in range(1, NJ))
    assert list(kt[0, 22:25]) == [15, 15, 15] and list(kt[0, 25:40:3]) == [20] * 5 and list(kt[0, 40:55:3]) == [21] * 5
    ref = human_synth.PoseRefiner(joints=NJ)
    assert ref(torch.zeros(1, 3 * (NJ - 1)))["Rs"].shape == (1, NJ - 1, 3, 3)
    assert human_synth.LbsOffsetDecoder(joints=NJ)(torch.zeros(1, 7, 3)).shape == (1, NJ, 7)
    # the SMPL body is still the default and unchanged in shape
    s = human_synth.body_arrays()
    assert s["weights"].shape == (6890, 24) and s["posedirs"].shape == (6890, 3, 207) and s["shapedirs"].shape == (6890, 3, 10)
