"""The skinning-offset network at SMPL-X's 55 bones, host side: the bone-count entry points of csrc/mlp.hip (declared, exported,
nb checked first), the module contracts of nets.py at 24 and 55 bones, and a decoder that survives pickle (GaussianModel.capture()
pickles it).  No GPU: every call here stops before a device is touched."""
import os
import pickle
import re
import sys
import types

import torch

from mygauhuman_amd import nets
from mygauhuman_amd._lib import SYMBOLS, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB_NAMES = ("gsr_lbs_offset_mlp_packed_floats_nb", "gsr_lbs_offset_mlp_pack_nb", "gsr_lbs_offset_mlp_forward_nb",
            "gsr_debug_lbs_offset_mlp_forward_bf16x3_nb", "gsr_lbs_offset_mlp_backward_workspace_floats_nb",
            "gsr_lbs_offset_mlp_backward_nb")


def test_bone_count_entry_points_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    for n in NB_NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert n in SYMBOLS and hasattr(lib, n) and getattr(lib, n).argtypes is not None, n


def test_unsupported_bone_count_is_refused_first():
    z5 = (lib.gsr_lbs_offset_mlp_pack_nb.argtypes[1]._type_ * 5)()
    # every other argument is null / zero: nb is looked at before them
    calls = (("gsr_lbs_offset_mlp_pack_nb", lambda: lib.gsr_lbs_offset_mlp_pack_nb(30, None, None, None, None)),
             ("gsr_lbs_offset_mlp_forward_nb", lambda: lib.gsr_lbs_offset_mlp_forward_nb(30, 0, None, None, None, None)),
             ("gsr_debug_lbs_offset_mlp_forward_bf16x3_nb",
              lambda: lib.gsr_debug_lbs_offset_mlp_forward_bf16x3_nb(30, 0, None, None, None, None)),
             ("gsr_lbs_offset_mlp_backward_nb",
              lambda: lib.gsr_lbs_offset_mlp_backward_nb(30, 0, None, None, None, None, z5, z5, None)))
    for name, call in calls:
        assert call() == -1, name
        msg = lib.gsr_last_error()
        assert name.encode() in msg and b"30" in msg and b"24" in msg and b"55" in msg, msg
    # the two size queries answer 0
    assert lib.gsr_lbs_offset_mlp_packed_floats_nb(30) == 0 and b"30" in lib.gsr_last_error()
    assert lib.gsr_lbs_offset_mlp_backward_workspace_floats_nb(30, 1000) == 0 and b"55" in lib.gsr_last_error()


def test_zero_points_is_a_no_op_for_both_bone_counts():
    z5 = (lib.gsr_lbs_offset_mlp_pack_nb.argtypes[1]._type_ * 5)()
    for nb in nets.FUSED_BONE_COUNTS:
        assert lib.gsr_lbs_offset_mlp_forward_nb(nb, 0, None, None, None, None) == 0
        assert lib.gsr_debug_lbs_offset_mlp_forward_bf16x3_nb(nb, 0, None, None, None, None) == 0
        assert lib.gsr_lbs_offset_mlp_backward_nb(nb, 0, None, None, None, None, z5, z5, None) == 0
        assert lib.gsr_lbs_offset_mlp_backward_workspace_floats_nb(nb, 0) == 0
        # a null pointer with P > 0 is still an argument error (after nb)
        assert lib.gsr_lbs_offset_mlp_forward_nb(nb, 5, None, None, None, None) == -1
        assert b"gsr_lbs_offset_mlp_forward_nb" in lib.gsr_last_error()


def test_packed_sizes():
    n24, n55 = lib.gsr_lbs_offset_mlp_packed_floats_nb(24), lib.gsr_lbs_offset_mlp_packed_floats_nb(55)
    assert n24 == lib.gsr_lbs_offset_mlp_packed_floats() and n55 > n24 and n55 % 4 == 0
    for P in (1, 256, 1000):
        assert lib.gsr_lbs_offset_mlp_backward_workspace_floats_nb(24, P) == lib.gsr_lbs_offset_mlp_backward_workspace_floats(P)
        assert lib.gsr_lbs_offset_mlp_backward_workspace_floats_nb(55, P) > lib.gsr_lbs_offset_mlp_backward_workspace_floats(P)


def test_module_contracts_at_24_and_55_bones():
    assert nets.FUSED_BONE_COUNTS == (24, 55)
    assert nets.FusedLBSOffsetDecoder().use_fused
    assert not nets.FusedLBSOffsetDecoder(total_bones=55).use_fused
    assert not nets.FusedLBSOffsetDecoder(total_bones=30).use_fused
    for nb in (24, 55):
        dec = nets.LBSOffsetDecoder(total_bones=nb)
        assert dec.use_fused and isinstance(dec, nets.FusedLBSOffsetDecoder)
        assert sorted(dec.state_dict()) == sorted([f"bw_linears.{i}.{k}" for i in range(4) for k in ("weight", "bias")]
                                                  + ["bw_fc.weight", "bw_fc.bias"])
        assert tuple(dec.bw_fc.weight.shape) == (nb, 128, 1)
    assert not nets.LBSOffsetDecoder(total_bones=30).use_fused
    assert nets.LBSOffsetDecoder().total_bones == 24


def test_dropin_hands_the_reference_the_fused_55_bone_decoder():
    import mygauhuman_amd
    sys.modules.setdefault("nets", types.ModuleType("nets"))   # (the reference's package when its tree is on the path)
    mygauhuman_amd.install_dropin(nets=True)
    from nets.mlp_delta_weight_lbs import LBSOffsetDecoder
    assert LBSOffsetDecoder is nets.LBSOffsetDecoder
    assert LBSOffsetDecoder(total_bones=55).use_fused     # GaussianModel(smpl_type="smplx", motion_offset_flag=True)
    assert not nets.FusedLBSOffsetDecoder(55).use_fused


def test_cpu_input_at_55_bones_takes_the_torch_ops_and_at_24_raises():
    torch.manual_seed(0)
    pts = torch.rand(1, 40, 3) - 0.5
    dec = nets.LBSOffsetDecoder(total_bones=55)
    with torch.no_grad():
        assert torch.equal(dec(pts), dec.forward_torch(pts))
    dec24 = nets.LBSOffsetDecoder(total_bones=24)
    try:
        with torch.no_grad():
            dec24(pts)
        raise AssertionError("a CPU input at 24 bones must raise")
    except RuntimeError as e:
        assert "HIP device" in str(e)


def test_pickled_decoder_runs():
    torch.manual_seed(1)
    pts = torch.rand(1, 33, 3) - 0.5
    for nb in (24, 55):
        dec = nets.LBSOffsetDecoder(total_bones=nb)
        dec._packed, dec._packed_key = torch.zeros(4), ("stale",)   # a device-side cache is not part of the pickle
        back = pickle.loads(pickle.dumps(dec))
        assert "_packed" not in back.__dict__ and back._packed is None and back._packed_key is None
        assert back.use_fused and back.total_bones == nb
        with torch.no_grad():
            assert torch.equal(back.forward_torch(pts), dec.forward_torch(pts))
    # a pickle made without the attributes at all (an older module): the class defaults take over
    dec = nets.FusedLBSOffsetDecoder(total_bones=55)
    state = dec.__getstate__()
    state.pop("use_fused")
    old = nets.FusedLBSOffsetDecoder.__new__(nets.FusedLBSOffsetDecoder)
    old.__setstate__(state)
    assert old.use_fused is False
    with torch.no_grad():
        assert torch.equal(old(pts), dec.forward_torch(pts))
