"""The pose-correction network (nets_pose.FusedBodyPoseRefiner, csrc/pose_refiner.hip), host side: the float64 restatement
(tests/pose_refiner_reference.py) against the fixture made by the reference's own BodyPoseRefiner (tests/golden/
make_golden_pose_refiner.py), the module's reference contracts (state_dict, initialisation bit for bit, forward_torch), the drop-in
registration, pickling, and the C entry points' argument checks.  No GPU: every call here stops before a device is touched."""
import hashlib
import os
import pickle
import re
import sys
import types

import numpy as np
import pytest
import torch

from mygauhuman_amd import nets_pose
from mygauhuman_amd._lib import SYMBOLS, lib
from tests import pose_refiner_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("w0", "b0", "w2", "b2", "w4", "b4")
INIT_SEED = 11      # tests/golden/make_golden_pose_refiner.py


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "pose_refiner.npz")) as z:
        return {k: z[k] for k in z.files}


def _case_params(golden, J):
    return [torch.from_numpy(golden[f"case_J{J}_{n}"].astype(np.float64)) for n in NAMES]


def _build(J):
    return nets_pose.FusedBodyPoseRefiner(total_bones=J, embedding_size=3 * (J - 1), mlp_width=128, mlp_depth=2)


@pytest.mark.parametrize("J", [24, 55])
@pytest.mark.parametrize("B", [1, 3])
def test_float64_restatement_matches_the_reference(golden, J, B):
    ps = [p.clone().requires_grad_(True) for p in _case_params(golden, J)]
    x = torch.from_numpy(golden[f"case_J{J}_x"][:B]).requires_grad_(True)
    g = torch.from_numpy(golden[f"case_J{J}_g"][:B])
    Rs = ref.forward(x, ps)
    tag = f"case_J{J}_B{B}"
    np.testing.assert_allclose(Rs.detach().numpy(), golden[f"{tag}_Rs"], rtol=0, atol=1e-12)
    (Rs * g).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), golden[f"{tag}_dx"], rtol=0, atol=1e-12)
    acts = {"w0": golden[f"case_J{J}_x"][0]}
    if B == 1:
        acts.update(w2=golden[f"{tag}_h1"], w4=golden[f"{tag}_h2"])
    for n, p in zip(NAMES, ps):
        if n.startswith("b") or B == 3:
            want = golden[f"{tag}_d{n}"]
        else:   # (B = 1: the reference's weight gradient is this outer product exactly)
            want = np.outer(golden[f"{tag}_d{'b' + n[1:]}"], acts[n])
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(p.grad.numpy(), want, rtol=0, atol=1e-12 * scale, err_msg=n)
    # the fixture covers what it claims: theta from 0.0032 (the zero row: sqrt(1e-5)) to large rotations
    r = ref.preactivations(x.detach(), [p.detach() for p in ps])[2].view(-1, 3)
    theta = torch.sqrt(1e-5 + (r * r).sum(1))
    assert float(theta.min()) == pytest.approx(np.sqrt(1e-5), rel=1e-9) and float(theta.max()) > 2.9


@pytest.mark.parametrize("J", [24, 55])
def test_state_dict_and_initialisation_equal_the_reference(golden, J):
    torch.manual_seed(INIT_SEED)
    m = _build(J)
    sd = m.state_dict()
    assert list(sd) == list(ref.PARAM_NAMES)
    for key, n in zip(ref.PARAM_NAMES, NAMES):
        a = sd[key].numpy()
        assert a.dtype == np.float32 and tuple(a.shape) == tuple(golden[f"init_J{J}_{n}_shape"]), key
        np.testing.assert_array_equal(a.reshape(-1)[:16], golden[f"init_J{J}_{n}_head"], err_msg=key)
        assert hashlib.sha256(a.tobytes()).hexdigest() == str(golden[f"init_J{J}_{n}_sha256"]), key   # bit for bit
    assert m.total_bones == J - 1 and isinstance(m.rodriguez, nets_pose.RodriguesModule)
    assert [type(x).__name__ for x in m.block_mlps] == ["Linear", "ReLU", "Linear", "ReLU", "Linear"]
    # the reference's defaults: 69 -> 256 x 4 -> 69
    d = nets_pose.BodyPoseRefiner()
    assert len(d.block_mlps) == 9 and tuple(d.block_mlps[-1].weight.shape) == (69, 256) and d.total_bones == 23


@pytest.mark.parametrize("J", [24, 55])
def test_cpu_forward_torch_matches_the_restatement(golden, J):
    m = _build(J).double()
    with torch.no_grad():
        for p, v in zip([t for i in (0, 2, 4) for t in (m.block_mlps[i].weight, m.block_mlps[i].bias)], _case_params(golden, J)):
            p.copy_(v)
    x = torch.from_numpy(golden[f"case_J{J}_x"])
    want = ref.forward(x, _case_params(golden, J))
    with torch.no_grad():
        got = m(x)["Rs"]                              # a CPU input: the torch ops
    assert got.shape == (3, J - 1, 3, 3)
    assert float((got - want).abs().max()) < 1e-12
    m32 = m.float()
    with torch.no_grad():
        got32 = m32(x.float())["Rs"]
    assert float((got32.double() - want).abs().max()) < 1e-5
    assert m32.fused_params(x.float()) is None        # (not a HIP tensor)


def test_dropin_registers_the_reference_module_path():
    import mygauhuman_amd
    saved = {k: sys.modules.get(k) for k in ("nets", "nets.mlp_delta_body_pose", "nets.mlp_delta_weight_lbs")}
    try:
        sys.modules.setdefault("nets", types.ModuleType("nets"))   # (the reference's package when its tree is on the path)
        sys.modules.pop("nets.mlp_delta_body_pose", None)
        mygauhuman_amd.install_dropin(nets=True)
        assert "nets.mlp_delta_body_pose" not in sys.modules        # nets=True keeps its meaning
        mygauhuman_amd.install_dropin(pose_refiner=True)
        from nets.mlp_delta_body_pose import BodyPoseRefiner, RodriguesModule
        assert BodyPoseRefiner is nets_pose.FusedBodyPoseRefiner and RodriguesModule is nets_pose.RodriguesModule
        assert BodyPoseRefiner(total_bones=55, embedding_size=162, mlp_width=128, mlp_depth=2).use_fused
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_pickle_round_trip_and_a_reference_pickle():
    torch.manual_seed(2)
    x = torch.randn(2, 69) * 0.3
    m = _build(24)
    with torch.no_grad():
        m.block_mlps[4].weight.mul_(1e4)
        want = m.forward_torch(x)["Rs"]
        back = pickle.loads(pickle.dumps(m))
        assert type(back) is nets_pose.FusedBodyPoseRefiner and back.use_fused
        assert torch.equal(back(x)["Rs"], want)
        # a module pickled without the fused-only attribute (as the reference's class pickles): the class default takes over
        del m.use_fused
        assert "use_fused" not in m.__dict__ and m.use_fused
        old = pickle.loads(pickle.dumps(m))
        assert "use_fused" not in old.__dict__ and torch.equal(old(x)["Rs"], want)
    # the reference's own class names under the reference's module path, pickled, then unpickled after the drop-in
    fake = types.ModuleType("nets.mlp_delta_body_pose")
    fake.BodyPoseRefiner = type("BodyPoseRefiner", (torch.nn.Module,), {"__module__": "nets.mlp_delta_body_pose"})
    fake.RodriguesModule = type("RodriguesModule", (torch.nn.Module,), {"__module__": "nets.mlp_delta_body_pose"})
    saved = {k: sys.modules.get(k) for k in ("nets", "nets.mlp_delta_body_pose")}
    try:
        sys.modules.setdefault("nets", types.ModuleType("nets"))
        sys.modules["nets.mlp_delta_body_pose"] = fake
        m.__class__, m.rodriguez.__class__ = fake.BodyPoseRefiner, fake.RodriguesModule
        blob = pickle.dumps(m)
        sys.modules["nets.mlp_delta_body_pose"] = nets_pose
        theirs = pickle.loads(blob)
        assert type(theirs) is nets_pose.FusedBodyPoseRefiner and type(theirs.rodriguez) is nets_pose.RodriguesModule
        with torch.no_grad():
            assert torch.equal(theirs(x)["Rs"], want)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_unfused_configurations_take_the_torch_ops():
    x = torch.randn(3, 69)
    for m in (nets_pose.BodyPoseRefiner(), nets_pose.BodyPoseRefiner(total_bones=30, embedding_size=87, mlp_width=128, mlp_depth=2),
              _build(24)):
        assert m.fused_params(torch.randn(3, m.block_mlps[0].in_features)) is None
    assert _build(24)(x)["Rs"].shape == (3, 23, 3, 3)


def test_entry_points_are_declared_exported_and_check_their_arguments():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    for n in ("gsr_pose_refiner_forward", "gsr_pose_refiner_backward"):
        assert re.search(r"\b" + n + r"\s*\(", hdr) and n in SYMBOLS and getattr(lib, n).argtypes is not None, n
    z3 = (lib.gsr_pose_refiner_forward.argtypes[6]._type_ * 3)()
    fwd = lambda J, B, W, x=None, w=z3: lib.gsr_pose_refiner_forward(J, B, W, x, 1, 1, w, w, None, None)  # noqa: E731
    bwd = lambda J, B, W, x=None, w=z3: lib.gsr_pose_refiner_backward(J, B, W, x, 1, 1, w, w, None, w, w, None, None)  # noqa: E731
    for call, name in ((fwd, b"gsr_pose_refiner_forward"), (bwd, b"gsr_pose_refiner_backward")):
        assert call(30, 1, 128) == -1                      # J first: every pointer is null
        msg = lib.gsr_last_error()
        assert name in msg and b"30" in msg and b"24" in msg and b"55" in msg, msg
        assert call(24, 1, 256) == -1 and b"width" in lib.gsr_last_error()
        for B in (0, 17):
            assert call(55, B, 128) == -1 and b"B = %d" % B in lib.gsr_last_error()
        assert call(24, 1, 128) == -1 and b"null" in lib.gsr_last_error()
        assert call(24, 1, 128, x=16) == -1 and b"layer 0" in lib.gsr_last_error()   # (a non-null x, null weights)


def test_human_synth_refuses_an_unknown_pose_decoder():
    from mygauhuman_amd import human_synth
    with pytest.raises(ValueError, match="pose_decoder"):
        human_synth.build(10, motion=True, pose_decoder="reference")
