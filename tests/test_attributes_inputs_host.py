"""Host half of the float64 parity tests of the attribute kernel (tests/test_gpu_attributes_f64.py), no GPU needed:

  * the seeded inputs of every case keep the Gaussians whose non-differentiable selections (minimum-axis argsort, view flip,
    colour clamp) sit within attributes_cases.MARGIN of their switching point -- the ones the GPU comparison leaves out -- to at
    most 0.5 % per case, judged by the float64 reference alone;
  * the float32 and float64 CPU chains agree on every selection outside that margin (so the margin is wide enough for the
    checker's own arithmetic);
  * frame_attributes refuses tensors of the wrong shape, naming the argument, before it looks for a device.
"""
import numpy as np
import pytest
import torch

from tests import attributes_cases as ac


@pytest.mark.parametrize("P,layout,M,deg", ac.CASES, ids=[f"P{c[0]}-{c[1]}-M{c[2]}-deg{c[3]}" for c in ac.CASES])
def test_excluded_fraction_stays_within_the_cap(P, layout, M, deg):
    d, cam, _, _ = ac.make_inputs(P, M, ac.seed_of(P, layout, M, deg))
    ax, cl = ac.excluded_rows(d, cam, deg)
    n = int((ax | cl).sum())
    assert n <= ac.MAX_EXCLUDED_FRAC * P, f"{n} of {P} Gaussians within {ac.MARGIN} of a selection: pick another seed"


def test_float32_and_float64_chains_select_alike_outside_the_margin():
    """P = 513, degree 3: outside the margin the float32 chain clamps the same colour channels and flips the same axes as the
    float64 chain (a different selection would show as an O(1) difference of the axis feature / a zero against a non-zero)."""
    r = ac.reference(513, "one", 16, 3)
    keep = ~r["excluded"]
    assert np.array_equal(r["out32"]["colors"][keep] == 0, r["out64"]["colors"][keep] == 0)
    assert np.abs(r["out32"]["features"][keep, 15:] - r["out64"]["features"][keep, 15:]).max() < 1e-4


def _good(P=5):
    z = lambda *s: torch.zeros(s)  # noqa: E731
    return dict(means3D=z(P, 3), transforms=z(P, 3, 3), world_normals=z(P, 3), scales=z(P, 3), rot_cov=z(P, 4), rot_axis=z(P, 4),
                albedo=z(P, 3), roughness=z(P, 3), occlusion=z(P, 3), shs=z(P, 16, 3))


def _call(a):
    from mygauhuman_amd.attributes import frame_attributes
    return frame_attributes(a["means3D"], a["transforms"], a["world_normals"], a["scales"], 1.0, a["rot_cov"], a["rot_axis"],
                            a["albedo"], a["roughness"], a["occlusion"], a["shs"], 3, torch.zeros(3), torch.eye(4))


BAD = [("albedo", (5, 1)), ("roughness", (5, 1)), ("occlusion", (5, 1)), ("albedo", (4, 3)), ("roughness", (15,)), ("occlusion", (5, 4)),
       ("scales", (5, 1)), ("scales", (6, 3)), ("rot_cov", (5, 3)), ("rot_axis", (5, 3)), ("rot_axis", (4, 4)), ("transforms", (5, 3, 4)),
       ("transforms", (4, 3, 3)), ("world_normals", (5, 4)), ("world_normals", (6, 3)), ("shs", (4, 16, 3)), ("shs", (6, 16, 3))]


@pytest.mark.parametrize("name,shape", BAD, ids=[f"{n}{list(s)}" for n, s in BAD])
def test_frame_attributes_names_the_argument_of_a_wrong_shape(name, shape):
    a = _good()
    a[name] = torch.zeros(shape)
    with pytest.raises(RuntimeError, match=rf"frame_attributes: {name} must"):
        _call(a)


def test_frame_attributes_checks_both_tensors_of_an_sh_pair():
    a = _good()
    a["shs"] = (torch.zeros(5, 1, 3), torch.zeros(4, 15, 3))
    with pytest.raises(RuntimeError, match=r"frame_attributes: shs \(features_rest\) must"):
        _call(a)
    a["shs"] = (torch.zeros(6, 1, 3), torch.zeros(5, 15, 3))
    with pytest.raises(RuntimeError, match=r"frame_attributes: shs must"):
        _call(a)


def test_well_shaped_host_tensors_reach_the_device_check():
    """The shape contract is checked first and lets correct shapes through: what stops a CPU call is the device check."""
    with pytest.raises(RuntimeError, match="HIP device"):
        _call(_good())
