"""The float64 / float32 restatements of the deform path (tests/deform_reference.py) and the case builders
(tests/deform_cases.py), checked without a GPU: against the C oracle that tests/golden pins to the imported smplx.lbs, against
the J = 55 golden fixture, and for everything the builders promise.  tests/test_gpu_deform_f64.py relies on all of it."""
import os

import numpy as np
import pytest
import torch

from tests import deform_cases as dc
from tests import deform_reference as dr

NOISE = 16 * dr.ULP   # "float32 noise" between two float32 evaluations of the same chain, by the measure of util.assert_close


def _t(a, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float64)).to(dtype)


def _exactly_float32(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


def _check_e32(name, w32, w64, scale=None):
    """A float32 checker that is accidentally float64 has e32 = 0; one that is accidentally wrong has a large one.  e32 = 0 is in
    order only where the float64 result needs no rounding at all (an identity matrix, a gradient that is exactly zero)."""
    if np.asarray(w64).size == 0:
        return
    e = dr.measure(w32, w64) if scale is None else dr.measure_reduced(w32, w64, scale)
    assert e < 1e-5, (name, e)
    assert e > 0.0 or _exactly_float32(w64), (name, "the float32 checker reproduces float64 exactly")


# ------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", ["P257", "no_offsets", "sparse", "P1"])
def test_deform_float32_matches_c_oracle(oracle, name):
    c = dc.lbs_case(name, 24)
    ids = oracle.nearest_vertex(c["query"], c["verts"])
    want = oracle.lbs_deform(c["query"], c["normals"], ids, c["weights"], c["A_big"], c["A_pose"], c["off_big"], c["off_shape"],
                             c["off_pose"], c["R"], c["Th"], lbs_off=c["loff"])
    got = dr.deform64(*[_t(c[k], torch.float32) for k in dr.LBS_INPUTS], torch.from_numpy(ids.astype(np.int64)),
                      _t(c["weights"], torch.float32))
    for k_got, k_want in (("world_pts", "world_src"), ("smpl_pts", "smpl_src"), ("bweights", "bweights"), ("transforms", "transforms"),
                          ("translation", "translation"), ("world_normals", "world_normals")):
        e = dr.measure(got[k_got].numpy(), want[k_want])
        assert e < NOISE, (k_got, e)


def test_pose_chain_matches_c_oracle(oracle):
    from tests.test_gpu_lbs import make_smpl
    m = make_smpl(300, 4)
    rng = np.random.default_rng(2)
    for pose in (dc.big_pose(24), rng.normal(0, 0.4, 72).astype(np.float32), np.zeros(72, np.float32)):
        betas = rng.normal(0, 1, 10).astype(np.float32)
        rot_o = oracle.rodrigues(pose)
        A_o, joints_o = oracle.joint_transforms(m, betas, rot_o)
        for dtype, tol in ((torch.float32, NOISE), (torch.float64, NOISE)):
            rot, A = dr.pose_chain64(_t(pose, dtype), _t(joints_o, dtype), dc.PARENTS_SMPL)
            assert dr.measure(rot.numpy(), rot_o) < tol and dr.measure(A.numpy(), A_o) < tol, dtype
            assert torch.equal(A[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=dtype).expand(24, 4))


def test_pose_chain_matches_golden_fixtures(golden_dir):
    """The J = 55 fixture of test_pose_chain_55_matches_reference_fixture (and the J = 24 one): A and rot_mats of the imported
    reference, from joints regressed in float64."""
    for name, J in (("lbs_smplx.npz", 55), ("lbs_smpl.npz", 24)):
        g = np.load(os.path.join(golden_dir, name))
        d = lambda k: np.asarray(g[k], np.float64)  # noqa: E731
        nb = g["betas"].shape[-1]
        joints = d("smpl_J_regressor") @ (d("smpl_v_template") + d("smpl_shapedirs")[..., :nb] @ d("betas").reshape(-1))
        for dtype in (torch.float64, torch.float32):
            rot, A = dr.pose_chain64(_t(g["pose"].reshape(-1), dtype), _t(joints, dtype), [int(v) for v in g["smpl_parents"]])
            assert dr.measure(A.numpy(), g["A"]) < 1e-5 and dr.measure(rot.numpy(), g["rot_mats"]) < 1e-5, (name, dtype)
    assert dc.parents_smplx() == tuple(int(v) for v in np.load(os.path.join(golden_dir, "lbs_smplx.npz"))["smpl_parents"])


def test_rodrigues_matches_golden_vectors(golden_dir):
    g = np.load(os.path.join(golden_dir, "lbs_smpl.npz"))
    assert dr.measure(dr.rodrigues64(_t(g["rodrigues_in"])).numpy(), g["rodrigues_out"]) < NOISE


# ------------------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("J", dc.JOINTS)
@pytest.mark.parametrize("name", ["P257", "no_normals", "single_vertex"])
def test_two_stage_gradients_equal_autograd(oracle, name, J):
    """The two-stage sums of d_A_pose / d_off_pose are what autograd gives for the whole map (float64), and inv3 is the inverse."""
    c = dc.lbs_case(name, J)
    _, (_, g, s_abs), _ = dc.reference(oracle, c, (name, J))
    for k in ("A_pose", "off_pose"):
        assert dr.measure_reduced(g[k], g[k + "_autograd"], s_abs[k]) < 1e-13, k
        assert (s_abs[k] >= np.abs(g[k]) * (1 - 1e-12)).all()
    assert not g["A_pose"][:, 3].any()
    m = torch.from_numpy(np.random.default_rng(0).normal(0, 1, (5, 3, 3)))
    assert float((dr.inv3(m) - torch.inverse(m)).abs().max()) < 1e-10


@pytest.mark.parametrize("J", dc.JOINTS)
@pytest.mark.parametrize("name", sorted(dc.LBS_CASES))
def test_lbs_cases_keep_their_promises_and_have_a_float32_noise_floor(oracle, name, J):
    c = dc.lbs_case(name, J)
    P = c["query"].shape[0]
    assert P <= 513 and c["verts"].shape[0] <= 2049 and c["weights"].shape == (c["verts"].shape[0], J)
    # world transform
    R = np.asarray(c["R"], np.float64)
    s = np.linalg.svd(R, compute_uv=False)
    assert 0.7 <= s.min() and s.max() <= 1.4 and np.abs(R @ R.T - np.eye(3)).max() > 0.05 and np.abs(c["Th"]).min() > 0
    assert np.abs(np.linalg.inv(R) - R.T).max() > 0.05
    ids, (o64, g64, s_abs), (o32, g32, _) = dc.reference(oracle, c, (name, J))
    assert np.array_equal(ids, dc.nearest_f32(c["query"], c["verts"]))
    if P:
        cond = dc.blended_big_condition(c, ids)
        if name == "illcond":
            assert 50 <= cond.min() and cond.max() <= 500, (cond.min(), cond.max())
        else:
            assert cond.max() <= 20, cond.max()
    w = c["weights"]
    assert np.abs(w.sum(1) - 1).max() < 1e-6
    if name.startswith("sparse") or name in ("saturated", "equal_offsets"):
        nz = (w != 0).sum(1)
        assert nz.min() == 1 and nz.max() <= 4 and (nz == 1).sum() >= w.shape[0] // 4 and (w[nz == 1].max(1) == 1.0).all()
    if name == "saturated":
        assert ((c["loff"] == 30.0).sum(1) == (np.arange(P) % 2 == 0)).all()
        assert np.isfinite(g64["loff"]).all() and np.abs(g64["loff"].sum(1)).max() < 1e-9   # a softmax adjoint sums to zero
        assert np.abs(g64["loff"][0::2]).max() < 1e-2 * np.abs(g64["loff"][1::2]).max(), "the saturated rows are near zero"
    if name == "equal_offsets":
        assert (c["loff"] == c["loff"][:, :1]).all()
        assert dr.measure(o64["bweights"], w[ids]) < dr.ULP   # (w + 1e-9) / (1 + 1e-9 J): the plain weights to under one ulp
    if name == "clustered":
        assert len(np.unique(ids)) == 3
    if name == "one_joint":
        assert (w[:, 3] == 1).all()
    # the noise floor
    for k in dr.LBS_OUTPUTS:
        if o64[k] is not None:
            _check_e32(k, o32[k], o64[k])
    for k in ("query", "normals", "loff"):
        if k in g64:
            _check_e32("d_" + k, g32[k], g64[k])
    for k in ("A_pose", "off_pose"):
        _check_e32("d_" + k, g32[k], g64[k], s_abs[k])


@pytest.mark.parametrize("J", dc.JOINTS)
def test_illcond_noise_is_the_rounding_of_the_blend_weights(oracle, J):
    """Why the GPU test gives d_lbs_offsets and d_query of the case "illcond" a factor above two (measured 3.16 and 2.25 x e32):
    the float32 checker with its blend weights re-rounded by at most two ulps (what another logf / expf / division, each good to
    an ulp, does to them) moves further from float64 than that in both tensors -- the condition number at work.  One-sided: the
    statement is that the rounding of the weights accounts for AT LEAST the measured excess."""
    c = dc.lbs_case("illcond", J)
    ids, (_, g64, _), (_, g32, _) = dc.reference(oracle, c, ("illcond", J))
    worst = {"query": 0.0, "loff": 0.0}
    for seed in range(3):
        rng = np.random.default_rng(seed)
        hook = lambda bw: bw * (1 + torch.from_numpy(rng.uniform(-1, 1, tuple(bw.shape)).astype(np.float32)) * np.float32(2 * dr.ULP))  # noqa: E731,B023
        _, g, _ = dr.deform_reference(c, ids, torch.float32, bw_hook=hook)
        for k in worst:
            worst[k] = max(worst[k], dr.measure(g[k], g64[k]) / dr.measure(g32[k], g64[k]))
    print(worst)
    assert worst["loff"] > 3.16 and worst["query"] > 2.25, worst


@pytest.mark.parametrize("J", dc.JOINTS)
@pytest.mark.parametrize("V", dc.V_TAILS)
def test_vertex_tail_cases_have_their_planted_answers(oracle, J, V):
    c = dc.vtail_case(J, V)
    assert c["verts"].shape == (V, 3) and c["query"].shape == (257, 3)
    ids = oracle.nearest_vertex(c["query"], c["verts"])
    pl = c["planted"]
    assert len(pl["last"]) and (ids[pl["last"]] == V - 1).all()
    if V >= 1025:
        assert len(pl["first_of_tile"]) and (ids[pl["first_of_tile"]] == 1024).all()
        q, v = c["query"][pl["tie"]], c["verts"]
        d = lambda i: ((v[i, 0] - q[:, 0]) ** 2 + (v[i, 1] - q[:, 1]) ** 2) + (v[i, 2] - q[:, 2]) ** 2   # noqa: E731  (float32, the kernels' expression)
        assert d(1023).dtype == np.float32 and np.array_equal(d(1023), d(1024)) and len(pl["tie"])
        assert (ids[pl["tie"]] == 1023).all()
        others = np.delete(np.arange(V), [1023, 1024])
        assert (((v[others][None] - q[:, None]) ** 2).sum(-1).min(1) > 4 * d(1023)).all()
    else:
        assert not len(pl["tie"]) and not len(pl["first_of_tile"])
    _, (o64, _, _), (o32, _, _) = dc.reference(oracle, c, ("vtail", J, V))
    for k in dr.LBS_OUTPUTS:
        _check_e32(k, o32[k], o64[k])


@pytest.mark.parametrize("J", dc.JOINTS)
def test_cache_case_has_known_radii(oracle, J):
    c = dc.cache_case(J)
    rho, rho_rings = dc.cache_radii(c)
    ids = oracle.nearest_vertex(c["query"], c["verts"])
    assert (ids[5:8] == 10).all() and np.array_equal(rho == 0, ids == 10)   # the duplicated vertex, and nothing else, ties
    still = np.ones(257, bool)
    still[list(dc.CACHE_MOVED)] = False
    assert ((rho_rings[still] == 0) == (rho[still] == 0)).all() and rho_rings[still & (rho > 0)].min() > 1e-5
    step = np.abs(c["query2"].astype(np.float64) - c["query"])
    assert (step[still].max(1) > 0).all() and np.sqrt((step[still] ** 2).sum(1)).max() < 3e-6
    spacing = (1.8 * 1.8 * 0.3 / 300) ** (1 / 3)
    assert (np.sqrt((step[~still] ** 2).sum(1)) > 3 * spacing).all()


def test_nonfinite_case_rows():
    bad, fin = dc.nonfinite_case(24)
    q = bad["query"]
    assert np.isnan(q[0]).all() and np.isposinf(q[100]).all() and (q[256] == np.float32(3e19)).all()
    with np.errstate(over="ignore"):
        assert np.isinf(q[256, 0] * q[256, 0])          # the squared distance overflows
    rest = np.delete(np.arange(257), list(dc.NONFINITE_ROWS))
    assert np.array_equal(q[rest], fin["query"][rest]) and np.isfinite(fin["query"]).all()


# ------------------------------------------------------------------------------------------------------ pose cases
@pytest.mark.parametrize("tree,J", dc.POSE_TREES)
@pytest.mark.parametrize("kind", dc.POSE_KINDS)
def test_pose_cases_keep_their_promises_and_have_a_float32_noise_floor(tree, J, kind):
    c = dc.pose_case(tree, J, kind)
    par, p = c["parents"], c["poses"].astype(np.float64)
    assert len(par) == J and all(0 <= par[i] < i for i in range(1, J))
    if tree == "chain":
        assert all(par[i] == i - 1 for i in range(1, J))
    if tree == "star":
        assert all(par[i] == 0 for i in range(1, J))
    ang = np.linalg.norm(p, axis=1)
    if kind == "zero":
        assert not p.any()
    elif kind == "big":
        assert (p != 0).sum() == min(4, sum(k < 3 * J for k, _ in dc.BIG_POSE_ENTRIES)) and (J != 24 or (p == 0).sum() == 68)
    elif kind in ("tiny7", "tiny4"):
        assert np.allclose(ang[1::2], 1e-7 if kind == "tiny7" else 1e-4, rtol=1e-3) and (ang[0::2] > 1e-2).all()
    elif kind == "axis":
        assert ((p != 0).sum(1) == 1).all()
    elif kind == "near_pi":
        assert np.allclose(ang, np.array(dc.NEAR_PI)[np.arange(J) % 3], atol=1e-6) and (ang[1::3] > np.pi).all() and (ang[0::3] < np.pi).all()
    cr = c["correct_Rs"].astype(np.float64)
    assert np.abs(cr @ cr.transpose(0, 2, 1) - np.eye(3)).max() > 0.05
    for with_correct in (False, True):
        for loss in ("A", "rot", "both"):
            r64, r32 = dc.pose_reference(tree, J, kind, with_correct, loss)
            assert all(np.isfinite(v).all() for v in r64.values())
            assert np.array_equal(r64["A"][:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (J, 1)))
            for k in r64:
                _check_e32(f"{k} ({loss}, correct_Rs {with_correct})", r32[k], r64[k])
    if kind == "zero":
        assert np.array_equal(dc.pose_reference(tree, J, kind, False, "both")[0]["rot_mats"], np.tile(np.eye(3), (J, 1, 1)))


def test_deep_chain_noise_floor_moves_with_half_an_ulp():
    """Why the GPU test gives A of the 64-deep chain at angles around pi a factor above two (measured 4.0 x e32): A evaluated in
    float32 in the kernel's order (row times column, left to right), from the checker's own rot_mats and from eight copies of them
    re-rounded by at most half an ulp, scatters by more than the factor of two the default bound allows: 64 chained products
    amplify which way each one was rounded, and e32 is ONE sample of that.  One-sided on purpose."""
    c = dc.pose_case("chain", 64, "near_pi")
    r64, r32 = dc.pose_reference("chain", 64, "near_pi", True, "both")
    f = np.float32
    joints, par = c["joints"].astype(f), c["parents"]

    def chain(rot):
        G = np.zeros((64, 3, 4), f)
        G[0, :, :3], G[0, :, 3] = rot[0], joints[0]
        for i in range(1, 64):
            Gp = G[par[i]]
            tm = np.concatenate([rot[i], (joints[i] - joints[par[i]])[:, None]], 1)
            acc = (Gp[:, 0:1] * tm[0:1] + Gp[:, 1:2] * tm[1:2]) + Gp[:, 2:3] * tm[2:3]
            acc[:, 3] += Gp[:, 3]
            G[i] = acc
        A = np.zeros((64, 4, 4))
        A[:, :3, :3], A[:, 3, 3] = G[:, :, :3], 1.0
        A[:, :3, 3] = G[:, :, 3] - ((G[:, :, 0] * joints[:, 0:1] + G[:, :, 1] * joints[:, 1:2]) + G[:, :, 2] * joints[:, 2:3])
        return A
    rot = r32["rot_mats"].astype(f)
    rng = np.random.default_rng(0)
    errs = [dr.measure(r32["A"], r64["A"]), dr.measure(chain(rot), r64["A"])]
    for _ in range(8):
        errs.append(dr.measure(chain((rot * (1 + rng.uniform(-1, 1, rot.shape).astype(f) * f(2.0 ** -24))).astype(f)), r64["A"]))
    print(errs)
    assert max(errs) > 2 * min(errs), errs
