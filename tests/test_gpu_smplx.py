"""GPU tests of the SMPL-X (55-joint) articulated path: the pose chain, the 486-column pose-blend GEMV, the LBS kernels at J = 55
(forward variants, temporal cache, backward), coarse_deform_c2source with an SMPL-X-shaped model dict, render() end to end (eager
and as one graph), and the J = 24 case of the joint-count entry points against the original 24-joint ones.  The checkers are the
golden vectors of the reference (tests/golden/lbs_smplx.npz) and float64 torch restatements of scene/gaussian_model.py:768-980."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import util
from tests.deform_reference import deform64
from tests.torch_reference import pose_transforms_torch, rigid_chain, smpl_pose_transforms_torch

pytestmark = pytest.mark.gpu

NJ = 55


@pytest.fixture(scope="module", autouse=True)
def _release_smplx_tables():
    """The SMPL-X tables are large (posedirs alone 61 MB): drop what the LBS caches keep of them and hand the cached blocks back
    once this module is done, so later tests start from the allocator state they would see without it."""
    yield
    import gc

    from mygauhuman_amd import lbs
    torch.cuda.synchronize()
    lbs._GRIDS.entries.clear()
    lbs._CONSTANTS.entries.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)


def _body(V=None, seed=0):
    from mygauhuman_amd import human_synth
    b = human_synth.body_arrays(V, seed, body="smplx")
    b["kintree_table"] = human_synth.kintree_table("smplx")
    return b


def _smpl_dict(b, dev="cuda", dtype=torch.float32):
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev, dtype) for k, v in b.items() if k != "kintree_table"}
    out["kintree_table"] = torch.from_numpy(b["kintree_table"]).to(dev)
    return out


def _deform64(*args):
    """tests/deform_reference.deform64 as the tuple (world, transforms, normals, translation, bweights)."""
    o = deform64(*args)
    return o["world_pts"], o["transforms"], o["world_normals"], o["translation"], o["bweights"]


def _coarse64(smpl64, query, params, t_params, t_vertices, ids, lbs_weights=None, correct_Rs=None, normals=None):
    """float64 restatement of coarse_deform_c2source (:768-872) on CPU tensors."""
    from mygauhuman_amd.lbs import batch_rodrigues
    V = smpl64["v_template"].shape[0]

    def chain(p, cr=None):
        rot = batch_rodrigues(p["poses"].reshape(-1, 3)).view(1, -1, 3, 3)
        if cr is not None:
            rot = torch.cat([rot[:, :1], rot[:, 1:] @ cr.reshape(1, -1, 3, 3)], dim=1)
        A, _, _, _ = pose_transforms_torch(smpl64, p, rot_mats=rot)
        off = ((rot[0, 1:] - torch.eye(3, dtype=rot.dtype)).reshape(-1) @ smpl64["posedirs"].reshape(V * 3, -1).t()).reshape(V, 3)
        return A[0], off
    A_big, off_big = chain(t_params)
    A_pose, off_pose = chain(params, correct_Rs)
    nb = params["shapes"].shape[-1]
    off_shape = (smpl64["shapedirs"][..., :nb] @ params["shapes"].reshape(-1, 1)).squeeze(-1)
    return _deform64(query, normals, lbs_weights, A_big, A_pose, off_big, off_shape, off_pose, params["R"].reshape(3, 3),
                     params["Th"].reshape(3), ids, smpl64["weights"])


# ------------------------------------------------------------------------------------------------------------ 1. pose chain
def test_pose_chain_55_matches_reference_fixture(golden_dir):
    from mygauhuman_amd import lbs
    g = np.load(os.path.join(golden_dir, "lbs_smplx.npz"))
    d = util.to_dev
    smpl = dict(v_template=d(g["smpl_v_template"]), shapedirs=d(g["smpl_shapedirs"]), J_regressor=d(g["smpl_J_regressor"]),
                kintree_table=torch.from_numpy(np.stack([g["smpl_parents"], np.arange(NJ)])).cuda())
    params = dict(poses=d(g["pose"]), shapes=d(g["betas"]))
    A, rot, joints = lbs.smpl_pose_transforms(smpl, params)
    assert A.shape == (1, NJ, 4, 4) and rot.shape == (1, NJ, 3, 3)
    assert _rel(A[0], g["A"]) < 1e-5 and _rel(rot[0], g["rot_mats"]) < 1e-5


@pytest.mark.parametrize("with_correct", [False, True])
def test_pose_chain_55_forward_backward_float64(with_correct):
    from mygauhuman_amd import human_synth, lbs
    rng = np.random.default_rng(55 + with_correct)
    dev = torch.device("cuda:0")
    parents = tuple(int(v) for v in human_synth.PARENTS_SMPLX)
    poses = torch.tensor(rng.normal(0, 0.4, (1, 3 * NJ)), dtype=torch.float32, device=dev, requires_grad=True)
    joints = torch.tensor(rng.normal(0, 0.3, (NJ, 3)), dtype=torch.float32, device=dev, requires_grad=True)
    cr = None
    if with_correct:
        cr = torch.tensor(np.stack([np.eye(3) + rng.normal(0, 0.05, (3, 3)) for _ in range(NJ - 1)]), dtype=torch.float32,
                          device=dev, requires_grad=True)
    wA = torch.tensor(rng.normal(0, 1, (NJ, 4, 4)), dtype=torch.float32, device=dev)
    wR = torch.tensor(rng.normal(0, 1, (NJ, 3, 3)), dtype=torch.float32, device=dev)
    rot, A = lbs._SmplPose.apply(poses, cr, joints, parents)
    ((A * wA).sum() + (rot * wR).sum()).backward()

    p64 = poses.detach().double().requires_grad_(True)
    j64 = joints.detach().double().requires_grad_(True)
    c64 = None if cr is None else cr.detach().double().requires_grad_(True)
    rot64 = lbs.batch_rodrigues(p64.view(-1, 3)).view(1, NJ, 3, 3)
    if c64 is not None:
        rot64 = torch.cat([rot64[:, 0:1], torch.matmul(rot64[0, 1:], c64)[None]], dim=1)
    A64 = rigid_chain(rot64, j64[None], list(parents))
    ((A64[0] * wA.double()).sum() + (rot64[0] * wR.double()).sum()).backward()
    assert _rel(A.detach(), A64[0].detach()) < 1e-4 and _rel(rot.detach(), rot64[0].detach()) < 1e-4
    assert _rel(poses.grad, p64.grad) < 1e-4 and _rel(joints.grad, j64.grad) < 1e-4
    if cr is not None:
        assert _rel(cr.grad, c64.grad) < 1e-4
    assert torch.equal(A[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).expand(NJ, 4))


# ------------------------------------------------------------------------------------------------------------ 2. GEMV
@pytest.mark.parametrize("R,K", [(31425, 486), (31425, 257), (4099, 512), (1, 300)])
def test_row_gemv_wide_forward_backward(R, K):
    from mygauhuman_amd import lbs
    g = torch.Generator().manual_seed(R + K)
    mat = torch.randn((R, K), generator=g).cuda()
    vec = torch.randn((K,), generator=g).cuda().requires_grad_(True)
    w = torch.randn((R,), generator=g).cuda()
    out = lbs._RowGemv.apply(mat, vec)
    (out * w).sum().backward()
    ref = mat.double() @ vec.detach().double()
    dref = mat.double().t() @ w.double()
    assert float((out.detach().double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max() + 1e-30)
    assert float((vec.grad.double() - dref).abs().max()) <= 2e-5 * float(dref.abs().max() + 1e-30)


# ------------------------------------------------------------------------------------------------------------ 3./4. LBS at J = 55
def _lbs_case(P, seed, with_offsets):
    from mygauhuman_amd.lbs import batch_rodrigues
    rng = np.random.default_rng(seed)
    b = _body(seed=seed)
    V = b["v_template"].shape[0]
    parents = list(b["kintree_table"][0])
    joints = torch.from_numpy(rng.normal(0, 0.3, (1, NJ, 3)))

    def A_of(scale):
        rot = batch_rodrigues(torch.from_numpy(rng.normal(0, scale, (NJ, 3)))).view(1, NJ, 3, 3)
        return rigid_chain(rot, joints, parents)[0].numpy().astype(np.float32)
    big_verts = (b["v_template"] + 0.01 * rng.normal(0, 1, (V, 3))).astype(np.float32)
    c = dict(w=b["weights"], A_big=A_of(0.1), A_pose=A_of(0.3), big_verts=big_verts,
             off_big=rng.normal(0, 0.01, (V, 3)).astype(np.float32), off_shape=rng.normal(0, 0.01, (V, 3)).astype(np.float32),
             off_pose=rng.normal(0, 0.01, (V, 3)).astype(np.float32),
             query=(big_verts[rng.integers(0, V, P)] + rng.normal(0, 0.02, (P, 3))).astype(np.float32),
             normals=rng.normal(0, 1, (P, 3)).astype(np.float32),
             R=np.array([[np.cos(0.4), -np.sin(0.4), 0], [np.sin(0.4), np.cos(0.4), 0], [0, 0, 1]], np.float32),
             Th=np.array([0.1, -0.3, 2.5], np.float32),
             loff=rng.normal(0, 0.5, (P, NJ)).astype(np.float32) if with_offsets else None)
    return c


def _run_lbs(lbs, c, query, normals, search, cached, verts):
    d = util.to_dev
    old = (lbs.NEAREST_VERTEX_SEARCH, lbs.NN_TEMPORAL_CACHE)
    lbs.NEAREST_VERTEX_SEARCH, lbs.NN_TEMPORAL_CACHE = search, cached
    try:
        return lbs.lbs_deform(query, normals, None if c["loff"] is None else d(c["loff"]), d(c["A_big"]), d(c["A_pose"]),
                              d(c["off_big"]), d(c["off_shape"]), d(c["off_pose"]), d(c["R"]), d(c["Th"]), verts, d(c["w"]))
    finally:
        lbs.NEAREST_VERTEX_SEARCH, lbs.NN_TEMPORAL_CACHE = old


@pytest.mark.parametrize("P", [1, 20000])
@pytest.mark.parametrize("with_offsets", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
def test_lbs_forward_55_variants_identical_and_match_float64(oracle, P, with_offsets, with_normals):
    from mygauhuman_amd import lbs
    c = _lbs_case(P, 3 + P, with_offsets)
    d = util.to_dev
    verts = d(c["big_verts"])
    q, n = d(c["query"]), (d(c["normals"]) if with_normals else None)
    outs = {v: _run_lbs(lbs, c, q, n, *v, verts) for v in (("brute", False), ("grid", False), ("grid", True))}
    ids = oracle.nearest_vertex(c["query"], c["big_verts"])
    base = outs[("brute", False)]
    np.testing.assert_array_equal(base["vert_ids"].cpu().numpy(), ids)
    keys = ("world_pts", "transforms", "smpl_pts", "bweights", "translation", "vert_ids") + (("world_normals",) if with_normals else ())
    for v, o in outs.items():
        for k in keys:
            assert torch.equal(o[k], base[k]), (v, k)
    assert base["bweights"].shape == (P, NJ)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    world, tf, wn, transl, bw = _deform64(t64(c["query"]), t64(c["normals"]) if with_normals else None,
                                          None if c["loff"] is None else t64(c["loff"]), t64(c["A_big"]), t64(c["A_pose"]),
                                          t64(c["off_big"]), t64(c["off_shape"]), t64(c["off_pose"]), t64(c["R"]), t64(c["Th"]),
                                          torch.from_numpy(ids.astype(np.int64)), t64(c["w"]))
    util.assert_close("world_pts", base["world_pts"].cpu().numpy(), world.numpy(), tol=1e-4)
    util.assert_close("transforms", base["transforms"].cpu().numpy(), tf.numpy(), tol=1e-4)
    util.assert_close("translation", base["translation"].cpu().numpy(), transl.numpy(), tol=1e-4)
    util.assert_close("bweights", base["bweights"].cpu().numpy(), bw.numpy(), tol=1e-4)
    if with_normals:
        util.assert_close("world_normals", base["world_normals"].cpu().numpy(), wn.numpy(), tol=1e-4)


def test_lbs_55_temporal_cache_exact_across_frames(oracle):
    from mygauhuman_amd import lbs
    c = _lbs_case(20000, 9, True)
    d = util.to_dev
    verts = d(c["big_verts"])   # a tensor of its own: the cache starts empty
    q = d(c["query"])
    direction = torch.randn_like(q)
    for step in (0.0, 1e-3, 2e-2):
        q.add_(direction * step)
        got = _run_lbs(lbs, c, q, None, "grid", True, verts)
        want = _run_lbs(lbs, c, q, None, "grid", False, verts)
        for k in ("vert_ids", "world_pts", "transforms", "bweights"):
            assert torch.equal(got[k], want[k]), (step, k)
        np.testing.assert_array_equal(got["vert_ids"].cpu().numpy(), oracle.nearest_vertex(q.cpu().numpy(), c["big_verts"]))


@pytest.mark.parametrize("with_offsets", [False, True])
def test_lbs_backward_55_matches_autograd(oracle, with_offsets):
    from mygauhuman_amd import lbs
    P = 2500
    c = _lbs_case(P, 21, with_offsets)
    rng = np.random.default_rng(4)
    gw, gt, gn = rng.normal(0, 1, (P, 3)), rng.normal(0, 1, (P, 3, 3)), rng.normal(0, 1, (P, 3))
    ids = oracle.nearest_vertex(c["query"], c["big_verts"])
    t64 = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)  # noqa: E731
    rq, rn, rA, ro = t64(c["query"], True), t64(c["normals"], True), t64(c["A_pose"], True), t64(c["off_pose"], True)
    rl = t64(c["loff"], True) if with_offsets else None
    w, tf, wn, _, _ = _deform64(rq, rn, rl, t64(c["A_big"]), rA, t64(c["off_big"]), t64(c["off_shape"]), ro, t64(c["R"]),
                                t64(c["Th"]), torch.from_numpy(ids.astype(np.int64)), t64(c["w"]))
    ((w * t64(gw)).sum() + (tf * t64(gt)).sum() + (wn * t64(gn)).sum()).backward()
    d = util.to_dev
    hq, hn = d(c["query"]).requires_grad_(True), d(c["normals"]).requires_grad_(True)
    hA, ho = d(c["A_pose"]).requires_grad_(True), d(c["off_pose"]).requires_grad_(True)
    hl = d(c["loff"]).requires_grad_(True) if with_offsets else None
    o = lbs.lbs_deform(hq, hn, hl, d(c["A_big"]), hA, d(c["off_big"]), d(c["off_shape"]), ho, d(c["R"]), d(c["Th"]),
                       d(c["big_verts"]), d(c["w"]))
    ((o["world_pts"] * d(gw.astype(np.float32))).sum() + (o["transforms"] * d(gt.astype(np.float32))).sum()
     + (o["world_normals"] * d(gn.astype(np.float32))).sum()).backward()
    util.assert_close("d_query", hq.grad.cpu().numpy(), rq.grad.numpy(), tol=1e-4)
    util.assert_close("d_normals", hn.grad.cpu().numpy(), rn.grad.numpy(), tol=1e-4)
    assert hA.grad.shape == (NJ, 4, 4)
    util.assert_close("d_A_pose", hA.grad.cpu().numpy()[:, :3, :], rA.grad.numpy()[:, :3, :], tol=1e-4)
    util.assert_close("d_off_pose", ho.grad.cpu().numpy(), ro.grad.numpy(), tol=1e-4)
    if with_offsets:
        assert hl.grad.shape == (P, NJ)
        util.assert_close("d_lbs_offsets", hl.grad.cpu().numpy(), rl.grad.numpy(), tol=1e-4)


# ------------------------------------------------------------------------------------------------------------ 5. coarse deform
def test_coarse_deform_c2source_smplx(oracle):
    from mygauhuman_amd import lbs
    rng = np.random.default_rng(8)
    b = _body(seed=1)
    V, P = b["v_template"].shape[0], 6000
    smpl, smpl64 = _smpl_dict(b), _smpl_dict(b, "cpu", torch.float64)
    t_vertices = (b["v_template"] + 0.01 * rng.normal(0, 1, (V, 3))).astype(np.float32)
    query = (t_vertices[rng.integers(0, V, P)] + rng.normal(0, 0.02, (P, 3))).astype(np.float32)
    normals = rng.normal(0, 1, (P, 3)).astype(np.float32)
    cr = np.stack([np.eye(3) + rng.normal(0, 0.03, (3, 3)) for _ in range(NJ - 1)])[None].astype(np.float32)
    loff = rng.normal(0, 0.5, (1, P, NJ)).astype(np.float32)
    ang = 0.3
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    params_np = dict(poses=rng.normal(0, 0.2, (1, 3 * NJ)), shapes=rng.normal(0, 0.5, (1, 20)), R=R, Th=np.array([[0.1, 0.2, 2.0]]))
    t_np = dict(poses=np.zeros((1, 3 * NJ)), shapes=np.zeros((1, 20)), R=np.eye(3), Th=np.zeros((1, 3)))
    dv = lambda a: util.to_dev(np.asarray(a, np.float32))  # noqa: E731
    c64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    smpl_src, world, bw, tf, transl, wn = lbs.coarse_deform_c2source(
        smpl, dv(query[None]), {k: dv(v) for k, v in params_np.items()}, {k: dv(v) for k, v in t_np.items()}, dv(t_vertices[None]),
        lbs_weights=dv(loff), correct_Rs=dv(cr), return_transl=True, normals=dv(normals[None]))
    assert smpl_src.shape == (1, P, 3) and bw.shape == (1, P, NJ) and tf.shape == (1, P, 3, 3) and transl.shape == (1, P, 3)
    ids = torch.from_numpy(oracle.nearest_vertex(query, t_vertices).astype(np.int64))
    w64, tf64, wn64, tr64, bw64 = _coarse64(smpl64, c64(query), {k: c64(v) for k, v in params_np.items()},
                                            {k: c64(v) for k, v in t_np.items()}, c64(t_vertices), ids, lbs_weights=c64(loff[0]),
                                            correct_Rs=c64(cr), normals=c64(normals))
    for name, got, want in (("world", world, w64), ("transforms", tf, tf64), ("translation", transl, tr64), ("normals", wn, wn64),
                            ("bweights", bw, bw64)):
        util.assert_close(name, got[0].cpu().numpy(), want.numpy(), tol=1e-4)


# ------------------------------------------------------------------------------------------------------------ 6./7. render()
def _smplx_scene(P=4000, W=160, H=128, seed=0):
    from mygauhuman_amd import human_synth
    model, body = human_synth.build(P, seed=seed, motion=True, body="smplx")
    cam = human_synth.view_camera(body, W, H, view=1)
    return model, body, cam


def test_render_smplx_end_to_end(oracle):
    from mygauhuman_amd import lbs
    from mygauhuman_amd.gaussian_renderer import render
    model, body, cam = _smplx_scene()
    assert model.pose_decoder(cam.smpl_param["poses"][:, 3:])["Rs"].shape == (1, NJ - 1, 3, 3)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = util.to_dev(np.array([0.1, 0.2, 0.3], np.float32))
    W, H = cam.cam_np["W"], cam.cam_np["H"]
    w_img = torch.rand((3, H, W), device="cuda")
    out = render(1, cam, model, pipe, bg)
    assert out["render"].shape == (3, H, W) and bool(torch.isfinite(out["render"]).all()) and float(out["render_alpha"].max()) > 0.1
    assert out["correct_Rs"].shape == (1, NJ - 1, 3, 3)
    # the image against render() given the transforms of the float64 deform (its cached-transforms branch)
    with torch.no_grad():
        xyz = model.get_xyz
        cr = model.pose_decoder(cam.smpl_param["poses"][:, 3:])["Rs"]
        lw = model.lweight_offset_decoder(xyz[None]).permute(0, 2, 1)
    from mygauhuman_amd import human_synth
    smpl64 = _smpl_dict(dict(body, kintree_table=human_synth.kintree_table("smplx")), "cpu", torch.float64)
    c64 = lambda t: t.detach().double().cpu()  # noqa: E731
    tv = cam.big_pose_world_vertex.reshape(-1, 3)
    ids = torch.from_numpy(oracle.nearest_vertex(xyz.detach().cpu().numpy(), tv.cpu().numpy()).astype(np.int64))
    _, tf64, _, tr64, _ = _coarse64(smpl64, c64(xyz), {k: c64(v) for k, v in cam.smpl_param.items()},
                                    {k: c64(v) for k, v in cam.big_pose_smpl_param.items()}, c64(tv), ids, lbs_weights=c64(lw[0]),
                                    correct_Rs=c64(cr))
    ref = render(1, cam, model, pipe, bg, transforms=tf64.float().cuda(), translation=tr64.float().cuda())
    dimg = (out["render"] - ref["render"]).abs()
    assert float(dimg.mean()) < 2e-5 and float((dimg > 2e-3).float().mean()) < 1e-3, float(dimg.max())
    # backward: the pose refiner's gradient through the HIP chain equals the one through the torch chain
    grads = {}
    hip_chain = lbs.smpl_pose_transforms
    for chain in ("hip", "torch"):
        lbs.smpl_pose_transforms = hip_chain if chain == "hip" else smpl_pose_transforms_torch
        try:
            for p in model.parameters():
                p.grad = None
            model.pose_decoder.zero_grad(set_to_none=True)
            model.lweight_offset_decoder.zero_grad(set_to_none=True)
            o = render(1, cam, model, pipe, bg)
            ((o["render"] * w_img).sum() + o["normal"].mean()).backward()
            grads[chain] = [p.grad.clone() for p in (model.pose_decoder.w1, model.pose_decoder.w2, model.lweight_offset_decoder.A)]
            grads[chain + "_xyz"] = model._xyz.grad.clone()
        finally:
            lbs.smpl_pose_transforms = hip_chain
    for a, b_ in zip(grads["hip"], grads["torch"]):
        scale = float(b_.abs().max())
        assert scale > 0 and float((a - b_).abs().max()) < 2e-3 * scale, (float((a - b_).abs().max()), scale)
    assert bool(torch.isfinite(grads["hip_xyz"]).all()) and float(grads["hip_xyz"].abs().max()) > 0


def test_render_smplx_step_as_one_graph_equals_eager():
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.graph import GraphedFrame
    model, body, cam = _smplx_scene(seed=3)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = util.to_dev(np.array([0.2, 0.3, 0.1], np.float32))
    params = list(model.parameters()) + list(model.pose_decoder.parameters()) + list(model.lweight_offset_decoder.parameters())
    keys = ("render", "render_alpha", "normal", "render_axis")

    def step():
        o = render(1, cam, model, pipe, bg)
        sum(o[k].mean() for k in keys).backward()
        return o

    def eager():
        for p in params:
            p.grad = None
        o = step()
        return o["render"].detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

    frame = GraphedFrame(step, warmup=3, zero_grads=params)
    for trial in range(2):
        if trial == 1:
            cam.smpl_param["poses"].add_(0.05 * torch.randn_like(cam.smpl_param["poses"]))
        img_e, grads_e = eager()
        out = frame.replay()
        torch.cuda.synchronize()
        frame.check()
        assert torch.equal(out["render"].detach(), img_e), trial
        for p, ge in zip(params, grads_e):
            if ge is None:
                continue
            scale = float(ge.abs().max()) + 1e-20
            assert float((p.grad - ge).abs().max()) / scale < 2e-5, trial


# ------------------------------------------------------------------------------------------------------------ 8. J = 24 unchanged
def test_joint_count_entry_points_at_24_equal_original_ones(oracle):
    from mygauhuman_amd._lib import lib, ptr
    from tests.test_gpu_lbs import PARENTS, make_case
    c = make_case(oracle, 6890, 20000, 24, True)
    d = util.to_dev
    P, V = c["query"].shape[0], c["big_verts"].shape[0]
    ins = [d(c[k]) for k in ("query", "normals")] + [d(c["big_verts"]), d(c["m"]["weights"]), d(c["loff"])] + \
          [d(c[k]) for k in ("A_big", "A_pose", "off_big", "off_shape", "off_pose", "R", "Th")]
    s = torch.cuda.current_stream().cuda_stream

    def outs():
        return [torch.empty((P,), dtype=torch.int32, device="cuda")] + [torch.empty((P, n), device="cuda") for n in (24, 3, 3, 9, 3, 3)]
    ws = torch.empty((lib.gsr_lbs_workspace_bytes(V),), dtype=torch.uint8, device="cuda")
    results = []
    for nj in (False, True):
        per = []
        for variant in ("brute", "grid", "cached"):
            o = outs()
            args = [P, V] + [ptr(t) for t in ins] + [ptr(t) for t in o]
            pre = [24] if nj else []
            if variant == "brute":
                rc = (lib.gsr_lbs_forward_nj if nj else lib.gsr_lbs_forward)(*pre, *args, s)
            elif variant == "grid":
                rc = (lib.gsr_lbs_forward_grid_nj if nj else lib.gsr_lbs_forward_grid)(*pre, *args, ptr(ws), ws.numel(), 0, s)
            else:
                nn = torch.empty((lib.gsr_lbs_nn_cache_bytes(P),), dtype=torch.uint8, device="cuda")
                f = lib.gsr_lbs_forward_cached_nj if nj else lib.gsr_lbs_forward_cached
                rc = f(*pre, *args, ptr(ws), ws.numel(), ptr(nn), nn.numel(), 0, s)
                rc |= f(*pre, *args, ptr(ws), ws.numel(), ptr(nn), nn.numel(), 1, s)
            assert rc == 0
            per.append(o)
        # backward with partials (no atomics: deterministic)
        g = [torch.randn((P, 3), generator=torch.Generator(device="cuda").manual_seed(1), device="cuda"),
             torch.randn((P, 9), generator=torch.Generator(device="cuda").manual_seed(2), device="cuda"),
             torch.randn((P, 3), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")]
        dq, dn, dl = torch.empty((P, 3), device="cuda"), torch.empty((P, 3), device="cuda"), torch.empty((P, 24), device="cuda")
        dA = torch.zeros((24, 16), device="cuda")
        part = torch.empty((lib.gsr_lbs_backward_workgroups(P), 24 * 12), device="cuda")
        bargs = [P, V, ptr(ins[0]), ptr(ins[1]), ptr(per[0][0]), ptr(ins[3]), ptr(ins[4])] + [ptr(t) for t in ins[5:11]] + \
                [ptr(t) for t in g] + [ptr(dq), ptr(dn), ptr(dl), ptr(dA), None, ptr(part)]
        assert (lib.gsr_lbs_backward_nj(24, *bargs, s) if nj else lib.gsr_lbs_backward(*bargs, s)) == 0
        per.append([dq, dn, dl, part])
        # pose chain
        par = (C.c_int * 24)(*[int(v) for v in PARENTS])
        rng = np.random.default_rng(2)
        poses, joints = d(rng.normal(0, 0.4, 72).astype(np.float32)), d(rng.normal(0, 0.3, (24, 3)).astype(np.float32))
        cr = d(np.stack([np.eye(3) + rng.normal(0, 0.05, (3, 3)) for _ in range(23)]).astype(np.float32))
        rot, A = torch.empty((24, 9), device="cuda"), torch.empty((24, 16), device="cuda")
        gA, gR = d(rng.normal(0, 1, (24, 16)).astype(np.float32)), d(rng.normal(0, 1, (24, 9)).astype(np.float32))
        dp, dc, dj = torch.empty(72, device="cuda"), torch.empty((23, 9), device="cuda"), torch.empty((24, 3), device="cuda")
        fa = [ptr(poses), ptr(cr), ptr(joints), par, ptr(rot), ptr(A), s]
        ba = [ptr(poses), ptr(cr), ptr(joints), par, ptr(gA), ptr(gR), ptr(dp), ptr(dc), ptr(dj), s]
        if nj:
            assert lib.gsr_body_pose_forward(24, *fa) == 0 and lib.gsr_body_pose_backward(24, *ba) == 0
        else:
            assert lib.gsr_smpl_pose_forward(*fa) == 0 and lib.gsr_smpl_pose_backward(*ba) == 0
        per.append([rot, A, dp, dc, dj])
        results.append(per)
    torch.cuda.synchronize()
    for group_old, group_new in zip(*results):
        for a, b in zip(group_old, group_new):
            assert torch.equal(a, b)
