"""csrc/lbs.hip and csrc/pose.hip against the float64 CPU restatements of the chain they replace (tests/deform_reference.py), at
the sizes where the kernels branch, on the edges of their inputs, with guard bands around everything the bindings allocate.

The bound is measured: for every tensor the float32 CPU evaluation of the same restatement is compared with the float64 one by
the measure of util.assert_close (e32, computed inside the test on the same inputs), and the kernel must stay within
2 x e32 + 4 float32 ulps of the tensor's scale; no bound may exceed the 1e-4 of the fixed-tolerance tests.  The two gradients the
backward reduces over the points, d_A_pose and d_off_pose, are measured against S_abs, the sum of the absolute per-point
contributions of an element, and their float32 checker adds the contributions one after the other in float32.  Every element of
every tensor is compared: the only discontinuity, the nearest-vertex choice, is an INPUT of the reference (the ids of the exact
float32 search, oracle.nearest_vertex), and the ids themselves are compared exactly.  The cases and what they promise:
tests/deform_cases.py, asserted without a GPU in tests/test_deform_reference_host.py.

Measured on one MI355X, by that measure.  Per tensor, worst over the cases: e32 = the float32 checker against float64, kernel =
the kernel against float64, k/e32 = the worst ratio of the two within one case, /bound = the worst share of the bound used:

    LBS (all cases but one)    e32      kernel   k/e32  /bound     case "illcond"             e32      kernel   k/e32  /bound
    world_pts                  1.8e-07  1.9e-07  2.40   0.23       world_pts                  2.9e-06  4.8e-06  1.91   0.87
    transforms                 5.8e-07  5.3e-07  1.86   0.43       transforms                 4.4e-06  7.3e-06  2.02   0.94
    world_normals              3.9e-07  4.7e-07  1.81   0.47       world_normals              2.7e-06  4.4e-06  1.79   0.82
    smpl_pts                   6.3e-07  5.7e-07  1.97   0.42       smpl_pts                   4.0e-06  5.0e-06  1.49   0.68
    bweights                   2.3e-07  5.6e-07  3.54   0.65       bweights                   1.7e-07  1.8e-07  1.10   0.22
    translation                1.1e-07  1.1e-07  1.50   0.17       translation                5.1e-06  8.0e-06  2.04   0.94
    d_query                    6.2e-07  5.5e-07  3.89   0.47       d_query (factor 3)         3.8e-06  8.6e-06  2.25   0.72
    d_normals                  3.8e-07  3.8e-07  1.91   0.35       d_normals                  3.1e-06  3.7e-06  1.19   0.55
    d_lbs_offsets              6.9e-07  8.4e-07  1.93   0.54       d_lbs_offsets (factor 4)   6.6e-06  1.1e-05  3.16   0.76
    d_A_pose (S_abs)           2.7e-06  2.5e-06  1.85   0.53       d_A_pose (S_abs)           3.8e-07  5.4e-07  1.54   0.46
    d_off_pose (S_abs)         8.6e-07  8.9e-07  4.24   0.46       d_off_pose (S_abs)         3.3e-07  3.3e-07  1.00   0.29

    pose chain                 e32      kernel   k/e32  /bound
    A                          8.6e-07  1.2e-06  2.50   0.67       d_joints                   7.9e-07  9.4e-07  7.65   0.95
    rot_mats                   4.2e-07  4.8e-07  1.41   0.41       d_joints (zero pose)       1.0e-06  6.0e-07  0.58   0.24
    rot_mats (zero pose)       0        0        -      0          d_correct_Rs               1.0e-06  1.6e-06  2.41   0.89
    d_poses                    1.0e-06  1.3e-06  3.09   0.75       A, 64-deep chain near pi (factor 4)  4.9e-07  1.5e-06  4.02  0.76

Three tensors have a factor above two -- the ones that measurably exceeded the default bound, each at the smallest whole factor
that holds, with the reason and a host test that reproduces the excess next to the constant (ILLCOND_FACTORS,
DEEP_CHAIN_NEAR_PI_A_FACTOR below); every other tensor is held to two.  Where k/e32 exceeds two elsewhere, the checker's own error in
that case is below two ulps and the kernel's is within the 4-ulp floor (d_joints at 0.95 of its bound: e32 = 2e-08).
Temporal cache, frame 2: 9 misses with 4 zero-radius entries (J = 24), 8 with 3 (J = 55).
"""
import numpy as np
import pytest
import torch

from tests import deform_cases as dc
from tests import deform_reference as dr
from tests.test_gpu_guardband import GuardedTorch

pytestmark = pytest.mark.gpu

DEV = "cuda"
RECORD = {}
VARIANTS = (("brute", False), ("grid", False), ("grid", True))
PER_POINT = ("query", "normals", "loff")


@pytest.fixture(autouse=True)
def guarded(monkeypatch):
    """4 KB margins around every tensor lbs.py and knn_cuda.py allocate, checked when the test is over."""
    from mygauhuman_amd import knn_cuda, lbs
    g = GuardedTorch()
    monkeypatch.setattr(lbs, "torch", g)
    monkeypatch.setattr(knn_cuda, "torch", g)
    yield g
    g.check("deform bindings")


@pytest.fixture(scope="module", autouse=True)
def _table():
    """Worst figures per tensor over the cases that ran (the table of the module docstring is one run's output of this)."""
    yield
    print("\n    tensor                     e32      kernel   k/e32  /bound")
    for name, rows in RECORD.items():
        e32, ek = max(r[0] for r in rows), max(r[1] for r in rows)
        ratio = max((r[1] / r[0] for r in rows if r[0] > 0), default=float("nan"))
        share = max(r[1] / r[2] for r in rows)
        print(f"    {name:26s} {e32:8.1e} {ek:8.1e} {ratio:6.2f} {share:6.2f}")
    from mygauhuman_amd import lbs
    torch.cuda.synchronize()
    lbs._GRIDS.entries.clear()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_lbs(c, search="grid", cached=True, lean=False, requires=(), loss=None, query=None, verts=None):
    """One forward (and, with a loss, one backward) through lbs.lbs_deform.  Returns (outputs, ids, grads): numpy; grads[k] is None
    for an input that got no gradient.  The inputs handed over are compared with clones afterwards."""
    from mygauhuman_amd import lbs
    t = {k: _dev(c[k]) for k in dr.LBS_INPUTS}
    if query is not None:
        t["query"] = _dev(query)
    for k in requires:
        t[k].requires_grad_(True)
    verts_t, w = (_dev(c["verts"]) if verts is None else verts), _dev(c["weights"])
    saved = {k: v.detach().clone() for k, v in t.items() if v is not None}
    saved.update(verts=verts_t.clone(), weights=w.clone())
    old = (lbs.NEAREST_VERTEX_SEARCH, lbs.NN_TEMPORAL_CACHE)
    lbs.NEAREST_VERTEX_SEARCH, lbs.NN_TEMPORAL_CACHE = search, cached
    try:
        o = lbs.lbs_deform(*[t[k] for k in dr.LBS_INPUTS], verts_t, w, lean=lean)
    finally:
        lbs.NEAREST_VERTEX_SEARCH, lbs.NN_TEMPORAL_CACHE = old
    grads = None
    if loss is not None:
        terms = [(o[n] * _dev(c[dr.UPSTREAM[n]])).sum() for n in dr.LOSS_TERMS[loss] if o[n] is not None]
        total = sum(terms[1:], terms[0])
        if total.requires_grad:
            total.backward()
        grads = {k: (None if t[k].grad is None else t[k].grad.cpu().numpy()) for k in dr.LBS_GRADS if t[k] is not None}
    torch.cuda.synchronize()
    for k, v in saved.items():
        now = verts_t if k == "verts" else w if k == "weights" else t[k].detach()
        assert torch.equal(now.view(torch.int32), v.view(torch.int32)), f"input {k} was written to"
    outs = {k: (None if o[k] is None else o[k].detach().cpu().numpy()) for k in dr.LBS_OUTPUTS}
    return outs, o["vert_ids"].cpu().numpy(), grads


# Factors above two, per tensor: only the tensors that measurably exceeded 2 x e32 + 4 ulp, at the smallest whole factor that holds.
# Case "illcond" (blended big-pose rotation of condition 50 .. 60): d_lbs_offsets measured 3.16 x e32 (J = 24), d_query 2.25 x e32
# (J = 55: 8.6e-06 against a bound of 8.1e-06).  The operation: the ROUNDING OF THE BLEND WEIGHTS -- logf, expf and a division, each
# good to an ulp on the device as in torch, but not the same ulp -- times that condition number.  Re-rounding the float32 checker's
# blend weights by at most two ulps moves its own error in these two tensors by more than the measured excess
# (test_deform_reference_host.py::test_illcond_noise_is_the_rounding_of_the_blend_weights).  Every other tensor of the case stayed
# within the default bound and keeps it.
ILLCOND_FACTORS = {"d_loff": 4.0, "d_query": 3.0}


def check_forward(outs, ids, ref, lean=False, tag="", factors=None):
    factors = factors or {}
    ref_ids, (o64, _, _), (o32, _, _) = ref
    assert ids.dtype == np.int32 and np.array_equal(ids, ref_ids), "vertex ids differ from the exact float32 search"
    for k in dr.LBS_OUTPUTS:
        if lean and k in ("smpl_pts", "bweights", "translation"):
            assert outs[k].size == 0
        elif o64[k] is None:
            assert outs[k] is None
        else:
            assert outs[k].shape == o64[k].shape and outs[k].dtype == np.float32, k
            dr.check_measured(k + tag, outs[k], o64[k], o32[k], RECORD, factors.get(k, dr.FACTOR))


def check_backward(grads, ref, names, tag="", factors=None):
    factors = factors or {}
    _, (_, g64, s_abs), (_, g32, _) = ref
    for k in names:
        assert grads[k] is not None and grads[k].shape == g64[k].shape and grads[k].dtype == np.float32, k
        if k in PER_POINT:
            dr.check_measured("d_" + k + tag, grads[k], g64[k], g32[k], RECORD, factors.get("d_" + k, dr.FACTOR))
        else:
            dr.check_reduced("d_" + k + tag, grads[k], g64[k], g32[k], s_abs[k], RECORD, factors.get("d_" + k, dr.FACTOR))
    if "A_pose" in names:
        assert not grads["A_pose"][:, 3].any(), "row 3 of every A is constant: its gradient is exactly zero"


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _inputs_with_grad(c):
    return tuple(k for k in dr.LBS_GRADS if c[k] is not None)


# ------------------------------------------------------------------------------------------------------ every case, all gradients
@pytest.mark.parametrize("J", dc.JOINTS)
@pytest.mark.parametrize("name", sorted(dc.LBS_CASES))
def test_lbs_forward_and_backward_match_float64(oracle, name, J):
    """P in {0, 1, 63, 64, 65, 255, 256, 257, 513}; normals / offsets present and absent; sparse, one-hot, saturated, equal-offset
    and single-joint weights; the ill-conditioned blend; V = 1 and the clustered query (all points into three rows of d_off_pose):
    the six outputs, the ids and the five gradients, default search path."""
    c = dc.lbs_case(name, J)
    ref = dc.reference(oracle, c, (name, J))
    names = _inputs_with_grad(c)
    outs, ids, grads = run_lbs(c, requires=names, loss="all")
    P, V = c["query"].shape[0], c["verts"].shape[0]
    assert outs["world_pts"].shape == (P, 3) and outs["transforms"].shape == (P, 3, 3) and outs["bweights"].shape == (P, J)
    tag, factors = (" [illcond]", ILLCOND_FACTORS) if name == "illcond" else ("", None)
    check_forward(outs, ids, ref, tag=tag, factors=factors)
    check_backward(grads, ref, names, tag=tag, factors=factors)
    assert all(np.isfinite(g).all() for g in grads.values())
    if P == 0:
        assert grads["A_pose"].shape == (J, 4, 4) and not grads["A_pose"].any() and grads["off_pose"].shape == (V, 3) and not grads["off_pose"].any()
    if name == "equal_offsets":   # softmax(log(w + 1e-9) + c) = the plain weights (to 1e-9 J)
        dr.check_measured("bweights (equal offsets)", outs["bweights"], c["weights"][ids].astype(np.float64), ref[2][0]["bweights"], RECORD)
    if name == "saturated":
        sat = np.abs(grads["loff"][0::2]).max()
        assert sat < 1e-2 * np.abs(grads["loff"][1::2]).max(), sat


# ------------------------------------------------------------------------------------------------------ vertex-count tails
@pytest.mark.parametrize("J", dc.JOINTS)
@pytest.mark.parametrize("V", dc.V_TAILS)
def test_vertex_count_tails_three_searches_identical(oracle, J, V):
    """V in {1, 2, 1023, 1024, 1025, 2049} (VTILE = 1024): winners in the last slot, in the first slot of the second tile, and ties
    across the tile boundary that the lower index wins; brute force, grid and grid + temporal cache bit for bit the same.  The
    cached variant keeps one vertex tensor: its first frame makes the entries, a second frame with every coordinate moved by one
    ulp goes through the cache-update kernel (the tie rows have radius 0 and are searched again)."""
    from mygauhuman_amd import lbs
    c = dc.vtail_case(J, V)
    ref = dc.reference(oracle, c, ("vtail", J, V))
    names = _inputs_with_grad(c)
    verts = _dev(c["verts"])
    runs = {v: run_lbs(c, *v, requires=names, loss="all", verts=verts if v[1] else None) for v in VARIANTS}
    outs, ids, grads = runs[VARIANTS[0]]
    check_forward(outs, ids, ref)
    check_backward(grads, ref, names)
    pl = c["planted"]
    assert (ids[pl["last"]] == V - 1).all() and (ids[pl["first_of_tile"]] == 1024).all() and (ids[pl["tie"]] == 1023).all()
    for v in VARIANTS[1:]:
        o, i, g = runs[v]
        assert np.array_equal(i, ids), v
        for k in dr.LBS_OUTPUTS:
            assert _bits(o[k], outs[k]), (v, k)
        for k in PER_POINT + ("A_pose",):
            assert _bits(g[k], grads[k]), (v, k)
    moved = np.nextafter(c["query"], np.float32(np.inf))
    got = run_lbs(c, "grid", True, verts=verts, query=moved)
    misses, _ = lbs._GRIDS.nn_cache_stats(verts, 257)
    want = run_lbs(c, "brute", False, query=moved)
    assert np.array_equal(got[1], oracle.nearest_vertex(moved, c["verts"])) and np.array_equal(got[1], want[1])
    for k in dr.LBS_OUTPUTS:
        assert _bits(got[0][k], want[0][k]), k
    assert len(pl["tie"]) <= misses <= 257, misses
    if V > 1:
        assert misses < 257, "with more than one vertex most entries have a radius far above one ulp"


# ------------------------------------------------------------------------------------------------------ temporal cache
@pytest.mark.parametrize("J", dc.JOINTS)
def test_temporal_cache_at_wave_granularity(oracle, J):
    """Frame 2 moves exactly the points {0, 63, 64, 255, 256} (first and last lane of a wave, of a workgroup, the one-point last
    workgroup) out of their entries: ids and outputs as without the cache, and exactly those -- plus the zero-radius entries --
    are searched."""
    from mygauhuman_amd import lbs
    c = dc.cache_case(J)
    verts = _dev(c["verts"])
    first = run_lbs(c, "grid", True, verts=verts)
    assert np.array_equal(first[1], oracle.nearest_vertex(c["query"], c["verts"]))
    got = run_lbs(c, "grid", True, verts=verts, query=c["query2"])
    misses, _ = lbs._GRIDS.nn_cache_stats(verts, 257)
    want = run_lbs(c, "grid", False, verts=verts, query=c["query2"])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[1], oracle.nearest_vertex(c["query2"], c["verts"]))
    assert (got[1][list(dc.CACHE_MOVED)] != first[1][list(dc.CACHE_MOVED)]).all(), "the moved points must change their vertex"
    for k in dr.LBS_OUTPUTS:
        assert _bits(got[0][k], want[0][k]), k
    still = np.ones(257, bool)
    still[list(dc.CACHE_MOVED)] = False
    n_zero = int((dc.cache_radii(c)[0][still] == 0).sum())
    print(f"misses {misses}, zero-radius entries among the unmoved points {n_zero}")
    assert 5 <= misses <= 5 + n_zero, (misses, n_zero)


# ------------------------------------------------------------------------------------------------------ lean / normals / offsets
@pytest.mark.parametrize("J", dc.JOINTS)
@pytest.mark.parametrize("with_normals,with_offsets", sorted(dc.SWITCH_CASES))
def test_lean_forward_and_backward_equal_the_full_ones(oracle, J, with_normals, with_offsets):
    """lean=True (what render() uses) skips three stores: its three outputs and the backward after it have the bits of the full
    run (d_A_pose comes from per-workgroup partials: deterministic); d_off_pose, float atomics, is held to the bound."""
    name = dc.SWITCH_CASES[(with_normals, with_offsets)]
    c = dc.lbs_case(name, J)
    ref = dc.reference(oracle, c, (name, J))
    names = _inputs_with_grad(c)
    assert ("normals" in names) == with_normals and ("loff" in names) == with_offsets
    full = run_lbs(c, requires=names, loss="all")
    again = run_lbs(c, requires=names, loss="all")
    lean = run_lbs(c, lean=True, requires=names, loss="all")
    check_forward(lean[0], lean[1], ref, lean=True)
    check_backward(lean[2], ref, names)
    assert (lean[0]["world_normals"] is None) == (not with_normals)
    for k in ("world_pts", "transforms") + (("world_normals",) if with_normals else ()):
        assert _bits(lean[0][k], full[0][k]), k
    for k in names:
        if k != "off_pose":
            assert _bits(lean[2][k], full[2][k]), k
    assert _bits(again[2]["A_pose"], full[2]["A_pose"])


# ------------------------------------------------------------------------------------------------------ gradient routing
REQUIRES = [(k,) for k in dr.LBS_GRADS] + [dr.LBS_GRADS, ("query", "normals", "loff", "A_pose"), ("query", "normals", "loff", "off_pose")]


@pytest.mark.parametrize("J", dc.JOINTS)
@pytest.mark.parametrize("loss", sorted(dr.LOSS_TERMS))
def test_gradient_routing(oracle, J, loss):
    """Each input requiring grad alone, all five, A_pose without off_pose and the reverse (need_A / need_off switch the LDS product
    and the atomics), under a loss on the world points, the transforms, the world normals alone and on all three: what is produced
    is within the bound, what was not asked for is None."""
    c = dc.lbs_case("P257", J)
    ref = dc.reference(oracle, c, ("P257", J), loss)
    for requires in REQUIRES:
        for lean in (False, True):
            _, _, grads = run_lbs(c, lean=lean, requires=requires, loss=loss)
            check_backward(grads, ref, requires)
            for k in dr.LBS_GRADS:
                assert (grads[k] is None) == (k not in requires), (requires, k)


# ------------------------------------------------------------------------------------------------------ non-finite points
@pytest.mark.parametrize("J", dc.JOINTS)
def test_nonfinite_points_take_vertex_zero_and_disturb_nothing(oracle, J):
    """Rows 0 / 100 / 256 of query are NaN / +inf / 3e19 (squared distance overflows): no distance compares below the initial
    best, so all three searches return vertex 0 for them -- an index inside the tables -- and every other row has the bits of the
    run in which those rows are ordinary points."""
    from mygauhuman_amd import knn_cuda, lbs
    bad, fin = dc.nonfinite_case(J)
    rows = sorted(dc.NONFINITE_ROWS)
    rest = np.ones(257, bool)
    rest[rows] = False
    V = bad["verts"].shape[0]
    ref = dc.reference(oracle, fin, ("P257", J))
    base = run_lbs(fin, "brute", False)
    verts = _dev(bad["verts"])
    ids_brute = None
    for search, cached, frames in (("brute", False, 1), ("grid", False, 1), ("grid", True, 2)):
        for frame in range(frames):   # the second cached frame goes through the cache-update kernel
            outs, ids, _ = run_lbs(bad, search, cached, verts=verts if cached else None)
            assert ((ids >= 0) & (ids < V)).all(), (search, cached, frame, ids[rows])
            ids_brute = ids if ids_brute is None else ids_brute
            assert np.array_equal(ids, ids_brute) and (ids[rows] == 0).all() and np.array_equal(ids[rest], ref[0][rest])
            for k in dr.LBS_OUTPUTS:
                assert _bits(outs[k][rest], base[0][k][rest]), (search, cached, frame, k)
    # the rows made finite again are searched again
    outs, ids, _ = run_lbs(fin, "grid", True, verts=verts)
    assert np.array_equal(ids, ref[0])
    for k in dr.LBS_OUTPUTS:
        assert _bits(outs[k], base[0][k]), k
    # the stand-alone query
    dist, idx = knn_cuda.knn_nearest(verts, _dev(bad["query"]))
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert ((idx >= 0) & (idx < V)).all() and np.array_equal(idx, ids_brute)
    assert (dist[rows] == np.sqrt(np.float32(np.finfo(np.float32).max))).all() and np.isfinite(dist[rest]).all(), dist[rows]
    _, idx3 = knn_cuda.KNN(k=1, transpose_mode=True)(verts[None], _dev(bad["query"])[None])
    assert np.array_equal(idx3[0, :, 0].cpu().numpy(), ids_brute)
    # backward: the per-point gradients of the other rows (the reduced ones take the NaN of the three rows, as the reference's do)
    _, _, grads = run_lbs(bad, requires=dr.LBS_GRADS, loss="all")
    _, (_, g64, _), (_, g32, _) = ref
    for k in PER_POINT:
        dr.check_measured("d_" + k, grads[k][rest], g64[k][rest], g32[k][rest], RECORD)
    assert lbs.NEAREST_VERTEX_SEARCH == "grid" and lbs.NN_TEMPORAL_CACHE is True   # what the runs above call the default path


# ------------------------------------------------------------------------------------------------------ pose chain
# One tensor of one pose case has a factor above two: A of the 64-deep chain at angles around pi measured 4.02 x e32 (1.5e-06
# against 3.8e-07); every other tensor of every tree and kind stayed within the default bound.  The operation: 64 chained 3x4
# products amplify which way each one was rounded.  The float32 checker's own error there moves by more than a factor of two when
# its rot_mats are re-rounded by half an ulp or the products are summed in the kernel's order
# (test_deform_reference_host.py::test_deep_chain_noise_floor_moves_with_half_an_ulp): e32 is one sample of that noise.
DEEP_CHAIN_NEAR_PI_A_FACTOR = 4.0


def _subtree_abs(c, loss):
    """S_abs of d_joints where the reference is exactly zero (all rotations the identity): d_joints[i] is the sum over i's subtree
    of the incoming dL/dA translation columns minus the same terms again."""
    J, S = c["J"], np.zeros((c["J"], 3))
    if loss != "rot":
        S[:] = np.abs(c["wA"][:, :3, 3].astype(np.float64))
        for i in range(J - 1, 0, -1):
            S[c["parents"][i]] += S[i]
    return S


def _run_pose(c, with_correct, loss, requires):
    from mygauhuman_amd import lbs
    poses, joints = _dev(c["poses"].reshape(1, -1)), _dev(c["joints"])
    cr = _dev(c["correct_Rs"]) if with_correct else None
    t = dict(poses=poses, joints=joints, correct_Rs=cr)
    for k in requires:
        t[k].requires_grad_(True)
    saved = {k: v.detach().clone() for k, v in t.items() if v is not None}
    rot, A = lbs._SmplPose.apply(poses, cr, joints, tuple(c["parents"]))
    total = 0.0
    if loss in ("A", "both"):
        total = total + (A * _dev(c["wA"])).sum()
    if loss in ("rot", "both"):
        total = total + (rot * _dev(c["wR"])).sum()
    total.backward()
    torch.cuda.synchronize()
    for k, v in saved.items():
        assert torch.equal(t[k].detach(), v), k
    n = lambda x: None if x is None else x.detach().cpu().numpy()  # noqa: E731
    J = c["J"]
    return dict(A=n(A), rot_mats=n(rot), d_poses=None if poses.grad is None else n(poses.grad).reshape(J, 3), d_joints=n(joints.grad),
                d_correct_Rs=None if cr is None else n(cr.grad))


@pytest.mark.parametrize("tree,J", dc.POSE_TREES)
@pytest.mark.parametrize("kind", dc.POSE_KINDS)
def test_pose_chain_matches_float64(tree, J, kind):
    """J in {2, 24, 55, 64}: SMPL and SMPL-X trees, a 64-deep chain, a 64-wide star; the all-zero pose, the big pose (exact zeros),
    magnitudes 1e-7 and 1e-4, single-axis vectors, angles around pi and near 2 pi, N(0, 0.4); with and without general (not
    orthogonal) correct_Rs; a loss on A, on rot_mats, on both; every input requiring grad alone and all together."""
    c = dc.pose_case(tree, J, kind)
    deep = tree == "chain" and kind == "near_pi"
    a_tag, a_factor = (" [64-deep, near pi]", DEEP_CHAIN_NEAR_PI_A_FACTOR) if deep else ("", dr.FACTOR)
    for with_correct in (False, True):
        inputs = ("poses", "joints") + (("correct_Rs",) if with_correct else ())
        for loss in ("A", "rot", "both"):
            r64, r32 = dc.pose_reference(tree, J, kind, with_correct, loss)
            for requires in [(k,) for k in inputs] + [inputs]:
                got = _run_pose(c, with_correct, loss, requires)
                assert np.array_equal(got["A"][:, 3], np.tile(np.float32([0, 0, 0, 1]), (J, 1)))
                dr.check_measured("pose A" + a_tag, got["A"], r64["A"], r32["A"], RECORD, a_factor)
                dr.check_measured("pose rot_mats", got["rot_mats"], r64["rot_mats"], r32["rot_mats"], RECORD)
                for k in ("poses", "joints", "correct_Rs"):
                    g = got["d_" + k]
                    assert (g is None) == (k not in requires), (requires, k)
                    if g is not None:
                        assert np.isfinite(g).all(), k
                        if k == "joints" and kind == "zero" and (not with_correct or tree == "star"):
                            # zero by cancellation, everywhere (no correct_Rs) or at the root of the star (two 63-term sums of
                            # the children's terms, whose rotations are then one correct_Rs each, of norm <= 1.5): such an
                            # element is accurate to the sum of the absolute terms, not to the tensor's scale
                            S = _subtree_abs(c, loss) * (1.5 if with_correct else 1.0)
                            dr.check_reduced("pose d_joints (zero pose)", g, r64["d_" + k], r32["d_" + k], S, RECORD)
                        else:
                            dr.check_measured("pose d_" + k, g, r64["d_" + k], r32["d_" + k], RECORD)
                if kind == "zero" and not with_correct:
                    dr.check_measured("pose rot_mats (zero pose)", got["rot_mats"], np.tile(np.eye(3), (J, 1, 1)), r32["rot_mats"], RECORD)


def test_pose_joint_count_limits():
    """One lane per joint: J = 1 and J = 65 are refused, J = 2 and J = 64 run (above)."""
    from mygauhuman_amd import lbs
    from mygauhuman_amd._lib import GsrError
    for J in (1, 65):
        with pytest.raises((GsrError, RuntimeError)):
            lbs._SmplPose.apply(torch.zeros(1, 3 * J, device=DEV), None, torch.zeros(J, 3, device=DEV), (-1,) + tuple(range(J - 1)))
