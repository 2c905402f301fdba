"""Tuning knob "blend_sort": the plain four-wave blend forward sorts the short lists (<= 512 entries) of its own tile instead of a
binning launch doing it.  Keys are unique (they contain the Gaussian id), so the lists, the sorted keys and everything computed from
them must be bit-identical to the binning's sort (blend_sort = 0)."""
import math

import numpy as np
import pytest
import torch

from mygauhuman_amd import synthetic
from tests import util

pytestmark = pytest.mark.gpu

# per-tile list lengths of the 4 x 4-tile frame below: both sides of every run boundary, of the forward's limit (512) and of the
# long-list sort's LDS capacity (2048); the 2100-entry list is also far above the frame's mean, so the frame is cut into segments
LENGTHS = [0, 1, 63, 64, 65, 320, 512, 513, 2100, 7, 128, 129, 200, 448, 384, 0]


@pytest.fixture
def knobs():
    from mygauhuman_amd import _lib
    _lib.set_tuning("deterministic", 1)  # gradients without float atomics: comparable bit for bit
    yield lambda v: _lib.set_tuning("blend_sort", v)
    _lib.set_tuning("blend_sort", 1)
    _lib.set_tuning("deterministic", 0)


def _lengths_scene(seed=5):
    """Tiny Gaussians (a footprint of a few pixels) placed well inside chosen tiles: tile t gets exactly LENGTHS[t] instances."""
    W = H = 64
    cam, _ = synthetic.uniform_scene(1, W, H, seed=seed, sh_degree=3)
    P = sum(LENGTHS)
    g = synthetic.uniform_gaussians(P, seed, 3, log_scale_mean=math.log(0.001))
    rng = np.random.default_rng(seed)
    tile = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
    px = (tile % 4) * 16 + rng.uniform(5.0, 10.0, P)
    py = (tile // 4) * 16 + rng.uniform(5.0, 10.0, P)
    z = rng.uniform(2.5, 4.5, P)
    # identity camera, fx = fy = W / (2 tan(fov / 2)), principal point at the image centre
    tx, ty = cam["tanfovx"], cam["tanfovy"]
    x = ((2.0 * px + 1.0) / W - 1.0) * z * tx
    y = ((2.0 * py + 1.0) / H - 1.0) * z * ty
    g["means3D"] = np.stack([x, y, z], 1).astype(np.float32)
    g["opacities"] = rng.uniform(0.3, 0.9, (P, 1)).astype(np.float32)  # every instance reaches alpha >= 1/255: none is culled
    return cam, g


def _frame(cam, g, bg, mode="sh"):
    f = util.hip_forward(cam, g, bg, mode, debug=True)
    out = {k: util.hip_query(f, k) for k in ("POINT_LIST", "KEYS_SORTED", "RANGES", "N_CONTRIB", "FINAL_T")}
    # the lists fill [0, kept); the instances the exact tile cull dropped leave the rest of the R entries unwritten by any path
    kept = int(out["RANGES"].view(np.uint32).reshape(-1, 2)[:, 1].max())
    out["POINT_LIST"], out["KEYS_SORTED"] = out["POINT_LIST"][:kept], out["KEYS_SORTED"][:kept]
    out.update({k: f[k].cpu().numpy() for k in ("color", "depth", "alpha")})
    W, H = cam["W"], cam["H"]
    rng = np.random.default_rng(7)
    dc = rng.normal(0, 1, (3, H, W)).astype(np.float32)
    dd = rng.normal(0, 1, (1, H, W)).astype(np.float32)
    da = rng.normal(0, 1, (1, H, W)).astype(np.float32)
    grads = util.hip_backward(f, dc, dd, da, debug=True)
    out.update({k: v for k, v in grads.items() if v.size})
    return f["R"], out


def _assert_same(knobs, cam, g, bg, mode="sh"):
    res = {}
    for v in (0, 1):
        knobs(v)
        res[v] = _frame(cam, g, bg, mode)
    assert res[0][0] == res[1][0]
    for k, want in res[0][1].items():
        np.testing.assert_array_equal(res[1][1][k], want, err_msg=k)
    return res[1][1]


def test_list_lengths_around_every_boundary(knobs):
    cam, g = _lengths_scene()
    out = _assert_same(knobs, cam, g, np.array([0.1, 0.4, 0.2], np.float32))
    r = out["RANGES"].view(np.uint32).reshape(-1, 2).astype(np.int64)
    assert (r[:, 1] - r[:, 0]).tolist() == LENGTHS


def test_segmented_frame(knobs):
    from tests.test_gpu_segments import _clustered_scene, _order
    cam, g = _clustered_scene(7000, 160, 128, seed=31)
    bg = np.array([0.2, 0.5, 0.7], np.float32)
    _assert_same(knobs, cam, g, bg, "precomp")
    f = util.hip_forward(cam, g, bg, "precomp")
    _, _, entries = _order(f, 80)
    assert ((entries >> 25) & 7).max() >= 1  # some list really was walked in segments


@pytest.mark.parametrize("P,scale", [(200_000, 0.01), (500_000, 0.005)], ids=["C3", "C5"])
def test_bench_scenes(knobs, P, scale):
    cam, g = synthetic.uniform_scene(P, 1024, 1024, seed=0, sh_degree=3, log_scale_mean=math.log(scale))
    _assert_same(knobs, cam, g, np.array([0.0, 0.0, 0.0], np.float32))


def _session_inputs(P, W, H, seed):
    cam, g = util.make_scene(P, W, H, seed, 3)
    params = dict(means3D=util.to_dev(g["means3D"]), shs=util.to_dev(g["shs"]), opacities=util.to_dev(g["opacities"]),
                  scales=util.to_dev(g["scales"]), rotations=util.to_dev(g["rotations"]))
    camd = dict(cam, viewmatrix=util.to_dev(cam["viewmatrix"]), projmatrix=util.to_dev(cam["projmatrix"]),
                campos=util.to_dev(cam["campos"]))
    return params, camd, util.to_dev(np.array([0.2, 0.1, 0.4], np.float32))


def test_async_session_and_capacity_overflow(knobs):
    from mygauhuman_amd.fastpath import RasterSession
    P, W, H = 6000, 144, 80
    params, camd, bg = _session_inputs(P, W, H, 8)
    cols = {}
    for v in (0, 1):
        knobs(v)
        s = RasterSession(P, W, H, 16, "cuda", capacity=200_000)
        cols[v] = s.forward(params, camd, bg, 3)[0].clone()
        assert not s.overflowed()
        R = s.num_rendered()
        small = RasterSession(P, W, H, 16, "cuda", capacity=max(1, R // 3))
        col = small.forward(params, camd, bg, 3)[0]
        assert small.overflowed() and small.num_rendered() == R
        np.testing.assert_array_equal(col.cpu().numpy(), np.broadcast_to(bg.cpu().numpy()[:, None, None], (3, H, W)))
    assert torch.equal(cols[0], cols[1])


def test_graphed_forward_replay(knobs):
    from mygauhuman_amd.fastpath import RasterSession
    from mygauhuman_amd.graph import GraphedFrame
    P, W, H = 6000, 144, 80
    params, camd, bg = _session_inputs(P, W, H, 9)
    out = {}
    for v in (0, 1):
        knobs(v)
        s = RasterSession(P, W, H, 16, "cuda", capacity=200_000)
        frame = GraphedFrame(lambda: s.forward(params, camd, bg, 3)[0], warmup=2)
        frame.replay()
        torch.cuda.synchronize()
        frame.check()
        out[v] = frame.result.clone()
    assert torch.equal(out[0], out[1])
