"""CPU-only tests of the fused Adam step (mygauhuman_amd.optim, csrc/adam.hip): the C ABI is declared, exported and validates its
arguments before any HIP call; FusedAdam refuses what it does not implement; its state and state_dict() are laid out like
torch.optim.Adam's; the launch plan covers every element exactly once; there is no CPU path."""
import ctypes as C
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gsr_adam_step", "gsr_stats_update", "gsr_adam_chunk_floats")
# the reference's groups (scene/gaussian_model.py:256-281): name, row shape
GROUPS = (("xyz", (3,)), ("f_dc", (1, 3)), ("f_rest", (15, 3)), ("opacity", (1,)), ("scaling", (3,)), ("rotation", (4,)),
          ("normal", (3,)), ("albedo", (3,)), ("roughness", (1,)))


def _groups(P=7, device="cpu"):
    g = torch.Generator().manual_seed(0)
    return [{"params": [torch.nn.Parameter(torch.randn((P,) + shp, generator=g).to(device))], "lr": 1e-3 * (i + 1), "name": n}
            for i, (n, shp) in enumerate(GROUPS)]


def test_symbols_are_declared_and_exported():
    from mygauhuman_amd import _lib, optim
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert n in _lib.SYMBOLS and hasattr(_lib.lib, n)
    assert _lib.lib.gsr_adam_chunk_floats() == optim.CHUNK
    assert ("adam.hip", []) in __import__("mygauhuman_amd.build", fromlist=["SOURCES"]).SOURCES   # default contraction
    # the ctypes mirrors have the sizes of the C structs (8-byte pointers, natural alignment)
    assert C.sizeof(_lib.AdamArray) == 48 and C.sizeof(_lib.AdamGroup) == 32 and C.sizeof(_lib.AdamStats) == 56


def _call(n_arrays=1, arrays="own", n_groups=1, groups="own", steps=1 << 12, beta1=0.9, beta2=0.999, eps=1e-15, count=8, slot=0,
          stats=None, ptr=1 << 12):
    """gsr_adam_step with fake (never dereferenced: every call here must fail validation) device pointers."""
    from mygauhuman_amd import _lib
    arr = (_lib.AdamArray * max(1, n_arrays))()
    for k in range(n_arrays):
        arr[k] = _lib.AdamArray(ptr, ptr, ptr, ptr, count, 0, slot + k)
    grp = (_lib.AdamGroup * max(1, n_groups))()
    for k in range(n_groups):
        grp[k] = _lib.AdamGroup(beta1, beta2, 1e-3, eps, -math.inf, k)
    rc = _lib.lib.gsr_adam_step(n_arrays, arr if arrays == "own" else None, n_groups, grp if groups == "own" else None, None, steps,
                                stats, 0, None)
    return rc, _lib.lib.gsr_last_error()


def test_argument_validation_without_a_gpu():
    from mygauhuman_amd import _lib
    rc, msg = _call(arrays=None)
    assert rc == -1 and b"null" in msg
    rc, msg = _call(groups=None)
    assert rc == -1 and b"null" in msg
    rc, msg = _call(steps=None)
    assert rc == -1 and b"null" in msg
    rc, msg = _call(n_arrays=65)
    assert rc == -1 and b"at most 64 arrays" in msg
    rc, msg = _call(n_arrays=-1)
    assert rc == -1
    rc, msg = _call(n_groups=17)
    assert rc == -1 and b"16 groups" in msg
    for kw in (dict(beta1=1.0), dict(beta2=1.0), dict(beta1=-0.1), dict(beta2=float("nan"))):
        rc, msg = _call(**kw)
        assert rc == -1 and b"beta" in msg, kw
    for eps in (0.0, -1e-8, float("nan")):
        rc, msg = _call(eps=eps)
        assert rc == -1 and b"eps" in msg
    rc, msg = _call(count=-1)
    assert rc == -1 and b"count" in msg
    rc, msg = _call(ptr=None)
    assert rc == -1 and b"null pointer" in msg
    rc, msg = _call(n_arrays=2, slot=-1)          # slots -1, 0
    assert rc == -1
    arr = (_lib.AdamArray * 2)(_lib.AdamArray(16, 16, 16, 16, 4, 0, 3), _lib.AdamArray(32, 32, 32, 32, 4, 0, 3))
    grp = (_lib.AdamGroup * 1)(_lib.AdamGroup(0.9, 0.999, 1e-3, 1e-8, -math.inf, 0))
    assert _lib.lib.gsr_adam_step(2, arr, 1, grp, None, 1 << 12, None, 0, None) == -1 and b"share step slot" in _lib.lib.gsr_last_error()
    bad = _lib.AdamStats(5, 3, None, 16, 16, 16, 16, 16)
    rc, msg = _call(stats=C.byref(bad))
    assert rc == -1 and b"statistics" in msg
    assert _lib.lib.gsr_stats_update(None, 0, None) == -1 and b"null" in _lib.lib.gsr_last_error()
    assert _lib.lib.gsr_stats_update(C.byref(bad), 0, None) == -1
    assert _lib.lib.gsr_stats_update(C.byref(_lib.AdamStats(-1, 3, 16, 16, 16, 16, 16, 16)), 0, None) == -1
    assert _lib.lib.gsr_stats_update(C.byref(_lib.AdamStats(5, 1, 16, 16, 16, 16, 16, 16)), 0, None) == -1
    # nothing to do is not an error and launches nothing
    assert _lib.lib.gsr_adam_step(0, None, 0, None, None, None, None, 0, None) == 0
    assert _lib.lib.gsr_stats_update(C.byref(_lib.AdamStats(0, 3, None, None, None, None, None, None)), 0, None) == 0


def test_constructor_refusals():
    from mygauhuman_amd.optim import FusedAdam
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(ValueError):
            FusedAdam(_groups(), lr=0.0, eps=1e-15, **kw)
    with pytest.raises(ValueError):
        FusedAdam(_groups(), lr=0.0, eps=0.0)
    with pytest.raises(ValueError):
        FusedAdam(_groups(), lr=0.0, betas=(1.0, 0.999))
    opt = FusedAdam(_groups(), lr=0.0, eps=1e-15)
    assert isinstance(opt, torch.optim.Adam)
    assert [g["lr"] for g in opt.param_groups] == [1e-3 * (i + 1) for i in range(9)]


def test_state_layout_and_state_dict_keys_equal_torch_adam():
    from mygauhuman_amd.optim import FusedAdam
    ours = FusedAdam(_groups(), lr=0.0, eps=1e-15)
    assert len(ours.state) == 0                                      # lazily, as torch
    ours.init_state()
    theirs = torch.optim.Adam(_groups(), lr=0.0, eps=1e-15, fused=True)   # torch's fused layout: step a float32 0-dim tensor
    for group in theirs.param_groups:
        group["params"][0].grad = torch.zeros_like(group["params"][0])
    theirs.step()
    a, b = ours.state_dict(), theirs.state_dict()
    assert a.keys() == b.keys() and len(a["param_groups"]) == len(b["param_groups"]) == 9
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert ga.keys() == gb.keys() and ga["name"] == gb["name"] and ga["params"] == gb["params"]
        assert (ga["lr"], ga["betas"], ga["eps"], ga["weight_decay"], ga["amsgrad"]) == (gb["lr"], gb["betas"], gb["eps"], 0, False)
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in ("step", "exp_avg", "exp_avg_sq"):
            ta, tb = a["state"][k][name], b["state"][k][name]
            assert ta.dtype == tb.dtype == torch.float32 and ta.shape == tb.shape and ta.device == tb.device, (k, name)
    # the counters are views into one flat table, one slot each
    slots = [ours._slot_of(ours.state[g["params"][0]]["step"]) for g in ours.param_groups]
    assert slots == list(range(9))
    assert all(float(ours.state[g["params"][0]]["step"]) == 0.0 for g in ours.param_groups)


def test_a_state_dict_with_cpu_step_tensors_loads_and_round_trips():
    from mygauhuman_amd.optim import FusedAdam
    ref = torch.optim.Adam(_groups(), lr=0.0, eps=1e-15)     # what the reference builds: step is a CPU float tensor
    for k in range(3):
        for group in ref.param_groups:
            p = group["params"][0]
            p.grad = torch.full_like(p, 0.5 + k)
        ref.step()
    sd = ref.state_dict()
    assert sd["state"][0]["step"].device.type == "cpu" and float(sd["state"][0]["step"]) == 3.0
    ours = FusedAdam(_groups(), lr=0.0, eps=1e-15)
    ours.load_state_dict(sd)
    for i, group in enumerate(ours.param_groups):
        st = ours.state[group["params"][0]]
        assert ours._slot_of(st["step"]) == i and float(st["step"]) == 3.0 and st["step"].dtype == torch.float32
        assert torch.equal(st["exp_avg"], sd["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
        assert group["lr"] == 1e-3 * (i + 1) and group["name"] == GROUPS[i][0]
    # and back into torch.optim.Adam, which then steps (CPU: torch's own fused implementation)
    back = torch.optim.Adam(_groups(), lr=0.0, eps=1e-15)
    back.load_state_dict(ours.state_dict())
    for group in back.param_groups:
        group["params"][0].grad = torch.ones_like(group["params"][0])
    back.step()
    assert all(float(back.state[g["params"][0]]["step"]) == 4.0 for g in back.param_groups)
    # a Python-number step (old checkpoints) is adopted too
    sd2 = ref.state_dict()
    for st in sd2["state"].values():
        st["step"] = 3
    again = FusedAdam(_groups(), lr=0.0, eps=1e-15)
    again.load_state_dict(sd2)
    assert all(float(again.state[g["params"][0]]["step"]) == 3.0 for g in again.param_groups)


def test_the_step_table_grows_and_keeps_its_counters():
    from mygauhuman_amd.optim import FusedAdam
    ps = [torch.nn.Parameter(torch.zeros(2)) for _ in range(3)]
    opt = FusedAdam(ps, lr=1e-3).init_state()
    opt.state[ps[1]]["step"].fill_(7.0)
    first = opt._steps
    for _ in range(200):
        opt._new_slot()
    assert opt._steps is not first and opt._steps.numel() >= 203
    assert [float(opt.state[p]["step"]) for p in ps] == [0.0, 7.0, 0.0]
    assert [opt._slot_of(opt.state[p]["step"]) for p in ps] == [0, 1, 2]


@pytest.mark.parametrize("chunk", [4096, 256])
def test_launch_plan_covers_every_element_exactly_once(chunk):
    from mygauhuman_amd import optim
    sizes = [0, 1, 3, 255, 256, 257, 9_000_135]
    counts = sizes + sizes[::-1] + [4096, 4095, 4097, 0]
    launches = optim.plan_launches(counts, chunk=chunk)
    assert len(launches) == 1 and launches[0].arrays == list(range(len(counts)))
    for launch in launches:
        assert len(launch.chunk_start) == len(launch.arrays) + 1 and launch.chunk_start[0] == 0
        chunks = optim.launch_chunks(launch, counts, chunk=chunk)
        assert len(chunks) == launch.chunk_start[-1]
        nxt = {i: 0 for i in launch.arrays}
        for e, (i, lo, hi) in enumerate(chunks):
            k = launch.arrays.index(i) if counts.count(counts[i]) == 1 else None
            assert lo == nxt[i] and lo < hi <= counts[i] and hi - lo <= chunk    # in order, no gap, no overlap, inside ITS array
            assert hi == counts[i] or hi - lo == chunk
            if k is not None:
                assert launch.chunk_start[k] <= e < launch.chunk_start[k + 1]
            nxt[i] = hi
        assert all(nxt[i] == counts[i] for i in launch.arrays)             # every element covered
        # the kernel's lookup: the array of entry e is the LARGEST k with chunk_start[k] <= e
        for e in (0, 1, launch.chunk_start[-1] // 2, launch.chunk_start[-1] - 1):
            k = max(j for j in range(len(launch.arrays)) if launch.chunk_start[j] <= e)
            assert launch.arrays[k] == chunks[e][0]


def test_launch_plan_splits_on_array_and_group_limits():
    from mygauhuman_amd import optim
    launches = optim.plan_launches([5] * 150)
    assert [len(x.arrays) for x in launches] == [64, 64, 22]
    assert sum((x.arrays for x in launches), []) == list(range(150))
    launches = optim.plan_launches([5] * 40, groups=list(range(40)))
    assert [len(x.arrays) for x in launches] == [16, 16, 8]
    launches = optim.plan_launches([5] * 40, groups=[0] * 20 + [1] * 20)
    assert [len(x.arrays) for x in launches] == [40]
    assert optim.plan_launches([]) == []
    with pytest.raises(ValueError):
        optim.plan_launches([-1])


def test_step_on_cpu_parameters_raises_no_cpu_path():
    from mygauhuman_amd import optim
    opt = optim.FusedAdam(_groups(), lr=0.0, eps=1e-15)
    opt.step()                                           # no gradients: nothing takes part, nothing to refuse
    for group in opt.param_groups:
        group["params"][0].grad = torch.ones_like(group["params"][0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()
    model = type("M", (), {})()
    model.xyz_gradient_accum, model.denom, model.max_radii2D = torch.zeros(7, 1), torch.zeros(7, 1), torch.zeros(7)
    vpt = torch.zeros(7, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="viewspace_point_tensor.grad is None"):
        optim.update_stats(model, vpt, torch.ones(7, dtype=torch.bool), torch.ones(7, dtype=torch.int32))
    vpt.grad = torch.ones(7, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        optim.update_stats(model, vpt, torch.ones(7, dtype=torch.bool), torch.ones(7, dtype=torch.int32))


def test_training_setup_default_is_still_torch_adam():
    import mygauhuman_amd
    from mygauhuman_amd import densify
    from mygauhuman_amd.scene_model import HumanGaussianModel
    assert mygauhuman_amd.optim.FusedAdam is not None
    lrs = {g: 1e-3 for g in densify.GROUPS}

    def model():
        m = HumanGaussianModel(3, device="cpu")
        for (n, shp) in GROUPS:
            setattr(m, densify.ATTR[n], torch.nn.Parameter(torch.zeros((5,) + shp)))
        return m
    for kw in ({}, {"fused_step": False}):
        opt = densify.training_setup(model(), lrs, **kw)
        assert type(opt) is torch.optim.Adam and [g["name"] for g in opt.param_groups] == list(densify.GROUPS)
    m = model()
    opt = densify.training_setup(m, lrs, fused_step=True)
    assert type(opt) is mygauhuman_amd.optim.FusedAdam and opt is m.optimizer
    assert [g["name"] for g in opt.param_groups] == list(densify.GROUPS) and all(g["eps"] == 1e-15 for g in opt.param_groups)
