"""FusedAdam: the reference's torch.optim.Adam(l, lr=0.0, eps=1e-15) (scene/gaussian_model.py:283) as two HIP launches per step
(gsr_adam_step, csrc/adam.hip), with the densification statistics of train.py:401-405 folded into the same launch.

It IS a torch.optim.Adam for everything but step(): the same constructor, param_groups, state, state_dict(), load_state_dict()
and add_param_group(), so update_learning_rate, densify.apply_plan, reset_opacity and the reference's checkpoints work unchanged.
What differs underneath:

  * every `state[p]["step"]` is a 0-dim float32 view into ONE flat device table, the kernels read the counts from it and advance
    them on the device: no host read, no per-tensor `_foreach_add_`;
  * `param_groups[i]["lr"]` stays the Python float callers assign.  Eagerly step() passes the current values by value.  While a
    stream capture is in progress it records the device table `lr_tensor()` instead, and the caller runs `sync_lr()` before each
    replay -- a torch step recorded into a graph would freeze the rate;
  * a group may carry `clamp_min` (default -inf): the parameter is clamped after the update, which is the reference's
    `cubemap.clamp_(min=0.0)` after the light step;
  * the launch table (pointers of parameter, gradient and both moments) is cached and rebuilt whenever one of those tensors has
    been replaced -- a host-side comparison of data_ptr()s, no device read.  A gradient that is not contiguous is replaced by a
    contiguous copy once (p.grad is reassigned; rare: autograd hands out contiguous gradients for contiguous leaves);
  * the kernels write the parameters, both moments and the statistics through their data_ptr()s, so step() and update_stats()
    bump the version counter of every tensor a launch wrote (torch.autograd.graph.increment_version: host-only, nothing is
    launched): a backward over values saved before the step raises as it does after torch's step, and caches keyed on `_version`
    see the write.  A step recorded into a graph bumps once, at record time; a REPLAY runs no host code and bumps nothing, so
    nothing derived from tensors a replay writes may be keyed on their version.

There is no CPU path: step() on CPU parameters raises.
"""
import ctypes as C
import math
from collections import namedtuple

import torch

from . import _lib
from ._lib import call

MAX_ARRAYS = _lib.ADAM_MAX_ARRAYS   # tensors per launch (include/gsr.h: GSR_ADAM_MAX_ARRAYS)
MAX_GROUPS = _lib.ADAM_MAX_GROUPS   # parameter groups per launch
CHUNK = 4096                        # floats per entry of a launch's work list (gsr_adam_chunk_floats(), csrc/adam.hip)

Launch = namedtuple("Launch", "arrays chunk_start")


def plan_launches(counts, groups=None, max_arrays=MAX_ARRAYS, max_groups=MAX_GROUPS, chunk=CHUNK):
    """Split tensors of `counts[i]` floats (tensor i in parameter group `groups[i]`) into launches of at most max_arrays tensors
    and max_groups distinct groups, in order.  Returns [Launch(arrays = tensor indices, chunk_start = exclusive prefix of their
    chunk counts, one longer than arrays)]: tensor arrays[k] owns entries chunk_start[k] .. chunk_start[k + 1] - 1 of the
    launch's work list, entry e of it the floats (e - chunk_start[k]) * chunk .. min(count, that + chunk) - 1.  A tensor without
    elements owns no entry (its step count still advances).  The same layout is built by gsr_adam_step."""
    groups = list(groups) if groups is not None else [0] * len(counts)
    out, cur, seen = [], [], set()
    for i, g in enumerate(groups):
        if cur and (len(cur) == max_arrays or (g not in seen and len(seen) == max_groups)):
            out.append(cur)
            cur, seen = [], set()
        cur.append(i)
        seen.add(g)
    if cur:
        out.append(cur)
    launches = []
    for arrays in out:
        start = [0]
        for i in arrays:
            if counts[i] < 0:
                raise ValueError("plan_launches: negative element count")
            start.append(start[-1] + (counts[i] + chunk - 1) // chunk)
        launches.append(Launch(arrays, start))
    return launches


def launch_chunks(launch, counts, chunk=CHUNK):
    """[(tensor index, first float, end float)] of every work-list entry of a Launch, in work-list order."""
    out = []
    for k, i in enumerate(launch.arrays):
        for e in range(launch.chunk_start[k + 1] - launch.chunk_start[k]):
            out.append((i, e * chunk, min(counts[i], (e + 1) * chunk)))
    return out


def _stats_block(model, viewspace_point_tensor, update_filter, radii):
    """(gsr_adam_stats, tensors to keep alive) for the statistics of `model`."""
    g = viewspace_point_tensor.grad
    if g is None:  # the message of densify.add_densification_stats
        raise RuntimeError("add_densification_stats: viewspace_point_tensor.grad is None (call backward() first and keep "
                           "retain_grad() on the screen-space points)")
    acc, den, mr = model.xyz_gradient_accum, model.denom, model.max_radii2D
    if acc.device.type != "cuda":
        raise RuntimeError("optim: the densification statistics live on the GPU (no CPU path)")
    P = int(acc.shape[0])
    if g.dtype != torch.float32 or g.dim() != 2 or g.shape[0] != P or g.shape[1] < 2:
        raise RuntimeError(f"optim: the screen-space gradient must be float32 [{P}, >= 2], got {g.dtype} {tuple(g.shape)}")
    if P and (g.stride(1) != 1 or g.stride(0) < 2):
        g = g.contiguous()
    f = update_filter
    if f.dtype == torch.bool:
        f = f.view(torch.uint8)
    if f.dtype != torch.uint8 or f.numel() != P:
        raise RuntimeError("optim: update_filter must be a bool / uint8 tensor with one entry per Gaussian")
    f = f.reshape(-1).contiguous()
    r = radii.reshape(-1)
    if r.dtype != torch.int32:
        r = r.to(torch.int32)
    r = r.contiguous()
    if r.numel() != P or mr.numel() != P or den.numel() != P:
        raise RuntimeError("optim: radii, denom and max_radii2D need one entry per Gaussian")
    for t in (acc, den, mr):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != acc.device:
            raise RuntimeError("optim: the statistics tensors must be contiguous float32 tensors on one device")
    for t in (g, f, r):
        if t.device != acc.device:
            raise RuntimeError("optim: the statistics inputs must be on the device of the model (no CPU path)")
    st = _lib.AdamStats(P, int(g.stride(0)) if P else 2, g.data_ptr(), f.data_ptr(), r.data_ptr(), acc.data_ptr(), den.data_ptr(),
                        mr.data_ptr())
    return st, (g, f, r, acc, den, mr)


def update_stats(model, viewspace_point_tensor, update_filter, radii, debug=False):
    """add_densification_stats + the max_radii2D update of train.py:403 in one launch (in place), for the iterations where
    densify_and_prune runs between the statistics and the step."""
    st, keep = _stats_block(model, viewspace_point_tensor, update_filter, radii)
    dev = keep[3].device
    call("gsr_stats_update", dev, C.byref(st), int(debug))
    _written(keep[3:])


def _written(tensors):
    """Tell torch that a kernel wrote these tensors in place (host-only; legal while a stream is being captured)."""
    torch.autograd.graph.increment_version(tensors)


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, debug=False):
        """foreach / capturable / fused are accepted for signature compatibility and have no effect: the step is always the one fused,
        capturable HIP launch.  The groups carry fused=True so that torch lays `step` out as a float32 device tensor when a state
        dict moves between this class and torch.optim.Adam."""
        if weight_decay != 0:
            raise ValueError("FusedAdam: weight_decay != 0 is not supported (the reference trains without it)")
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad is not supported")
        if maximize:
            raise ValueError("FusedAdam: maximize is not supported")
        if differentiable:
            raise ValueError("FusedAdam: differentiable is not supported")
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("FusedAdam: lr and betas are Python floats (lr_tensor() is the device-side learning-rate table)")
        if not eps > 0.0:
            raise ValueError(f"FusedAdam: eps must be > 0, got {eps}")
        self._debug = bool(debug)
        self._steps = None        # flat float32 step table; every state[p]["step"] is a 0-dim view into it
        self._next_slot = 0
        self._lr_table = None
        self._key = None          # what the cached launch tables were built from
        self._launches = []
        self._writes = []         # the tensors those launches write in place: parameters and both moments
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, foreach=False, maximize=False,
                         capturable=False, differentiable=False, fused=True)

    # ------------------------------------------------------------------ state
    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        return torch.device("cpu")

    def _slot_of(self, step):
        """The slot of a step tensor that is a view into the table, else -1."""
        if self._steps is None or step.device != self._steps.device or step.dtype != torch.float32:
            return -1
        off = step.data_ptr() - self._steps.data_ptr()
        return off // 4 if 0 <= off < 4 * self._steps.numel() and off % 4 == 0 else -1

    def _new_slot(self, value=None):
        """A 0-dim view of a fresh slot of the step table, holding `value` (a tensor or None = 0).  Grows the table when it is full:
        the existing counters move with it (device copy) and every state entry is re-pointed."""
        dev = self._device()
        if self._steps is None:
            n = sum(len(g["params"]) for g in self.param_groups)
            self._steps = torch.zeros(max(MAX_ARRAYS, 2 * n), dtype=torch.float32, device=dev)
        if self._next_slot == self._steps.numel():
            old = self._steps
            self._steps = torch.zeros(2 * old.numel(), dtype=torch.float32, device=old.device)
            self._steps[:old.numel()].copy_(old)
            for st in self.state.values():
                s = st.get("step")
                if torch.is_tensor(s) and s.device == old.device and s.dtype == torch.float32:
                    off = s.data_ptr() - old.data_ptr()
                    if 0 <= off < 4 * old.numel():
                        st["step"] = self._steps[off // 4]
            self._key = None
        view = self._steps[self._next_slot]
        self._next_slot += 1
        if value is not None:
            view.copy_(value.detach().reshape(()).to(torch.float32) if torch.is_tensor(value)
                       else torch.tensor(float(value), dtype=torch.float32))
        return view

    def _init_param_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = self._new_slot()
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif not torch.is_tensor(st["step"]) or self._slot_of(st["step"]) < 0:
            st["step"] = self._new_slot(st["step"])  # a counter that came from elsewhere (a loaded checkpoint) moves into the table
        return st

    def init_state(self):
        """Create the state of every parameter now instead of at its first step (what a caller does before it captures a step whose
        first execution would otherwise allocate and zero the moments inside the graph)."""
        for group in self.param_groups:
            for p in group["params"]:
                self._init_param_state(p)
        return self

    def load_state_dict(self, state_dict):
        """Accepts what the reference saves (GaussianModel.capture() -> optimizer.state_dict(): `step` a CPU float tensor) as well as
        this class's own dicts; the counters are moved into the flat device table."""
        super().load_state_dict(state_dict)
        self._steps, self._next_slot = None, 0  # a fresh table: the loaded counters are copied into it one by one
        for group in self.param_groups:
            group["fused"] = True
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdam: the loaded groups ask for weight_decay / amsgrad / maximize, which are not supported")
            for p in group["params"]:
                if len(self.state.get(p, {})) != 0:
                    self._init_param_state(p)
        self._key = None

    # ------------------------------------------------------------------ learning rates
    def lr_tensor(self):
        """The persistent float32 device table [>= len(param_groups)] a captured step reads its learning rates from."""
        n = len(self.param_groups)
        if self._lr_table is None or self._lr_table.numel() < n:
            self._lr_table = torch.zeros(max(MAX_GROUPS, 2 * n), dtype=torch.float32, device=self._device())
            self._lr_table[:n].copy_(torch.tensor([float(g["lr"]) for g in self.param_groups], dtype=torch.float32))
        return self._lr_table

    def sync_lr(self):
        """Copy the groups' current Python learning rates into lr_tensor(), in place (run it before each replay of a captured step)."""
        t = self.lr_tensor()
        n = len(self.param_groups)
        t[:n].copy_(torch.tensor([float(g["lr"]) for g in self.param_groups], dtype=torch.float32))
        return t

    # ------------------------------------------------------------------ the step
    def _collect(self):
        """[(param, grad, state, group index)] of the parameters that take part, after the host-side refusals."""
        items = []
        for gi, group in enumerate(self.param_groups):
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdam: weight_decay / amsgrad / maximize are not supported")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if p.device.type != "cuda":
                    raise RuntimeError("FusedAdam.step: the parameters must live on the GPU (no CPU path)")
                if g.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise RuntimeError(f"FusedAdam.step: float32 parameters and gradients only, got {p.dtype} / {g.dtype}")
                if not p.is_contiguous():
                    raise RuntimeError("FusedAdam.step: parameters must be contiguous")
                if g.device != p.device or g.shape != p.shape:
                    raise RuntimeError("FusedAdam.step: a gradient does not match its parameter's device or shape")
                if not g.is_contiguous():
                    g = g.contiguous()
                    p.grad = g
                st = self._init_param_state(p)
                if (st["exp_avg"].shape != p.shape or st["exp_avg_sq"].shape != p.shape or not st["exp_avg"].is_contiguous()
                        or not st["exp_avg_sq"].is_contiguous() or st["exp_avg"].dtype != torch.float32
                        or st["exp_avg_sq"].dtype != torch.float32 or st["exp_avg"].device != p.device):
                    raise RuntimeError("FusedAdam.step: exp_avg / exp_avg_sq must be contiguous float32 tensors shaped like the "
                                       "parameter, on its device")
                items.append((p, g, st, gi))
        return items

    def _build(self, items):
        counts = [p.numel() for p, _, _, _ in items]
        launches = []
        for launch in plan_launches(counts, [gi for _, _, _, gi in items]):
            gids = []
            for i in launch.arrays:
                if items[i][3] not in gids:
                    gids.append(items[i][3])
            arr = (_lib.AdamArray * len(launch.arrays))()
            for k, i in enumerate(launch.arrays):
                p, g, st, gi = items[i]
                slot = self._slot_of(st["step"])
                arr[k] = _lib.AdamArray(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                        counts[i], gids.index(gi), slot)
            grp = (_lib.AdamGroup * len(gids))()
            launches.append((arr, grp, gids))
        return launches

    @torch.no_grad()
    def step(self, closure=None, *, stats=None):
        """stats = (viewspace_point_tensor, update_filter, radii, model): also update model.xyz_gradient_accum / denom / max_radii2D
        (in place) in the same launch."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        items = self._collect()
        st_block, keep = (None, None)
        if stats is not None:
            vpt, update_filter, radii, model = stats
            st_block, keep = _stats_block(model, vpt, update_filter, radii)
        if not items:
            if st_block is not None:
                call("gsr_stats_update", keep[3].device, C.byref(st_block), int(self._debug))
                _written(keep[3:])
            return loss
        dev = items[0][0].device
        key = tuple((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(),
                     p.numel(), gi) for p, g, st, gi in items)
        if key != self._key:
            if any(p.device != dev for p, _, _, _ in items) or self._steps.device != dev:
                raise RuntimeError("FusedAdam.step: all parameters (and the step table) must be on one device")
            self._launches = self._build(items)
            # (the step table is written too, but only the kernels read it)
            self._writes = [t for p, _, st, _ in items for t in (p, st["exp_avg"], st["exp_avg_sq"])]
            self._key = key
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and (self._lr_table is None or self._lr_table.numel() < len(self.param_groups)):
            raise RuntimeError("FusedAdam.step under stream capture reads its learning rates from lr_tensor(): call sync_lr() once "
                               "before the capture (and before every replay)")
        lr_ptr = self._lr_table.data_ptr() if capturing else None
        for n, (arr, grp, gids) in enumerate(self._launches):
            for k, gi in enumerate(gids):
                group = self.param_groups[gi]
                b1, b2 = group["betas"]
                grp[k] = _lib.AdamGroup(float(b1), float(b2), float(group["lr"]), float(group["eps"]),
                                        float(group.get("clamp_min", -math.inf)), gi)
            last = n == len(self._launches) - 1
            call("gsr_adam_step", dev, len(arr), arr, len(grp), grp, lr_ptr, self._steps.data_ptr(),
                 C.byref(st_block) if (st_block is not None and last) else None, int(self._debug))
        _written(self._writes if st_block is None else self._writes + list(keep[3:]))
        return loss
