"""Time a densification step at training size, unfused (torch ops around gsr_gather_rows) against fused=True (csrc/densify.hip):
one JSON line per measurement, also appended to --out (default profiles/densify_bench.txt).

    python tools/densify_bench.py [--P 200000] [--reps 5] [--out FILE] [--no-launches] [--reference-structure]

  * kl_to_nearest, the six operations and densify_and_prune (plain and with kl_threshold) on the synthetic human (human_synth) with
    Adam moments and statistics in place; thresholds are taken from the cloud itself so that every operation selects a real subset;
  * ms = host clock around the call ending in a device synchronise (an operation contains its host reads), median of --reps on a
    fresh copy of the model each time, after the shader clock has settled (_lib.settle_clock);
  * launches = kernels the call put on the device, counted by the torch profiler in a separate, untimed call;
  * --reference-structure: also prune_points against the reference's structure (boolean-mask indexing and torch.cat per tensor,
    scene/gaussian_model.py:421-487) written with plain torch ops, the comparison this tool made before the fused path existed.
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mygauhuman_amd import _lib, densify, human_synth  # noqa: E402


def reference_structure_prune(m, mask):
    valid = ~mask
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        st = m.optimizer.state.get(p, None)
        if st is not None:
            st["exp_avg"] = st["exp_avg"][valid]
            st["exp_avg_sq"] = st["exp_avg_sq"][valid]
            del m.optimizer.state[p]
            group["params"][0] = torch.nn.Parameter(p[valid].requires_grad_(True))
            m.optimizer.state[group["params"][0]] = st
        else:
            group["params"][0] = torch.nn.Parameter(p[valid].requires_grad_(True))
        setattr(m, densify.ATTR[group["name"]], group["params"][0])
    m.xyz_gradient_accum = m.xyz_gradient_accum[valid]
    m.denom = m.denom[valid]
    m.max_radii2D = m.max_radii2D[valid]


def make_base(P, seed=0):
    """The synthetic human with Adam moments and densification statistics, as in the middle of training."""
    model, _ = human_synth.build(P, seed=seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    densify.training_setup(model, {k: 1e-3 for k in densify.GROUPS})
    for k in densify.GROUPS:
        p = getattr(model, densify.ATTR[k])
        model.optimizer.state[p] = dict(step=torch.tensor(100.0, device="cuda"),
                                        exp_avg=torch.randn(p.shape, device="cuda", generator=g) * 1e-3,
                                        exp_avg_sq=torch.rand(p.shape, device="cuda", generator=g) * 1e-6)
    model.denom = torch.randint(1, 4, (P, 1), device="cuda", generator=g).float()
    model.xyz_gradient_accum = torch.rand((P, 1), device="cuda", generator=g) * 8e-4 * model.denom
    model.max_radii2D = torch.rand((P,), device="cuda", generator=g) * 30
    return model


def fresh(base):
    """A model that owns copies of every per-Gaussian tensor of `base` (an operation replaces them)."""
    m = copy.copy(base)
    densify.training_setup(m, {k: 1e-3 for k in densify.GROUPS}, percent_dense=base.percent_dense)
    for k in densify.GROUPS:
        old = getattr(base, densify.ATTR[k])
        new = torch.nn.Parameter(old.detach().clone())
        setattr(m, densify.ATTR[k], new)
        m.optimizer.param_groups[densify.GROUPS.index(k)]["params"][0] = new
        m.optimizer.state[new] = {a: b.clone() for a, b in base.optimizer.state[old].items()}
    for s in ("xyz_gradient_accum", "denom", "max_radii2D"):
        setattr(m, s, getattr(base, s).clone())
    return m


def measure(base, fn, reps, count_launches):
    ts = []
    for _ in range(reps + 1):   # the first call warms the shapes up
        m = fresh(base)
        torch.manual_seed(0)    # the children's draws: the same for both paths
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(m)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = sorted(ts[1:])
    launches = None
    if count_launches:
        from torch.profiler import ProfilerActivity, profile
        m = fresh(base)
        torch.cuda.synchronize()
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn(m)
                torch.cuda.synchronize()
            launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                           and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        except Exception as ex:  # noqa: BLE001  (a profiler that does not start leaves the count unmeasured, not the times)
            print(f"[densify_bench] launches not measured: {ex}", flush=True)
    return ts[len(ts) // 2], ts[0], launches, m._xyz.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_bench.txt"))
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--reference-structure", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_bench: needs a HIP device (a timing taken anywhere else says nothing)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    clock = _lib.settle_clock()
    P = args.P
    base = make_base(P)
    # thresholds from the cloud: half of the gradients pass, the size test splits the set in two, the KL tests take 50 % / 20 %
    scal = base.get_scaling.detach()
    extent = float(scal.max(dim=1).values.median()) / base.percent_dense
    max_grad = 4e-4
    kl, _ = densify.kl_to_nearest(base, fused=True)
    kl_hi, kl_lo = float(kl.median()), float(torch.quantile(kl, 0.2))
    grads = (base.xyz_gradient_accum / base.denom).detach()
    mask = torch.rand((P,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) < 0.1
    verts = base.SMPL_NEUTRAL["v_template"].reshape(-1, 3).float()
    emit(dict(what="setup", P=P, device=torch.cuda.get_device_name(), settled_GHz=clock[-1][1], clock_readings=len(clock),
              extent=round(extent, 4), kl_median=round(kl_hi, 4), kl_p20=round(kl_lo, 4), reps=args.reps))
    ops = {
        "kl_to_nearest": lambda m, f: densify.kl_to_nearest(m, fused=f),
        "prune_points": lambda m, f: densify.prune_points(m, mask, fused=f),
        "densify_and_clone": lambda m, f: densify.densify_and_clone(m, grads, max_grad, extent, fused=f),
        "densify_and_split": lambda m, f: densify.densify_and_split(m, grads, max_grad, extent, fused=f),
        "kl_densify_and_clone": lambda m, f: densify.kl_densify_and_clone(m, grads, max_grad, extent, kl_threshold=kl_hi, fused=f),
        "kl_densify_and_split": lambda m, f: densify.kl_densify_and_split(m, grads, max_grad, extent, kl_threshold=kl_hi, fused=f),
        "kl_merge": lambda m, f: densify.kl_merge(m, grads, max_grad, extent, kl_threshold=kl_lo, fused=f),
        "densify_and_prune": lambda m, f: densify.densify_and_prune(m, max_grad, 0.005, extent, 20, t_vertices=verts, fused=f),
        "densify_and_prune_kl": lambda m, f: densify.densify_and_prune(m, max_grad, 0.005, extent, 20, t_vertices=verts,
                                                                       kl_threshold=kl_hi, fused=f),
    }
    for name, op in ops.items():
        rec = dict(what=name, P=P)
        for fused in (False, True):
            med, best, launches, rows = measure(base, lambda m: op(m, fused), args.reps, not args.no_launches)
            tag = "fused" if fused else "unfused"
            rec.update({f"{tag}_ms": round(med, 3), f"{tag}_best_ms": round(best, 3), f"{tag}_launches": launches, f"{tag}_rows": rows})
        rec["speedup"] = round(rec["unfused_ms"] / rec["fused_ms"], 2)
        emit(rec)
    if args.reference_structure:
        med, best, launches, rows = measure(base, lambda m: reference_structure_prune(m, mask), args.reps, not args.no_launches)
        emit(dict(what="prune_points, reference structure (torch ops)", P=P, ms=round(med, 3), best_ms=round(best, 3),
                  launches=launches, rows=rows))


if __name__ == "__main__":
    main()
