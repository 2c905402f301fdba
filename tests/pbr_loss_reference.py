"""Float64 restatement of the PBR-phase training loss (mygauhuman_amd.pbr.loss, csrc/pbr_loss.hip), written from the formulas of
train.py:47-95, :316-344 and utils/loss_utils.py:102-124 as torch expressions, plus the seeded inputs of the fixture cases
(tests/golden/make_golden_pbr_loss.py stores only the reference's outputs; the inputs are rebuilt here from an index hash).

Every term is a separate function so that each value and each gradient can be compared on its own.  entropy() follows the fused
path's rule for a column whose branch is not taken (zero gradient, where the reference's autograd gives NaN next to a taken one)."""
import numpy as np
import torch

from tests.pbr_reference import _u01

BINS = 15
EPS = 1e-6
TERMS = ("l1", "tv", "entropy", "smooth", "prior")
WEIGHTS = dict(l1=1.0, tv=1.0, entropy=5e-5, smooth=0.1, prior=0.001)


def l1(rgb, gt, bound):
    """mean |rgb - gt| over the 3 * n_b values with bound == 1 (n_b = 0: NaN, gradient 0)."""
    sel = (bound.reshape(-1) == 1)
    d = (rgb - gt).reshape(3, -1)[:, sel]
    return d.abs().mean()


def masked_tv(mask, pred):
    """[C,H,W] pred under [1,H,W] mask; masked-out entries stay in the denominators.  The mask products are float32, as in the
    reference (its mask.float() rounds a float64 mask's products; the kernels' are float32 too)."""
    m = mask.reshape(1, *pred.shape[1:]).float()
    th = (pred[:, 1:, :] - pred[:, :-1, :]) ** 2 * (m[:, 1:, :] * m[:, :-1, :])
    tw = (pred[:, :, 1:] - pred[:, :, :-1]) ** 2 * (m[:, :, 1:] * m[:, :, :-1])
    return th.mean() + tw.mean()


def entropy(x, bins=BINS, lo=0.0, hi=1.0):
    """Columns 0..2 of x.view(-1, W): histogram with sigma = unbiased variance; a column enters if its histogram sums to > 1e-6.
    The branch is decided on the values (detached), so a column that does not enter contributes no graph at all."""
    W = x.shape[-1]
    if W < 3:
        raise ValueError("W < 3")
    v = x.reshape(-1, W)
    delta = (hi - lo) / bins
    centres = lo + delta * (torch.arange(bins, dtype=x.dtype) + 0.5)
    total = x.new_zeros(())
    for j in range(3):
        col = v[:, j]
        sigma = col.var() if col.numel() > 1 else col.new_tensor(float("nan"))
        z = (col[None, :] - centres[:, None]) / sigma
        h = (torch.exp(-0.5 * z * z) / (sigma * np.sqrt(2 * np.pi)) * delta).sum(1)
        S = h.sum()
        if bool(S.detach() > EPS):
            p = h / S + EPS
            total = total - (p * torch.log(p)).sum()
    return total


def smooth(g, k1, k2):
    """mean_{P,C} |g[k1] - g[k2]| / (g[k2] + 1e-6)."""
    a, b = g[k1], g[k2]
    return ((a - b).abs() / (b + EPS)).mean()


def prior(roughness, alpha):
    """mean of 1 - roughness over alpha > 0 (n_a = 0: NaN, gradient 0); alpha takes no gradient."""
    sel = alpha.detach().reshape(-1) > 0
    return (1.0 - roughness.reshape(-1)[sel]).mean()


def all_terms(x):
    """{name: value} of every term over the inputs dict x (float64 tensors; albedo_g / roughness_g / knn optional)."""
    t = dict(l1=l1(x["rgb"], x["gt"], x["bound"]),
             tv=masked_tv(x["alpha"], torch.cat([x["albedo"], x["roughness"]], 0)),
             entropy_albedo=entropy(x["albedo"]), entropy_roughness=entropy(x["roughness"]),
             prior=prior(x["roughness"], x["alpha"]))
    if x.get("knn") is not None:
        k1, k2 = x["knn"][:, 1].long(), x["knn"][:, 2].long()
        t["smooth_albedo"] = smooth(x["albedo_g"], k1, k2)
        t["smooth_roughness"] = smooth(x["roughness_g"], k1, k2)
    return t


GRAD_INPUTS = ("rgb", "alpha", "albedo", "roughness", "albedo_g", "roughness_g")


def terms_and_grads(x, term_fn=all_terms):
    """(values {term: float}, grads {term: {input: ndarray}}) with each term differentiated on its own (zero where it does not
    depend on an input)."""
    x = {k: (v.detach().clone().requires_grad_(k in GRAD_INPUTS) if isinstance(v, torch.Tensor) and v.is_floating_point()
             else v) for k, v in x.items()}
    terms = term_fn(x)
    vals, grads = {}, {}
    for name, val in terms.items():
        vals[name] = float(val.detach())
        ins = [k for k in GRAD_INPUTS if k in x]
        gs = torch.autograd.grad(val, [x[k] for k in ins], allow_unused=True, retain_graph=True) if val.requires_grad else \
            [None] * len(ins)
        grads[name] = {k: (np.zeros(x[k].shape) if g is None else g.numpy()) for k, g in zip(ins, gs)}
    return vals, grads


# ---- the fixture cases -----------------------------------------------------------------------------------------------------------
CASES = {"random": (48, 64, 2000, 0), "edges": (20, 24, 300, 1), "empty_bound": (12, 16, 200, 2), "zero_alpha": (12, 16, 200, 3)}


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def case_inputs(name, H=None, W=None, P=None, salt=None):
    """Inputs (float64 tensors holding float32 values, knn int64) of a fixture case, or of a case of any size."""
    if name in CASES:
        H, W, P, salt = CASES[name]
    s = 1000 * salt
    rgb = _f32(_u01((3, H, W), s + 1))
    gt = _f32(_u01((3, H, W), s + 2))
    bound = (_u01((1, H, W), s + 3) > 0.35).astype(np.float64)
    alpha = _f32(_u01((1, H, W), s + 4))
    alpha[_u01((1, H, W), s + 5) < 0.3] = 0.0
    albedo = _f32(_u01((3, H, W), s + 6))
    roughness = _f32(_u01((1, H, W), s + 7) * 0.96 + 0.04)
    knn = np.empty((P, 3), np.int64)
    knn[:, 0] = np.arange(P)
    knn[:, 1:] = np.minimum((_u01((P, 2), s + 8) * P).astype(np.int64), P - 1)
    albedo_g = _f32(_u01((P, 3), s + 9) * 0.98 + 0.02)
    roughness_g = _f32(_u01((P, 1), s + 10) * 0.98 + 0.02)
    if name == "edges":  # constant columns: albedo's column 0 and roughness's column 2 (sigma = 0), and a tiny constant P-row
        albedo[:, :, 0] = 0.25
        roughness[:, :, 2] = np.float32(0.7)
        albedo_g[:5] = 0.5
    if name == "empty_bound":
        bound[:] = 0.0
    if name == "zero_alpha":
        alpha[:] = 0.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return dict(rgb=t(rgb), gt=t(gt), bound=t(bound), alpha=t(alpha), albedo=t(albedo), roughness=t(roughness), knn=t(knn),
                albedo_g=t(albedo_g), roughness_g=t(roughness_g))


def combine(vals, grads):
    """The five unweighted terms of PbrPhaseLoss, the weighted loss and its gradient per input (from per-term values / grads)."""
    groups = dict(l1=["l1"], tv=["tv"], entropy=["entropy_albedo", "entropy_roughness"], smooth=["smooth_albedo", "smooth_roughness"],
                  prior=["prior"])
    terms = {k: sum(vals[n] for n in ns if n in vals) for k, ns in groups.items()}
    loss = sum(WEIGHTS[k] * terms[k] for k in TERMS)
    inputs = set().union(*[g.keys() for g in grads.values()])
    dl = {i: sum(WEIGHTS[k] * grads[n][i] for k, ns in groups.items() for n in ns if n in grads and i in grads[n]) for i in inputs}
    return terms, loss, dl
