"""Scenes and yardsticks of the colour-only backward's tests (test_gpu_material_backward.py, test_material_backward_host.py).

A case is a scene in the precomputed-colour / precomputed-covariance mode with 18 extra colour channels, gradient images for the
main colour and for four of the six triples (two stay null), and per image two yardsticks of dL_dcolors: the CPU oracle's plain
pass with colors = that triple, and the float64 restatement (tests/raster_reference.py).  Computed once per process (CPU)."""
import types

import numpy as np

from tests import raster_reference as rr
from tests import scenes, util
from tests.test_raster_reference_host import BG, tolerance

W, H = 100, 70           # partial tiles on the right and bottom edges; 7 x 5 tiles is not a multiple of 8
LIVE_TRIPLES = (0, 2, 3, 5)   # triples that get a gradient image; 1 and 4 stay null
MAIN = 6                 # index of the main colour among the images of a case
STACKS = ("stack_translucent", "stack_opaque", "stack_tail")
NAMES = scenes.FAMILIES + STACKS
# keep = (fragile == 0) & ~margin covers at least this much of the image at 100 x 70 (general_skew: 0.953)
MIN_KEEP = {"general_skew": 0.95}
MIN_KEEP_DEFAULT = 0.98

_CASES = {}


def stack_scene(translucent, tail_only=False):
    """2000 Gaussians at 100 x 70 with rows 400: pulled towards the image centre: four tiles carry lists of ~1400-1600 entries
    (beyond the 512-entry sort limit and the blend_segments threshold) against a mean of ~190.  translucent: the stacked rows are
    faint, so the walk reaches the end of the lists; otherwise it terminates early inside a long list.  tail_only: rows 400: alone
    (P = 1600; tiles with empty lists)."""
    cam, g = util.make_scene(2000, W, H, seed=5, deg=3, scale=0.03, behind_frac=0.05)
    c = np.median(g["means3D"][:, :2], axis=0)
    g["means3D"][400:, :2] = c + 0.12 * (g["means3D"][400:, :2] - c)
    if translucent:
        g["opacities"][400:] *= 0.06
    if tail_only:
        P = g["means3D"].shape[0]
        g = {k: (v[400:] if isinstance(v, np.ndarray) and v.shape[:1] == (P,) else v) for k, v in g.items()}
    g["colors"] = np.random.default_rng(55).random((g["means3D"].shape[0], 3)).astype(np.float32)
    return cam, g


def scene(name):
    if name in scenes.FAMILIES:
        return scenes.make(name, 0, W=W, H=H)
    return stack_scene(name != "stack_opaque", tail_only=name == "stack_tail")


def family_of(name):
    """The key of tolerance(): the stack scenes hold to the default."""
    return name if name in scenes.FAMILIES else "stack"


def case(oracle, name):
    """cam, g, extra [P,18], keep [H,W], grads {image index: [3,H,W] float32} (MAIN and LIVE_TRIPLES), want / want64 {image index:
    [P,3]} (oracle float32 / float64), ref (the oracle's main pass), n_contrib_max, list lengths per tile."""
    if name in _CASES:
        return _CASES[name]
    cam, g = scene(name)
    P = g["means3D"].shape[0]
    rng = np.random.default_rng(1000 + NAMES.index(name))
    extra = rng.random((P, 18)).astype(np.float32)
    ref = util.oracle_forward(oracle, cam, g, BG, "precomp")
    r64 = rr.forward(cam, g, BG, "precomp")
    keep = (ref["img"]["fragile"] == 0) & ~r64["margin"]
    assert keep.mean() > MIN_KEEP.get(name, MIN_KEEP_DEFAULT), (name, keep.mean())
    zero1 = np.zeros((1, H, W), np.float32)
    grads, want, want64 = {}, {}, {}
    for i in LIVE_TRIPLES + (MAIN,):
        grads[i] = rr.upstream(H, W, 10 * NAMES.index(name) + i, keep)[0]
        gi = g if i == MAIN else {**g, "colors": np.ascontiguousarray(extra[:, 3 * i:3 * i + 3])}
        fwd = ref if i == MAIN else util.oracle_forward(oracle, cam, gi, BG, "precomp")
        want[i] = oracle.rasterize_backward(fwd, grads[i], zero1, zero1)["dL_dcolors"]
        want64[i] = rr.backward(cam, gi, BG, "precomp", grads[i], zero1, zero1)["dL_dcolors"]
    ranges = ref["bin"]["ranges"].astype(np.int64)
    out = types.SimpleNamespace(name=name, cam=cam, g=g, P=P, extra=extra, keep=keep, grads=grads, want=want, want64=want64, ref=ref,
                                n_contrib_max=int(ref["img"]["n_contrib"].max()), lists=ranges[:, 1] - ranges[:, 0],
                                culled=int((ref["pre"]["radii"] == 0).sum()))
    _CASES[name] = out
    return out


def bounds(name, size):
    """(tol against the oracle, tol against float64, max_bad_frac): the bounds tests/test_gpu_cameras.py holds dL_dcolors to."""
    t64 = tolerance(family_of(name), "dL_dcolors")
    t32 = max(1e-4, t64 if name == "needle" else 0.0)
    return t32, t64, max(3e-4, 2.5 / size)
