"""Scenes and CPU references shared by the tests of an ACTIVE SH degree below the STORED one (test_sh_degree_host.py without a
GPU, test_gpu_sh_degree.py with one): the configuration every training run starts in -- sixteen stored coefficients per
Gaussian, degree 0, raised by one every 1000 iterations.

A scene is made at its stored degree (M = 16 / 9 / 4 coefficients), then g["sh_degree"] = D and the coefficients of the bands
above D are multiplied by 50 (util.stored_above_active): a kernel that reads one band too many, or strides its rows by
(D + 1)^2 instead of M, is wrong by far more than any tolerance.  The references -- the CPU oracle and the float64 restatement
of tests/raster_reference.py -- are computed once per (scene, P, M, D, scale modifier) and shared; callers must not write to
them."""
import functools
import types

import numpy as np

from tests import raster_reference as rr
from tests import util
from tests.test_raster_reference_host import BG, IDENTITY, MAX_MARGIN_FRAC  # noqa: F401  (re-exported)

# the two identity-camera scenes of test_raster_reference_host.py: (P, W, H, seed, scale, behind_frac)
SCENES = {"p600": IDENTITY[1], "p300": IDENTITY[0]}
assert SCENES["p600"] == (600, 128, 96, 2, 0.03, 0.2) and SCENES["p300"] == (300, 80, 56, 1, 0.05, 0.1)
# block tails: the first P Gaussians of the 600-Gaussian scene (forward preprocess blocks of 256, backward blocks of 128)
TAILS = (1, 127, 129, 257)
STORED_DEGREE = {16: 3, 9: 2, 4: 1}
LAYOUTS = ((16, 0), (16, 1), (16, 2), (9, 0), (9, 1), (4, 0))   # (M stored coefficients, D active degree)
MODIFIERS = (0.5, 1.7)
PER_GAUSSIAN = ("means3D", "opacities", "scales", "rotations", "shs", "colors", "cov3D")


@functools.lru_cache(maxsize=None)
def scene(name, P, M, D):
    """(cam, g): scene `name` stored at M coefficients with active degree D (D == stored: untouched), cut to its first P."""
    P0, W, H, seed, scale, behind = SCENES[name]
    cam, g = util.make_scene(P0, W, H, seed, STORED_DEGREE[M], scale, behind)
    assert g["shs"].shape == (P0, M, 3)
    if D != STORED_DEGREE[M]:
        g = util.stored_above_active(g, D)
    if P != P0:
        g = {k: (np.ascontiguousarray(v[:P]) if k in PER_GAUSSIAN else v) for k, v in g.items()}
    return cam, g


def poisoned(g, value=np.nan):
    """A copy of g whose inactive coefficients are `value`."""
    out = dict(g)
    out["shs"] = g["shs"].copy()
    out["shs"][:, (g["sh_degree"] + 1) ** 2:] = value
    return out


def zeroed(g):
    return poisoned(g, 0.0)


_REF = {}


def reference(oracle, name, P, M, D, modifier=1.0):
    """Oracle and float64 results of one case: forward of both, the keep mask (off the oracle's fragile pixels and the
    restatement's margin), rr.upstream gradients that are zero outside it, and both backwards."""
    key = (name, P, M, D, float(modifier))
    if key not in _REF:
        cam, g = scene(name, P, M, D)
        ref = util.oracle_forward(oracle, cam, g, BG, "sh", scale_modifier=modifier)
        r64 = rr.forward(cam, g, BG, "sh", scale_modifier=modifier)
        keep = (ref["img"]["fragile"] == 0) & ~r64["margin"]
        up = rr.upstream(cam["H"], cam["W"], SCENES[name][3], keep)
        want = oracle.rasterize_backward(ref, *up)
        want64 = rr.backward(cam, g, BG, "sh", *up, scale_modifier=modifier)
        _REF[key] = types.SimpleNamespace(cam=cam, g=g, ref=ref, r64=r64, keep=keep, up=up, want=want, want64=want64,
                                          visible=ref["pre"]["radii"] > 0, M=M, D=D, n_active=(D + 1) ** 2)
    return _REF[key]


def assert_inactive_zero(what, dL_dsh, radii, D):
    """dL_dsh [P,M,3]: the bands above D exactly 0.0 in every row (no NaN, no tiny value, no -0.0 excepted: -0.0 == 0.0), and
    the whole row of a culled Gaussian exactly zero."""
    dL_dsh, radii = np.asarray(dL_dsh), np.asarray(radii)
    n = (D + 1) ** 2
    tail = dL_dsh[:, n:]
    assert not np.isnan(dL_dsh).any(), f"{what}: NaN in dL_dsh"
    assert np.all(tail == 0.0), (f"{what}: {int((tail != 0).sum())} non-zero gradients in the inactive bands, largest "
                                 f"{float(np.abs(tail).max()):.3e}")
    culled = dL_dsh[radii == 0]
    assert np.all(culled == 0.0), f"{what}: {int((culled != 0).sum())} non-zero gradients in rows of culled Gaussians"


def bits_equal(a, b):
    """Same bits (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
