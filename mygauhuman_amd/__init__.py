"""mygauhuman_amd -- MI355X-native articulated Gaussian-splat hot path.

Hand-written HIP kernels for gfx950 behind a C ABI (include/gsr.h, libgsr.so), with a PyTorch-ROCm host side that
mirrors the reference's operator surface:

  mygauhuman_amd.diff_gaussian_rasterization  <- submodules/diff-gaussian-rasterization/diff_gaussian_rasterization
  mygauhuman_amd.simple_knn._C.distCUDA2      <- submodules/simple-knn
  mygauhuman_amd.gaussian_renderer.render     <- gaussian_renderer/__init__.py
  mygauhuman_amd.pbr, mygauhuman_amd.nvdiffrast <- pbr/ (CubemapLight, pbr_shading) and nvdiffrast.torch.texture
  mygauhuman_amd.baking                       <- baking.py (bake_set: per-Gaussian occlusion)
  mygauhuman_amd.optim.FusedAdam              <- torch.optim.Adam of scene/gaussian_model.py:283 (+ the statistics of train.py:401-405)

`install_dropin()` registers those modules under the reference's import names so train.py / render.py style
callers work unmodified.
"""
import importlib
import os
import sys

# hipGraph replays on ROCm 7.2 (mygauhuman_amd.graph): with the HIP runtime's AQL "graph packet capture" a hipMemsetAsync NODE on
# memory of a graph's private pool replays wrong once other GPU work has run between two replays (tools/graph_bisect.py,
# profiles/r3_graph_bisect.txt); DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 turns the feature off, at the same replay time.  The variable is
# read when the HIP runtime starts.  This package does NOT touch the process environment on import (round 2 did: a global side effect
# of a library import, and one Python cannot make reliable anyway -- torch.cuda.is_available() may already have started the runtime):
#   * libgsr itself records no memset nodes (every zero-fill is a kernel), so graphs over it are right either way;
#   * the entry points that own their process -- bench.py, the rank launcher, tests/conftest.py -- export the variable before torch
#     is imported, because torch or another library may record memset nodes of its own inside a captured step;
#   * mygauhuman_amd.graph.GraphedFrame VERIFIES every captured graph once (replay, unrelated eager GPU work, replay, compare with
#     the eager step) and raises, naming the variable, if the replay is wrong.
# GRAPH_REPLAY_SAFE only reports whether the variable was "0" when the package was imported.
GRAPH_REPLAY_SAFE = os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") == "0"

__version__ = "0.1.0"


def __getattr__(name):
    # `mygauhuman_amd.optim` without an import statement of its own.  Loaded on first use: it binds libgsr.so, which does not exist
    # yet when mygauhuman_amd.build is imported to make it.
    if name == "optim":
        return importlib.import_module("mygauhuman_amd.optim")
    raise AttributeError(f"module 'mygauhuman_amd' has no attribute {name!r}")


def install_dropin(render=False, nets=False, pbr=False, bake=False, pose_refiner=False, materials_backward=False):
    """Make `import diff_gaussian_rasterization`, `from simple_knn._C import distCUDA2`, `from knn_cuda import KNN` resolve
    to this package.  render=True also registers `gaussian_renderer` (train.py:17 / render.py import `render` -- and train.py
    `network_gui` -- from it), so that the reference's own drivers reach the fused render() without an edit; the reference's
    gaussian_renderer module must then not have been imported before.  nets=True registers `nets.mlp_delta_weight_lbs`
    (scene/gaussian_model.py:27 imports LBSOffsetDecoder from it): the skinning-offset network on the fused kernels, same
    constructor, same state_dict keys.  pbr=True registers `pbr` (train.py / render.py: CubemapLight, get_brdf_lut, pbr_shading)
    and `nvdiffrast` / `nvdiffrast.torch` (texture() for the reference's call shapes): the image-based-lighting stage on the
    fused kernels of csrc/pbr.hip.  bake=True registers `baking` (bake_set on the kernels of csrc/bake.hip) and turns on baking
    in render(): at iteration > 30000 a camera without `occlusion` is baked and keeps it.  pose_refiner=True registers
    `nets.mlp_delta_body_pose` (scene/gaussian_model.py imports BodyPoseRefiner from it): the pose-correction network on the fused
    kernels of csrc/pose_refiner.hip (nets_pose.py), same constructor, same state_dict keys; nets=True alone leaves it alone.
    materials_backward=True sets gaussian_renderer.GEOMETRY_GRAD = "auto": render() takes the materials-only backward
    (csrc/blend_colors_bwd.hip) whenever none of the model's geometry leaves requires grad -- what update_learning_rate leaves
    behind after pbr_iteration (scene/gaussian_model.py:296-306).  The default leaves the switch at True: the full backward."""
    pairs = [("diff_gaussian_rasterization", "mygauhuman_amd.diff_gaussian_rasterization"),
             ("simple_knn", "mygauhuman_amd.simple_knn"),
             ("simple_knn._C", "mygauhuman_amd.simple_knn._C"),
             ("knn_cuda", "mygauhuman_amd.knn_cuda")]
    if render:
        pairs += [("gaussian_renderer", "mygauhuman_amd.gaussian_renderer"),
                  ("gaussian_renderer.network_gui", "mygauhuman_amd.gaussian_renderer.network_gui")]
    if nets:
        pairs += [("nets.mlp_delta_weight_lbs", "mygauhuman_amd.nets")]
    if pbr:
        pairs += [("pbr", "mygauhuman_amd.pbr"), ("pbr.light", "mygauhuman_amd.pbr.light"), ("pbr.shade", "mygauhuman_amd.pbr.shade"),
                  ("nvdiffrast", "mygauhuman_amd.nvdiffrast"), ("nvdiffrast.torch", "mygauhuman_amd.nvdiffrast.torch")]
    if bake:
        pairs += [("baking", "mygauhuman_amd.baking")]
    if pose_refiner:
        pairs += [("nets.mlp_delta_body_pose", "mygauhuman_amd.nets_pose")]
    for theirs, ours in pairs:
        sys.modules[theirs] = importlib.import_module(ours)
    if bake:
        importlib.import_module("mygauhuman_amd.gaussian_renderer").BAKE = True
    if materials_backward:
        importlib.import_module("mygauhuman_amd.gaussian_renderer").GEOMETRY_GRAD = "auto"
