"""ctypes binding of libgsr.so (the C ABI declared in include/gsr.h).

There is NO fallback: if the HIP library is missing or does not load, importing this module raises."""
import contextlib
import ctypes as C
import os

# torch ships its own libamdhip64 / libhsa-runtime64 under torch/lib.  Import it BEFORE libgsr.so is dlopen'ed so that both
# bind to ONE HIP runtime (the loader reuses the already loaded soname); the other order puts two runtimes in the process
# and the second one finds "no ROCm-capable device".
import torch  # noqa: F401  (load order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsr.so")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class Phase1LossStruct(C.Structure):
    """gsr_phase1_loss (include/gsr.h): the fused phase-1 training loss of render()."""
    _fields_ = [("gt_image", C.c_void_p), ("gt_normal", C.c_void_p), ("alpha_target", C.c_void_p), ("bound", C.c_void_p),
                ("w_image", C.c_float), ("w_alpha", C.c_float), ("w_normal", C.c_float), ("w_axis", C.c_float),
                ("normal_triple", C.c_int), ("axis_triple", C.c_int),
                ("color", C.c_void_p), ("alpha", C.c_void_p), ("extra_images", C.c_void_p), ("stats", C.c_void_p),
                ("upstream", C.c_void_p)]

PBR_MAX_LEVELS = 16


class PbrTexture(C.Structure):
    """gsr_pbr_texture (include/gsr.h): one 2-D texture or cube map with its mip levels (and their gradient buffers)."""
    _fields_ = [("cube", C.c_int), ("channels", C.c_int), ("levels", C.c_int),
                ("width", C.c_int * PBR_MAX_LEVELS), ("height", C.c_int * PBR_MAX_LEVELS),
                ("data", C.c_void_p * PBR_MAX_LEVELS), ("grad", C.c_void_p * PBR_MAX_LEVELS)]


class PbrShade(C.Structure):
    """gsr_pbr_shade (include/gsr.h): the fused pbr_shading pass."""
    _fields_ = [("n", C.c_int), ("tone", C.c_int), ("gamma", C.c_int)] + \
        [(k, C.c_void_p) for k in ("normals", "view_dirs", "albedo", "roughness", "mask", "occlusion", "metallic", "background")] + \
        [("diffuse", PbrTexture), ("specular", PbrTexture), ("lut", PbrTexture)] + \
        [(k, C.c_void_p) for k in ("render_rgb", "diffuse_rgb", "specular_rgb", "diffuse_light",
                                   "d_render_rgb", "d_diffuse_rgb", "d_specular_rgb", "d_diffuse_light",
                                   "d_albedo", "d_roughness", "d_occlusion", "d_metallic")]


class BakeScene(C.Structure):
    """gsr_bake_scene (include/gsr.h): the inputs of the occlusion bake."""
    _fields_ = [("P", C.c_int), ("C", C.c_int)] + [(k, C.c_void_p) for k in (
        "means3D", "scales", "rotations", "opacities", "cell", "views", "projs", "dir_texel")] + [("ndir", C.c_int)]


class PbrLoss(C.Structure):
    """gsr_pbr_loss (include/gsr.h): the fused PBR-phase training loss."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("rgb", C.c_void_p), ("rgb_stride", C.c_longlong * 3),
                ("gt", C.c_void_p), ("bound", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p), ("mask", C.c_void_p),
                ("ca", C.c_int), ("cb", C.c_int), ("tv", C.c_int), ("entropy", C.c_int * 2), ("prior", C.c_int),
                ("bins", C.c_int), ("lo", C.c_float), ("hi", C.c_float),
                ("P", C.c_int), ("k1", C.c_void_p), ("k2", C.c_void_p), ("g", C.c_void_p * 2), ("gc", C.c_int * 2),
                ("inv_off", C.c_void_p * 2), ("inv_idx", C.c_void_p * 2)] + \
        [(k, C.c_float) for k in ("w_l1", "w_tv", "w_entropy", "w_smooth", "w_prior")] + \
        [(k, C.c_void_p) for k in ("loss", "terms", "upstream", "d_rgb", "d_a", "d_b", "d_mask")] + [("d_g", C.c_void_p * 2)]


SSIM_CROP_MAX_GROUPS = 4
MASK_F32, MASK_U8 = 0, 1  # mask_dtype of gsr_bounding_rect


class SsimCrop(C.Structure):
    """gsr_ssim_crop (include/gsr.h): SSIM of up to four (img1, img2) groups on the rectangle held in device memory."""
    _G = SSIM_CROP_MAX_GROUPS
    _fields_ = [("groups", C.c_int), ("height", C.c_int), ("width", C.c_int), ("rect", C.c_void_p), ("planes", C.c_int * _G),
                ("img1", C.c_void_p * _G), ("img1_stride", (C.c_longlong * 3) * _G), ("img2", C.c_void_p * _G),
                ("dA", C.c_void_p * _G), ("dB", C.c_void_p * _G), ("dC", C.c_void_p * _G), ("value", C.c_void_p * _G),
                ("upstream", C.c_void_p * _G), ("d_img1", C.c_void_p * _G)]


ADAM_MAX_ARRAYS, ADAM_MAX_GROUPS = 64, 16


class AdamArray(C.Structure):
    """gsr_adam_array (include/gsr.h): one tensor of the fused Adam step."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("count", C.c_longlong), ("group", C.c_int), ("step_slot", C.c_int)]


class AdamGroup(C.Structure):
    """gsr_adam_group (include/gsr.h): the hyperparameters of one parameter group."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("lr", C.c_float), ("eps", C.c_float), ("clamp_min", C.c_float),
                ("lr_slot", C.c_int)]


class AdamStats(C.Structure):
    """gsr_adam_stats (include/gsr.h): the densification statistics folded into the step."""
    _fields_ = [("P", C.c_int), ("grad_stride", C.c_int), ("grad", C.c_void_p), ("filter", C.c_void_p), ("radii", C.c_void_p),
                ("grad_accum", C.c_void_p), ("denom", C.c_void_p), ("max_radii", C.c_void_p)]


EVAL_MAX_SLOTS = 16
EVAL_FILL, EVAL_FLIP_Z = 1, 2  # slot flags of gsr_eval_view


class EvalSlot(C.Structure):
    """gsr_eval_slot (include/gsr.h): one image of the evaluation view finish."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("u8", C.c_void_p), ("stride", C.c_longlong * 3), ("channels", C.c_int),
                ("flags", C.c_int)]


class EvalView(C.Structure):
    """gsr_eval_view (include/gsr.h): the images of one view, the bound mask, the device background and the metrics table."""
    _fields_ = [("slots", C.c_int), ("height", C.c_int), ("width", C.c_int), ("slot", EvalSlot * EVAL_MAX_SLOTS),
                ("mask", C.c_void_p), ("mask_dtype", C.c_int), ("background", C.c_void_p), ("metric_image", C.c_int),
                ("metric_gt", C.c_int), ("counter", C.c_void_p), ("table", C.c_void_p), ("capacity", C.c_int),
                ("overflow", C.c_void_p)]


# The prototypes of include/gsr.h, the ONE place a new entry point is bound:  name: (return type, parameters, STREAM | PLAIN).
# STREAM = the function's last parameter is the gsr_stream_t, which is NOT written in the list (_load() appends it, call() passes
# it).  tests/test_abi_table_host.py holds every line against the header.  Device pointers travel as integers (_P).
_I, _U, _F, _Z, _LL, _P = C.c_int, C.c_uint, C.c_float, C.c_size_t, C.c_longlong, C.c_void_p
_S, _IP, _PP, _U64P = C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong)
STREAM, PLAIN = True, False
_RASTER_IN = [_I, _I, _I, _P, _I, _I] + [_P] * 5 + [_F] + [_P] * 5 + [_F, _F, _I] + [_P] * 4 + [_I]  # P .. debug of the forwards
_RASTER_BWD = [_I, _I, _I, _I, _P, _I, _I] + [_P] * 5 + [_F] + [_P] * 5 + [_F, _F] + [_P] * 4  # P .. image_buffer of the backwards
_LBS_IN = [_I, _I] + [_P] * 19  # P, V, query .. world_normals
_ATTR_IN = [_I, _I, _I] + [_P] * 4 + [_F] + [_P] * 5  # P, sh_degree, M, means3D .. occlusion

TABLE = {
    "gsr_version": (_I, [], PLAIN),
    "gsr_has_experiments": (_I, [], PLAIN),
    "gsr_target_arch": (_S, [], PLAIN),
    "gsr_last_error": (_S, [], PLAIN),
    "gsr_set_binning_mode": (_I, [_I], PLAIN),
    "gsr_get_binning_mode": (_I, [], PLAIN),
    "gsr_set_tuning": (_I, [_S, _I], PLAIN),
    "gsr_set_stream_tuning": (_I, [_P, _S, _I], PLAIN),
    "gsr_clear_stream_tuning": (_I, [], STREAM),
    "gsr_profile_enable": (_I, [_U], PLAIN),
    "gsr_profile_reset": (_I, [], PLAIN),
    "gsr_profile_read": (_I, [_I, C.POINTER(C.c_double), C.POINTER(C.c_long)], PLAIN),
    "gsr_debug_wave_trace": (_I, [_P, _Z], PLAIN),
    "gsr_debug_clock_probe": (_I, [_I, _I, _P], STREAM),
    # rasterizer
    "gsr_mark_visible": (_I, [_I, _P, _P, _P, _P], STREAM),
    "gsr_rasterize_forward": (_I, [ALLOC_FN, _P] * 3 + _RASTER_IN + [_IP], STREAM),
    "gsr_geometry_bytes": (_Z, [_I], PLAIN),
    "gsr_image_bytes": (_Z, [_I, _I], PLAIN),
    "gsr_binning_bytes": (_Z, [_Z, _I, _I], PLAIN),
    "gsr_rasterize_forward_async": (_I, [_P, _P, _Z, _P] + _RASTER_IN + [_P], STREAM),
    "gsr_rasterize_backward": (_I, _RASTER_BWD + [_P] * 12 + [_I], STREAM),
    "gsr_phase1_loss_partials": (_Z, [], PLAIN),
    "gsr_phase1_loss_forward": (_I, [_I, _I, C.POINTER(Phase1LossStruct), _P], STREAM),
    "gsr_alpha_mask_loss_backward": (_I, [_I, _I, _P, _P, _P, _P, _F, _P, _P], STREAM),
    "gsr_rasterize_backward_alpha_mask_loss": (_I, _RASTER_BWD + [_P, _P, _P, _F] + [_P] * 9 + [_I, _I], STREAM),
    "gsr_query_state": (_I, [_I] * 5 + [_P] * 4, STREAM),
    # simple-knn, sorts, k-NN, row gather
    "gsr_dist2_workspace_bytes": (_Z, [_I], PLAIN),
    "gsr_dist2": (_I, [_I, _P, _P, _P, _Z], STREAM),
    "gsr_sort_workspace_bytes": (_Z, [_Z], PLAIN),
    "gsr_sort_pairs_u64": (_I, [_Z, _P, _P, _P, _P, _I, _P, _Z], STREAM),
    "gsr_sort_pairs_u32": (_I, [_Z, _P, _P, _P, _P, _I, _P, _Z], STREAM),
    "gsr_knn_self": (_I, [_I, _P, _I, _P, _P, _P, _Z], STREAM),
    "gsr_knn_nearest": (_I, [_I, _P, _I, _P, _P, _P, _P, _Z], STREAM),
    "gsr_gather_rows": (_I, [_I, _PP, _PP, _IP, _IP, _I, _P], STREAM),
    # densification: pair KL, selections, row plans, rows with the new ones computed
    "gsr_kl_pairs": (_I, [_I] + [_P] * 5, STREAM),
    "gsr_densify_select": (_I, [_I, _I, _P, _I, _P, _P, _F, _F, _F, _P], STREAM),
    "gsr_densify_plan_workspace_bytes": (_Z, [_I], PLAIN),
    "gsr_densify_plan": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _Z], STREAM),
    "gsr_build_rows": (_I, [_I, _PP, _PP, _IP, _IP, _IP, _I, _P, _I, _I, _I, _P, _P, _F, _P], STREAM),
    # skinning, pose chain, pose blend shapes
    "gsr_lbs_workspace_bytes": (_Z, [_I], PLAIN),
    "gsr_lbs_grid_build": (_I, [_I, _P, _P, _Z], STREAM),
    "gsr_lbs_nn_cache_bytes": (_Z, [_I], PLAIN),
    "gsr_lbs_forward": (_I, _LBS_IN, STREAM),
    "gsr_lbs_forward_grid": (_I, _LBS_IN + [_P, _Z, _I], STREAM),
    "gsr_lbs_forward_cached": (_I, _LBS_IN + [_P, _Z, _P, _Z, _I], STREAM),
    "gsr_lbs_backward_workgroups": (_I, [_I], PLAIN),
    "gsr_lbs_backward": (_I, [_I, _I] + [_P] * 20, STREAM),
    "gsr_smpl_pose_forward": (_I, [_P, _P, _P, _IP, _P, _P], STREAM),
    "gsr_smpl_pose_backward": (_I, [_P, _P, _P, _IP] + [_P] * 5, STREAM),
    "gsr_gemv_rows": (_I, [_I, _I, _P, _P, _P], STREAM),
    "gsr_gemv_rows_t": (_I, [_I, _I, _P, _P, _P], STREAM),
    # view-parallel exchange
    "gsr_sh_view_pack": (_I, [_I, _P, _P, _P], STREAM),
    "gsr_sh_grad_from_views": (_I, [_I] * 4 + [_P, _P, _Z, _F, _P, _P], STREAM),
    "gsr_sh_view_pack_posed": (_I, [_I, _P, _P, _P, _P, _P, _Z, _Z], STREAM),
    "gsr_sh_grad_from_views_posed": (_I, [_I, _I, _I, _P, _Z, _Z, _Z, _F, _P, _P, _P], STREAM),
    "gsr_step_status": (_I, [_I, _P, _P, _F, _P, _P], STREAM),
    "gsr_step_finish": (_I, [_P, _P, _Z, _Z, _F, _P, _P], STREAM),
    # losses
    "gsr_ssim_forward": (_I, [_I] * 3 + [_P] * 6, STREAM),
    "gsr_ssim_backward": (_I, [_I] * 3 + [_P] * 3 + [_F] + [_P] * 4, STREAM),
    "gsr_bounding_rect_workspace_ints": (_Z, [], PLAIN),
    "gsr_bounding_rect": (_I, [_I, _I, _P, _I, _P, _P], STREAM),
    "gsr_ssim_crop_workspace_floats": (_Z, [_I] * 3, PLAIN),
    "gsr_ssim_crop_forward": (_I, [C.POINTER(SsimCrop), _P], STREAM),
    "gsr_ssim_crop_backward": (_I, [C.POINTER(SsimCrop)], STREAM),
    "gsr_pbr_loss_workspace_floats": (_Z, [], PLAIN),
    "gsr_pbr_loss_forward": (_I, [C.POINTER(PbrLoss), _P], STREAM),
    "gsr_pbr_loss_backward": (_I, [C.POINTER(PbrLoss), _P], STREAM),
    # per-frame activations and attributes
    "gsr_model_activations_forward": (_I, [_I] + [_P] * 11, STREAM),
    "gsr_model_activations_backward": (_I, [_I] + [_P] * 16, STREAM),
    "gsr_model_activations_backward_acc": (_I, [_I] + [_P] * 17, STREAM),
    "gsr_frame_attributes_forward": (_I, _ATTR_IN + [_P] * 3 + [_P] * 3, STREAM),
    "gsr_frame_attributes_backward": (_I, _ATTR_IN + [_P] * 3 + [_P] * 3 + [_P] * 10, STREAM),
    "gsr_frame_attributes_forward_split": (_I, _ATTR_IN + [_P] * 4 + [_P] * 3, STREAM),
    "gsr_frame_attributes_backward_split": (_I, _ATTR_IN + [_P] * 4 + [_P] * 3 + [_P] * 11, STREAM),
    "gsr_frame_attributes_backward_acc": (_I, _ATTR_IN + [_P] * 4 + [_P] * 3 + [_P] * 11 + [_P], STREAM),
    # networks
    "gsr_lbs_offset_mlp_packed_floats": (_Z, [], PLAIN),
    "gsr_lbs_offset_mlp_pack": (_I, [_PP, _PP, _P], STREAM),
    "gsr_lbs_offset_mlp_forward": (_I, [_I, _P, _P, _P], STREAM),
    "gsr_lbs_offset_mlp_set_precision": (_I, [_I], PLAIN),
    "gsr_debug_lbs_offset_mlp_forward_bf16x3": (_I, [_I, _P, _P, _P], STREAM),
    "gsr_lbs_offset_mlp_backward_workspace_floats": (_Z, [_I], PLAIN),
    "gsr_lbs_offset_mlp_backward": (_I, [_I, _P, _P, _P, _P, _PP, _PP], STREAM),
    "gsr_pose_refiner_forward": (_I, [_I, _I, _I, _P, _LL, _LL, _PP, _PP, _P], STREAM),
    "gsr_pose_refiner_backward": (_I, [_I, _I, _I, _P, _LL, _LL, _PP, _PP, _P, _PP, _PP, _P], STREAM),
    # image-based lighting
    "gsr_pbr_texture_forward": (_I, [C.POINTER(PbrTexture), _I, _P, _P, _P], STREAM),
    "gsr_pbr_texture_backward": (_I, [C.POINTER(PbrTexture), _I, _P, _P, _P, _P, _P], STREAM),
    "gsr_pbr_cube_mip_forward": (_I, [_I, _I, _P, _P], STREAM),
    "gsr_pbr_cube_mip_backward": (_I, [_I, _I, _P, _P], STREAM),
    "gsr_pbr_diffuse_forward": (_I, [_I, _P, _P], STREAM),
    "gsr_pbr_diffuse_backward": (_I, [_I, _P, _P], STREAM),
    "gsr_pbr_specular_forward": (_I, [_I, _F, _F, _P, _P, _P], STREAM),
    "gsr_pbr_specular_backward": (_I, [_I, _F, _F, _P, _P, _P], STREAM),
    "gsr_pbr_shade_forward": (_I, [C.POINTER(PbrShade)], STREAM),
    "gsr_pbr_shade_backward": (_I, [C.POINTER(PbrShade)], STREAM),
    "gsr_pbr_env_grey": (_I, [_I, _P, _I, _P, _P], STREAM),
    "gsr_pbr_env_tv_workspace_floats": (_Z, [_I, _I], PLAIN),
    "gsr_pbr_env_tv_forward": (_I, [_I, _P, _I, _I, _P, _P, _P], STREAM),
    "gsr_pbr_env_tv_backward": (_I, [_I, _I, _I, _P, _P, _P, _P, _I], STREAM),
    "gsr_pbr_view_dirs": (_I, [_I, _P, _P, _P], STREAM),
    # occlusion bake
    "gsr_bake_grid_workspace_bytes": (_Z, [], PLAIN),
    "gsr_bake_grid": (_I, [_I, _P, _P, _P, _P, _P, _IP, _P, _Z], STREAM),
    "gsr_bake_plan_bytes": (_Z, [_I, _I], PLAIN),
    "gsr_bake_plan": (_I, [C.POINTER(BakeScene), _P, _Z, _U64P], STREAM),
    "gsr_bake_visibility_workspace_bytes": (_Z, [_I, _Z], PLAIN),
    "gsr_bake_visibility": (_I, [C.POINTER(BakeScene), _P, _P, _P, _Z, _U64P], STREAM),
    "gsr_bake_expand": (_I, [_I, _I, _P, _P, _P, _P, _P], STREAM),
    "gsr_bake_env_reduce": (_I, [_I, _P, _P, _P], STREAM),
    # optimizer, evaluation
    "gsr_adam_chunk_floats": (_I, [], PLAIN),
    "gsr_adam_step": (_I, [_I, C.POINTER(AdamArray), _I, C.POINTER(AdamGroup), _P, _P, C.POINTER(AdamStats), _I], STREAM),
    "gsr_stats_update": (_I, [C.POINTER(AdamStats), _I], STREAM),
    "gsr_eval_workspace_floats": (_Z, [_I, _I], PLAIN),
    "gsr_eval_view_finish": (_I, [C.POINTER(EvalView), _P], STREAM),
}


def _variant(base, lead=(), tail=()):
    """The prototype of `base` with parameters put in front of its own and behind them (before the stream)."""
    restype, argtypes, streamed = TABLE[base]
    return restype, [*lead, *argtypes, *tail], streamed


_EX_TAIL = [_P, _I, _P, _I]  # extra_features, n_extra, out_extra, sh_dtype
TABLE["gsr_rasterize_forward_ex"] = _variant("gsr_rasterize_forward", tail=_EX_TAIL)
TABLE["gsr_rasterize_forward_async_ex"] = _variant("gsr_rasterize_forward_async", tail=_EX_TAIL)
TABLE["gsr_rasterize_backward_ex"] = _variant("gsr_rasterize_backward", tail=[_P, _I, _PP, _P, _I])
TABLE["gsr_rasterize_backward_phase1_loss"] = _variant("gsr_rasterize_backward_ex", tail=[C.POINTER(Phase1LossStruct)])
# P, R, width, height, the three buffers, dL_dpix, dL_dcolor, n_extra, dL_dout_extra (host array), dL_dextra, debug
TABLE["gsr_rasterize_backward_colors"] = (_I, [_I] * 4 + [_P] * 5 + [_I, _PP, _P, _I], STREAM)
# joint-count (_nj, gsr_body_pose_*) and bone-count (_nb) variants: the same arguments after a leading count
for _n in ("gsr_lbs_forward", "gsr_lbs_forward_grid", "gsr_lbs_forward_cached", "gsr_lbs_backward"):
    TABLE[_n + "_nj"] = _variant(_n, lead=[_I])
for _n in ("forward", "backward"):
    TABLE["gsr_body_pose_" + _n] = _variant("gsr_smpl_pose_" + _n, lead=[_I])
for _n in ("gsr_lbs_offset_mlp_packed_floats", "gsr_lbs_offset_mlp_pack", "gsr_lbs_offset_mlp_forward",
           "gsr_debug_lbs_offset_mlp_forward_bf16x3", "gsr_lbs_offset_mlp_backward_workspace_floats", "gsr_lbs_offset_mlp_backward"):
    TABLE[_n + "_nb"] = _variant(_n, lead=[_I])

SYMBOLS = list(TABLE)  # every symbol include/gsr.h declares (tests check that the library exports all of them)

GSR_OK = 0
Q = dict(DEPTHS=0, MEANS2D=1, CONIC_OPACITY=2, RGB=3, COV3D=4, TILES_TOUCHED=5, POINT_OFFSETS=6, CLAMPED=7,
         POINT_LIST=8, KEYS_SORTED=9, RANGES=10, FINAL_T=11, N_CONTRIB=12, ORDER=13)
BINNING_GLOBAL_RADIX, BINNING_TILE_BUCKET = 0, 1
SH_F32, SH_F16 = 0, 1  # sh_dtype of the _ex entry points
N_EXTRA = 18  # extra feature channels of the fused multi-feature blend (six RGB triples)
DEFAULT_BINNING = BINNING_TILE_BUCKET
DEFAULT_TILE_CULL = 1  # tuning knob "tile_cull": exact ellipse-vs-tile culling in the tile-bucket back-end
DEFAULT_BWD_REDUCE = 3
DEFAULT_TILE_ORDER = 1  # tuning knob "tile_order" (csrc/gsr_common.h: Options)
DEFAULT_BLEND_LAYOUT = 0  # tuning knob "blend_layout"
DENSIFY_CLONE, DENSIFY_SPLIT, DENSIFY_MERGE = 0, 1, 2  # mode of gsr_densify_select
PLAN_PRUNE, PLAN_CLONE, PLAN_SPLIT, PLAN_MERGE = 0, 1, 2, 3  # kind of gsr_densify_plan
BUILD_MOVE, BUILD_CHILDREN, BUILD_MERGE = 0, 1, 2  # mode of gsr_build_rows
ROW_COPY, ROW_XYZ, ROW_LOG_SCALING, ROW_ROTATION, ROW_MEAN = 0, 1, 2, 3, 4  # role of an array in gsr_build_rows
ENV_TV_AUTO, ENV_TV_WINDOW, ENV_TV_WHOLE = 0, 1, 2  # gsr_pbr_env_tv_backward's reduce (include/gsr.h)
DEFAULT_BLEND_SEGMENTS = 8  # tuning knob "blend_segments": lists >= 8 / 4 x the frame's mean are walked in segments


class GsrError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP library first (python -m mygauhuman_amd.build, or "
            "__graft_entry__.build()).  There is no CPU/PyTorch fallback for the rasterizer.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes, streamed) in TABLE.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes + [C.c_void_p] * streamed
    return lib


lib = _load()


def check(rc, what):
    if rc != GSR_OK:
        msg = lib.gsr_last_error()
        raise GsrError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def call(name, device, *args, stream=None):
    """lib.<name>(*args, stream) on `device`, raising GsrError for a bad status: how every streamed entry point is launched.
    device None = the current device (no context is entered); stream None = the device's current stream, read now, else a raw
    handle or a torch.cuda.Stream."""
    if name not in TABLE:
        raise AttributeError(f"include/gsr.h declares no function {name}")
    if not TABLE[name][2]:
        raise TypeError(f"{name} takes no stream: call lib.{name} directly")
    stream = torch.cuda.current_stream(device).cuda_stream if stream is None else getattr(stream, "cuda_stream", stream)
    with contextlib.nullcontext() if device is None else torch.cuda.device(device):
        rc = getattr(lib, name)(*args, stream)
    check(rc, name)


def ptr(t):
    """Device pointer of a tensor, or None for an empty tensor (selects the other input mode, like the reference)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


PROF_STAGES = ["preprocess_fwd", "scan", "binning", "blend_fwd", "blend_bwd", "preprocess_bwd", "blend_bwd_colors"]


def profile_enable(stages):
    """stages: iterable of names from PROF_STAGES (empty = off)."""
    mask = 0
    for s in stages:
        mask |= 1 << PROF_STAGES.index(s)
    check(lib.gsr_profile_enable(mask), "gsr_profile_enable")
    check(lib.gsr_profile_reset(), "gsr_profile_reset")


def profile_read():
    """{stage: (total_ms, launches)} accumulated since profile_enable()."""
    out = {}
    for i, s in enumerate(PROF_STAGES):
        ms, n = C.c_double(0), C.c_long(0)
        check(lib.gsr_profile_read(i, C.byref(ms), C.byref(n)), "gsr_profile_read")
        out[s] = (ms.value, n.value)
    return out


def clock_probe(workgroups=1024, fmas=1 << 19, device=None):
    """Shader clock of the device right now, in GHz (gsr_debug_clock_probe; blocks until the probe kernel has run: ~2 ms at the
    default chain length).  Returns (GHz from s_memtime ticks over the constant 100 MHz counter, median over the workgroups;
    shader cycles per dependent v_fma_f32 of the chain: 8.8 on MI355X, a sanity value that does not move with the clock)."""
    import numpy as np
    out = torch.zeros(2 * workgroups, dtype=torch.int64, device=device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    call("gsr_debug_clock_probe", None, workgroups, fmas, out.data_ptr())
    v = out.cpu().numpy().reshape(workgroups, 2).astype(np.float64)
    ticks, cyc = float(np.median(v[:, 0])), float(np.median(v[:, 1]))
    if ticks <= 0:
        raise GsrError("gsr_debug_clock_probe: the 100 MHz counter did not advance")
    return cyc / (ticks * 10.0), cyc / fmas


def settle_clock(device=None, max_ms=1500.0, tol=0.004, probe_fmas=1 << 19, min_ms=0.0):
    """Run the clock probe back to back until five consecutive readings agree within `tol` (or max_ms have passed): brings a GPU
    that has just been handed to the process to the clock it sustains (2.26 -> 2.39 GHz over ~20 ms of load on MI355X; it falls
    back after ~50 ms of idle).  Returns the list of (ms since start, GHz) readings."""
    import time
    t0, hist = time.perf_counter(), []
    while True:
        ghz, _ = clock_probe(1024, probe_fmas, device)
        ms = (time.perf_counter() - t0) * 1e3
        hist.append((round(ms, 1), round(ghz, 4)))
        last = [h[1] for h in hist[-5:]]
        if (ms >= min_ms and len(last) == 5 and max(last) - min(last) <= tol * max(last)) or ms > max_ms:
            return hist


def set_tuning(key, value, stream=None):
    """Process default of a knob, or (stream = a torch.cuda.Stream / raw handle) that stream's own value."""
    if stream is None:
        check(lib.gsr_set_tuning(key.encode(), int(value)), "gsr_set_tuning")
    else:
        check(lib.gsr_set_stream_tuning(getattr(stream, "cuda_stream", stream), key.encode(), int(value)), "gsr_set_stream_tuning")


def clear_stream_tuning(stream):
    check(lib.gsr_clear_stream_tuning(getattr(stream, "cuda_stream", stream)), "gsr_clear_stream_tuning")
