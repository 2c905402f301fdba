"""ctypes binding of libgsr.so (the C ABI declared in include/gsr.h).

There is NO fallback: if the HIP library is missing or does not load, importing this module raises."""
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


# every symbol include/gsr.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "gsr_version", "gsr_has_experiments", "gsr_target_arch", "gsr_last_error", "gsr_set_binning_mode", "gsr_get_binning_mode", "gsr_set_tuning", "gsr_set_stream_tuning", "gsr_clear_stream_tuning", "gsr_profile_enable", "gsr_profile_reset", "gsr_profile_read", "gsr_debug_wave_trace", "gsr_debug_clock_probe",
    "gsr_mark_visible", "gsr_rasterize_forward", "gsr_rasterize_backward", "gsr_query_state",
    "gsr_geometry_bytes", "gsr_image_bytes", "gsr_binning_bytes", "gsr_rasterize_forward_async",
    "gsr_alpha_mask_loss_backward", "gsr_phase1_loss_partials", "gsr_phase1_loss_forward", "gsr_rasterize_backward_phase1_loss", "gsr_rasterize_backward_alpha_mask_loss", "gsr_rasterize_forward_ex", "gsr_rasterize_forward_async_ex", "gsr_rasterize_backward_ex",
    "gsr_dist2_workspace_bytes", "gsr_dist2", "gsr_sort_workspace_bytes", "gsr_sort_pairs_u64",
    "gsr_sort_pairs_u32", "gsr_lbs_forward", "gsr_lbs_backward", "gsr_lbs_backward_workgroups", "gsr_lbs_workspace_bytes", "gsr_lbs_grid_build", "gsr_lbs_forward_grid", "gsr_lbs_forward_cached", "gsr_lbs_nn_cache_bytes", "gsr_smpl_pose_forward", "gsr_smpl_pose_backward", "gsr_sh_view_pack", "gsr_sh_grad_from_views", "gsr_sh_view_pack_posed", "gsr_sh_grad_from_views_posed", "gsr_step_status", "gsr_step_finish", "gsr_knn_self", "gsr_knn_nearest", "gsr_gather_rows", "gsr_ssim_forward", "gsr_ssim_backward", "gsr_gemv_rows", "gsr_gemv_rows_t", "gsr_frame_attributes_forward", "gsr_frame_attributes_backward", "gsr_model_activations_forward", "gsr_model_activations_backward", "gsr_frame_attributes_forward_split", "gsr_frame_attributes_backward_split", "gsr_frame_attributes_backward_acc", "gsr_model_activations_backward_acc", "gsr_lbs_offset_mlp_packed_floats", "gsr_lbs_offset_mlp_pack", "gsr_lbs_offset_mlp_forward", "gsr_lbs_offset_mlp_backward_workspace_floats", "gsr_lbs_offset_mlp_backward", "gsr_debug_lbs_offset_mlp_forward_bf16x3", "gsr_lbs_offset_mlp_set_precision",
    "gsr_lbs_forward_nj", "gsr_lbs_forward_grid_nj", "gsr_lbs_forward_cached_nj", "gsr_lbs_backward_nj", "gsr_body_pose_forward",
    "gsr_body_pose_backward", "gsr_lbs_offset_mlp_packed_floats_nb", "gsr_lbs_offset_mlp_pack_nb", "gsr_lbs_offset_mlp_forward_nb",
    "gsr_debug_lbs_offset_mlp_forward_bf16x3_nb", "gsr_lbs_offset_mlp_backward_workspace_floats_nb", "gsr_lbs_offset_mlp_backward_nb",
    "gsr_pbr_texture_forward", "gsr_pbr_texture_backward", "gsr_pbr_cube_mip_forward", "gsr_pbr_cube_mip_backward",
    "gsr_pbr_diffuse_forward", "gsr_pbr_diffuse_backward", "gsr_pbr_specular_forward", "gsr_pbr_specular_backward",
    "gsr_pbr_shade_forward", "gsr_pbr_shade_backward",
    "gsr_pbr_env_grey", "gsr_pbr_env_tv_workspace_floats", "gsr_pbr_env_tv_forward", "gsr_pbr_env_tv_backward", "gsr_pbr_view_dirs",
    "gsr_bake_grid_workspace_bytes", "gsr_bake_grid", "gsr_bake_plan_bytes", "gsr_bake_plan", "gsr_bake_visibility_workspace_bytes",
    "gsr_bake_visibility", "gsr_bake_expand", "gsr_bake_env_reduce",
    "gsr_pbr_loss_workspace_floats", "gsr_pbr_loss_forward", "gsr_pbr_loss_backward",
    "gsr_pose_refiner_forward", "gsr_pose_refiner_backward",
    "gsr_bounding_rect_workspace_ints", "gsr_bounding_rect", "gsr_ssim_crop_workspace_floats", "gsr_ssim_crop_forward",
    "gsr_ssim_crop_backward",
    "gsr_adam_chunk_floats", "gsr_adam_step", "gsr_stats_update",
    "gsr_eval_workspace_floats", "gsr_eval_view_finish",
]

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
    vp, fp, ip, sz = C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t  # device pointers travel as integers
    lib.gsr_version.restype = C.c_int
    lib.gsr_has_experiments.restype = C.c_int
    lib.gsr_target_arch.restype = C.c_char_p
    lib.gsr_last_error.restype = C.c_char_p
    lib.gsr_set_binning_mode.argtypes = [C.c_int]
    lib.gsr_get_binning_mode.restype = C.c_int
    lib.gsr_set_tuning.argtypes = [C.c_char_p, C.c_int]
    lib.gsr_set_stream_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.gsr_clear_stream_tuning.argtypes = [C.c_void_p]
    lib.gsr_set_stream_tuning.restype = lib.gsr_clear_stream_tuning.restype = C.c_int
    lib.gsr_profile_enable.argtypes = [C.c_uint]
    lib.gsr_debug_wave_trace.argtypes = [C.c_void_p, C.c_size_t]
    lib.gsr_debug_clock_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.gsr_debug_clock_probe.restype = C.c_int
    lib.gsr_profile_read.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    lib.gsr_mark_visible.argtypes = [C.c_int, fp, fp, fp, vp, vp]
    lib.gsr_rasterize_forward.argtypes = [
        ALLOC_FN, vp, ALLOC_FN, vp, ALLOC_FN, vp, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, fp, fp, fp, fp,
        C.c_float, fp, fp, fp, fp, fp, C.c_float, C.c_float, C.c_int, fp, fp, fp, ip, C.c_int, C.POINTER(C.c_int), vp]
    lib.gsr_rasterize_backward.argtypes = [
        C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, fp, fp, fp, fp, C.c_float, fp, fp, fp, fp, fp,
        C.c_float, C.c_float, ip, vp, vp, vp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, vp]
    lib.gsr_geometry_bytes.argtypes = [C.c_int]
    lib.gsr_geometry_bytes.restype = sz
    lib.gsr_image_bytes.argtypes = [C.c_int, C.c_int]
    lib.gsr_image_bytes.restype = sz
    lib.gsr_binning_bytes.argtypes = [sz, C.c_int, C.c_int]
    lib.gsr_binning_bytes.restype = sz
    lib.gsr_rasterize_forward_async.argtypes = [
        vp, vp, sz, vp, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, fp, fp, fp, fp, C.c_float, fp, fp, fp, fp, fp,
        C.c_float, C.c_float, C.c_int, fp, fp, fp, ip, C.c_int, vp, vp]
    lib.gsr_rasterize_forward_async.restype = C.c_int
    lib.gsr_alpha_mask_loss_backward.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp, C.c_float, fp, fp, vp]
    lib.gsr_alpha_mask_loss_backward.restype = C.c_int
    lib.gsr_rasterize_forward_ex.argtypes = lib.gsr_rasterize_forward.argtypes[:-1] + [fp, C.c_int, fp, C.c_int, vp]
    lib.gsr_rasterize_forward_async_ex.argtypes = lib.gsr_rasterize_forward_async.argtypes[:-1] + [fp, C.c_int, fp, C.c_int, vp]
    lib.gsr_rasterize_backward_ex.argtypes = lib.gsr_rasterize_backward.argtypes[:-1] + [fp, C.c_int, C.POINTER(C.c_void_p), fp, C.c_int, vp]
    lib.gsr_rasterize_backward_alpha_mask_loss.argtypes = (lib.gsr_rasterize_backward.argtypes[:24] + [fp, fp, fp, C.c_float] + [fp] * 9
                                                           + [C.c_int, C.c_int, vp])
    lib.gsr_phase1_loss_partials.restype = sz
    lib.gsr_phase1_loss_forward.argtypes = [C.c_int, C.c_int, C.POINTER(Phase1LossStruct), fp, vp]
    lib.gsr_phase1_loss_forward.restype = C.c_int
    lib.gsr_rasterize_backward_phase1_loss.argtypes = lib.gsr_rasterize_backward_ex.argtypes[:-1] + [C.POINTER(Phase1LossStruct), vp]
    for _n in ("gsr_rasterize_forward_ex", "gsr_rasterize_forward_async_ex", "gsr_rasterize_backward_ex",
               "gsr_rasterize_backward_alpha_mask_loss", "gsr_rasterize_backward_phase1_loss"):
        getattr(lib, _n).restype = C.c_int
    lib.gsr_query_state.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.gsr_dist2_workspace_bytes.argtypes = [C.c_int]
    lib.gsr_dist2_workspace_bytes.restype = sz
    lib.gsr_dist2.argtypes = [C.c_int, fp, fp, vp, sz, vp]
    lib.gsr_sort_workspace_bytes.argtypes = [sz]
    lib.gsr_sort_workspace_bytes.restype = sz
    lib.gsr_sort_pairs_u64.argtypes = [sz, vp, vp, vp, vp, C.c_int, vp, sz, vp]
    lib.gsr_sort_pairs_u32.argtypes = [sz, vp, vp, vp, vp, C.c_int, vp, sz, vp]
    lib.gsr_lbs_forward.argtypes = [C.c_int, C.c_int] + [fp] * 12 + [ip] + [fp] * 6 + [vp]
    lib.gsr_lbs_forward_grid.argtypes = [C.c_int, C.c_int] + [fp] * 12 + [ip] + [fp] * 6 + [vp, sz, C.c_int, vp]
    lib.gsr_lbs_forward_cached.argtypes = [C.c_int, C.c_int] + [fp] * 12 + [ip] + [fp] * 6 + [vp, sz, vp, sz, C.c_int, vp]
    lib.gsr_lbs_forward_cached.restype = C.c_int
    lib.gsr_lbs_nn_cache_bytes.argtypes = [C.c_int]
    lib.gsr_lbs_nn_cache_bytes.restype = sz
    lib.gsr_lbs_grid_build.argtypes = [C.c_int, fp, vp, sz, vp]
    lib.gsr_lbs_grid_build.restype = C.c_int
    lib.gsr_lbs_forward_grid.restype = C.c_int
    lib.gsr_lbs_workspace_bytes.argtypes = [C.c_int]
    lib.gsr_lbs_workspace_bytes.restype = sz
    lib.gsr_smpl_pose_forward.argtypes = [fp, fp, fp, C.POINTER(C.c_int), fp, fp, vp]
    lib.gsr_smpl_pose_backward.argtypes = [fp, fp, fp, C.POINTER(C.c_int)] + [fp] * 5 + [vp]
    lib.gsr_smpl_pose_forward.restype = lib.gsr_smpl_pose_backward.restype = C.c_int
    lib.gsr_sh_view_pack.argtypes = [C.c_int, vp, fp, fp, vp]
    lib.gsr_sh_grad_from_views.argtypes = [C.c_int] * 4 + [fp, fp, sz, C.c_float, fp, fp, vp]
    lib.gsr_sh_view_pack.restype = lib.gsr_sh_grad_from_views.restype = C.c_int
    lib.gsr_step_status.argtypes = [C.c_int, vp, fp, C.c_float, fp, vp, vp]
    lib.gsr_step_status.restype = C.c_int
    lib.gsr_sh_view_pack_posed.argtypes = [C.c_int, fp, fp, fp, fp, fp, sz, sz, vp]
    lib.gsr_sh_grad_from_views_posed.argtypes = [C.c_int, C.c_int, C.c_int, fp, sz, sz, sz, C.c_float, fp, fp, fp, vp]
    lib.gsr_step_finish.argtypes = [vp, fp, sz, sz, C.c_float, fp, vp, vp]
    lib.gsr_sh_view_pack_posed.restype = lib.gsr_sh_grad_from_views_posed.restype = lib.gsr_step_finish.restype = C.c_int
    lib.gsr_knn_self.argtypes = [C.c_int, fp, C.c_int, ip, fp, vp, sz, vp]
    lib.gsr_knn_nearest.argtypes = [C.c_int, fp, C.c_int, fp, ip, fp, vp, sz, vp]
    lib.gsr_knn_self.restype = lib.gsr_knn_nearest.restype = C.c_int
    lib.gsr_gather_rows.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.c_int, ip, vp]
    lib.gsr_gather_rows.restype = C.c_int
    lib.gsr_ssim_forward.argtypes = [C.c_int] * 3 + [fp] * 6 + [vp]
    lib.gsr_ssim_backward.argtypes = [C.c_int] * 3 + [fp] * 3 + [C.c_float] + [fp] * 4 + [vp]
    lib.gsr_ssim_forward.restype = lib.gsr_ssim_backward.restype = C.c_int
    lib.gsr_gemv_rows.argtypes = [C.c_int, C.c_int, fp, fp, fp, vp]
    lib.gsr_gemv_rows_t.argtypes = [C.c_int, C.c_int, fp, fp, fp, vp]
    lib.gsr_gemv_rows.restype = lib.gsr_gemv_rows_t.restype = C.c_int
    lib.gsr_lbs_backward.argtypes = [C.c_int, C.c_int, fp, fp, ip] + [fp] * 8 + [fp] * 3 + [fp] * 6 + [vp]
    # joint-count variants: the same arguments after a leading J
    for name in ("gsr_lbs_forward", "gsr_lbs_forward_grid", "gsr_lbs_forward_cached", "gsr_lbs_backward"):
        getattr(lib, name + "_nj").argtypes = [C.c_int] + getattr(lib, name).argtypes
        getattr(lib, name + "_nj").restype = C.c_int
    lib.gsr_body_pose_forward.argtypes = [C.c_int] + lib.gsr_smpl_pose_forward.argtypes
    lib.gsr_body_pose_backward.argtypes = [C.c_int] + lib.gsr_smpl_pose_backward.argtypes
    lib.gsr_body_pose_forward.restype = lib.gsr_body_pose_backward.restype = C.c_int
    lib.gsr_lbs_backward_workgroups.argtypes = [C.c_int]
    lib.gsr_lbs_backward_workgroups.restype = C.c_int
    lib.gsr_frame_attributes_forward.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_float] + [fp] * 8 + [fp] * 3 + [vp]
    lib.gsr_frame_attributes_backward.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_float] + [fp] * 8 + [fp] * 3 + [fp] * 10 + [vp]
    lib.gsr_frame_attributes_forward_split.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_float] + [fp] * 9 + [fp] * 3 + [vp]
    lib.gsr_frame_attributes_backward_split.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_float] + [fp] * 9 + [fp] * 3 + [fp] * 11 + [vp]
    lib.gsr_model_activations_forward.argtypes = [C.c_int] + [fp] * 11 + [vp]
    lib.gsr_model_activations_backward.argtypes = [C.c_int] + [fp] * 16 + [vp]
    lib.gsr_model_activations_backward_acc.argtypes = [C.c_int] + [fp] * 17 + [vp]
    lib.gsr_lbs_offset_mlp_packed_floats.argtypes = []
    lib.gsr_lbs_offset_mlp_packed_floats.restype = C.c_size_t
    lib.gsr_lbs_offset_mlp_pack.argtypes = [C.POINTER(fp), C.POINTER(fp), fp, vp]
    lib.gsr_lbs_offset_mlp_pack.restype = C.c_int
    lib.gsr_lbs_offset_mlp_forward.argtypes = [C.c_int, fp, fp, fp, vp]
    lib.gsr_lbs_offset_mlp_forward.restype = C.c_int
    lib.gsr_debug_lbs_offset_mlp_forward_bf16x3.argtypes = [C.c_int, fp, fp, fp, vp]
    lib.gsr_debug_lbs_offset_mlp_forward_bf16x3.restype = C.c_int
    lib.gsr_lbs_offset_mlp_set_precision.argtypes = [C.c_int]
    lib.gsr_lbs_offset_mlp_set_precision.restype = C.c_int
    lib.gsr_lbs_offset_mlp_backward_workspace_floats.argtypes = [C.c_int]
    lib.gsr_lbs_offset_mlp_backward_workspace_floats.restype = C.c_size_t
    lib.gsr_lbs_offset_mlp_backward.argtypes = [C.c_int, fp, fp, fp, fp, C.POINTER(fp), C.POINTER(fp), vp]
    lib.gsr_lbs_offset_mlp_backward.restype = C.c_int
    # bone-count variants: the same arguments after a leading nb (24 or 55)
    for name in ("gsr_lbs_offset_mlp_packed_floats", "gsr_lbs_offset_mlp_pack", "gsr_lbs_offset_mlp_forward",
                 "gsr_debug_lbs_offset_mlp_forward_bf16x3", "gsr_lbs_offset_mlp_backward_workspace_floats", "gsr_lbs_offset_mlp_backward"):
        getattr(lib, name + "_nb").argtypes = [C.c_int] + getattr(lib, name).argtypes
        getattr(lib, name + "_nb").restype = getattr(lib, name).restype
    pt = C.POINTER(PbrTexture)
    lib.gsr_pbr_texture_forward.argtypes = [pt, C.c_int, fp, fp, fp, vp]
    lib.gsr_pbr_texture_backward.argtypes = [pt, C.c_int, fp, fp, fp, fp, fp, vp]
    lib.gsr_pbr_cube_mip_forward.argtypes = lib.gsr_pbr_cube_mip_backward.argtypes = [C.c_int, C.c_int, fp, fp, vp]
    lib.gsr_pbr_diffuse_forward.argtypes = lib.gsr_pbr_diffuse_backward.argtypes = [C.c_int, fp, fp, vp]
    lib.gsr_pbr_specular_forward.argtypes = [C.c_int, C.c_float, C.c_float, fp, fp, fp, vp]
    lib.gsr_pbr_specular_backward.argtypes = [C.c_int, C.c_float, C.c_float, fp, fp, fp, vp]
    lib.gsr_pbr_shade_forward.argtypes = lib.gsr_pbr_shade_backward.argtypes = [C.POINTER(PbrShade), vp]
    for name in ("texture_forward", "texture_backward", "cube_mip_forward", "cube_mip_backward", "diffuse_forward",
                 "diffuse_backward", "specular_forward", "specular_backward", "shade_forward", "shade_backward"):
        getattr(lib, "gsr_pbr_" + name).restype = C.c_int
    lib.gsr_pbr_env_grey.argtypes = [C.c_int, fp, C.c_int, fp, fp, vp]
    lib.gsr_pbr_env_tv_workspace_floats.argtypes = [C.c_int, C.c_int]
    lib.gsr_pbr_env_tv_workspace_floats.restype = sz
    lib.gsr_pbr_env_tv_forward.argtypes = [C.c_int, fp, C.c_int, C.c_int, fp, fp, fp, vp]
    lib.gsr_pbr_env_tv_backward.argtypes = [C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, C.c_int, vp]
    lib.gsr_pbr_view_dirs.argtypes = [C.c_int, fp, fp, fp, vp]
    for name in ("env_grey", "env_tv_forward", "env_tv_backward", "view_dirs"):
        getattr(lib, "gsr_pbr_" + name).restype = C.c_int
    sz, u64p = C.c_size_t, C.POINTER(C.c_ulonglong)
    bs = C.POINTER(BakeScene)
    lib.gsr_bake_grid_workspace_bytes.argtypes = []
    lib.gsr_bake_grid_workspace_bytes.restype = sz
    lib.gsr_bake_grid.argtypes = [C.c_int, fp, fp, fp, fp, fp, C.POINTER(C.c_int), vp, sz, vp]
    lib.gsr_bake_plan_bytes.argtypes = [C.c_int, C.c_int]
    lib.gsr_bake_plan_bytes.restype = sz
    lib.gsr_bake_plan.argtypes = [bs, vp, sz, u64p, vp]
    lib.gsr_bake_visibility_workspace_bytes.argtypes = [C.c_int, sz]
    lib.gsr_bake_visibility_workspace_bytes.restype = sz
    lib.gsr_bake_visibility.argtypes = [bs, vp, fp, vp, sz, u64p, vp]
    lib.gsr_bake_expand.argtypes = [C.c_int, C.c_int, fp, fp, fp, fp, fp, vp]
    lib.gsr_bake_env_reduce.argtypes = [C.c_int, fp, fp, fp, vp]
    for name in ("grid", "plan", "visibility", "expand", "env_reduce"):
        getattr(lib, "gsr_bake_" + name).restype = C.c_int
    lib.gsr_pbr_loss_workspace_floats.argtypes = []
    lib.gsr_pbr_loss_workspace_floats.restype = sz
    lib.gsr_pbr_loss_forward.argtypes = [C.POINTER(PbrLoss), fp, vp]
    lib.gsr_pbr_loss_backward.argtypes = [C.POINTER(PbrLoss), fp, vp]
    lib.gsr_pbr_loss_forward.restype = lib.gsr_pbr_loss_backward.restype = C.c_int
    ll = C.c_longlong
    lib.gsr_pose_refiner_forward.argtypes = [C.c_int, C.c_int, C.c_int, fp, ll, ll, C.POINTER(fp), C.POINTER(fp), fp, vp]
    lib.gsr_pose_refiner_backward.argtypes = [C.c_int, C.c_int, C.c_int, fp, ll, ll, C.POINTER(fp), C.POINTER(fp), fp,
                                              C.POINTER(fp), C.POINTER(fp), fp, vp]
    lib.gsr_pose_refiner_forward.restype = lib.gsr_pose_refiner_backward.restype = C.c_int
    lib.gsr_bounding_rect_workspace_ints.argtypes = []
    lib.gsr_bounding_rect_workspace_ints.restype = sz
    lib.gsr_bounding_rect.argtypes = [C.c_int, C.c_int, vp, C.c_int, ip, ip, vp]
    lib.gsr_ssim_crop_workspace_floats.argtypes = [C.c_int] * 3
    lib.gsr_ssim_crop_workspace_floats.restype = sz
    lib.gsr_ssim_crop_forward.argtypes = [C.POINTER(SsimCrop), fp, vp]
    lib.gsr_ssim_crop_backward.argtypes = [C.POINTER(SsimCrop), vp]
    lib.gsr_bounding_rect.restype = lib.gsr_ssim_crop_forward.restype = lib.gsr_ssim_crop_backward.restype = C.c_int
    lib.gsr_adam_chunk_floats.argtypes = []
    lib.gsr_adam_step.argtypes = [C.c_int, C.POINTER(AdamArray), C.c_int, C.POINTER(AdamGroup), fp, fp, C.POINTER(AdamStats),
                                  C.c_int, vp]
    lib.gsr_stats_update.argtypes = [C.POINTER(AdamStats), C.c_int, vp]
    lib.gsr_adam_chunk_floats.restype = lib.gsr_adam_step.restype = lib.gsr_stats_update.restype = C.c_int
    lib.gsr_eval_workspace_floats.argtypes = [C.c_int, C.c_int]
    lib.gsr_eval_workspace_floats.restype = sz
    lib.gsr_eval_view_finish.argtypes = [C.POINTER(EvalView), fp, vp]
    lib.gsr_eval_view_finish.restype = C.c_int
    lib.gsr_frame_attributes_backward_acc.argtypes = [C.c_int] * 3 + [fp] * 4 + [C.c_float] + [fp] * 9 + [fp] * 3 + [fp] * 11 + [fp] + [vp]
    for name in ("gsr_frame_attributes_forward", "gsr_frame_attributes_backward", "gsr_model_activations_forward", "gsr_model_activations_backward", "gsr_frame_attributes_forward_split", "gsr_frame_attributes_backward_split", "gsr_frame_attributes_backward_acc", "gsr_model_activations_backward_acc", "gsr_set_binning_mode", "gsr_set_tuning", "gsr_mark_visible", "gsr_rasterize_forward",
                 "gsr_rasterize_backward", "gsr_query_state", "gsr_dist2", "gsr_sort_pairs_u64", "gsr_sort_pairs_u32",
                 "gsr_lbs_forward", "gsr_lbs_backward"):
        getattr(lib, name).restype = C.c_int
    return lib


lib = _load()


def check(rc, what):
    if rc != GSR_OK:
        msg = lib.gsr_last_error()
        raise GsrError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a tensor, or None for an empty tensor (selects the other input mode, like the reference)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


PROF_STAGES = ["preprocess_fwd", "scan", "binning", "blend_fwd", "blend_bwd", "preprocess_bwd"]


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
    check(lib.gsr_debug_clock_probe(workgroups, fmas, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "gsr_debug_clock_probe")
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
