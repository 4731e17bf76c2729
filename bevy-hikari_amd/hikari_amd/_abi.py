"""ctypes mirror of include/hikari_amd.h and include/hikari_scene.h.

The product path is libhikari_amd.so (HIP kernels for gfx950).  Loading fails loudly if the
library is missing: there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["HK_LIB"]) if os.environ.get("HK_LIB") else HERE / "libhikari_amd.so"  # HK_LIB: experiment builds

HK_OK = 0
HK_ERR_INVALID = -1
HK_ERR_HIP = -2
HK_ERR_STATE = -3
HK_ERR_NO_DEVICE = -4

RESERVOIR_BUFFERS = 10  # HK_RESERVOIR_BUFFERS

# enum hk_math_fn in its order (HK_MATH_<NAME>; tests/test_math_cases.py compares this list with the header)
MATH_FN_NAMES = (
    "exp2", "exp", "exp_weight", "log2", "pow", "pow2", "pow5", "pow16", "sincos",
    "unorm16", "snorm8", "unpack_unorm16_fast", "unpack_snorm8_fast", "unorm8_fast", "random_float",
    "fract", "minf", "maxf", "saturate", "signf",
    "div", "sqrt", "rcp_exact", "rcp_fast", "div_by", "f2u32", "f2i32", "unpack_f16",
)
MATH_FN = {name: i for i, name in enumerate(MATH_FN_NAMES)}
MATH_FN_TWO_OPERANDS = ("pow", "unpack_snorm8_fast", "minf", "maxf", "div", "div_by")
MATH_FN_TWO_RESULTS = ("sincos", "unpack_f16")

# hk_output_id
OUT_ALBEDO = 0
OUT_VARIANCE = (1, 2, 3)
OUT_RENDER = (4, 5, 6)
OUT_DENOISED = (7, 8, 9)
OUT_TONE_MAPPED = 10
OUT_GBUF_POSITION = 11
OUT_GBUF_NORMAL = 12
OUT_GBUF_DEPTH_GRADIENT = 13
OUT_GBUF_INSTANCE_MATERIAL = 14
OUT_GBUF_VELOCITY_UV = 15
OUT_ACCUMULATED = 17
OUT_UPSCALED = 18
OUT_TAA = 19
OUT_TONE_MAPPED_PREVIOUS = 20
OUT_FSR_EASU = 21  # FSR1: upscale_output[0], S
OUT_FSR_RCAS = 22  # FSR1: upscale_output[1], S (the displayed frame)
OUT_DENOISE_INTERNAL_VARIANCE = 16
RESERVOIR_BUFFERS = 10


class hk_array(C.Structure):
    _fields_ = [("data", C.c_void_p), ("count", C.c_uint32)]


class hk_scene_desc(C.Structure):
    _fields_ = [(n, hk_array) for n in ("vertices", "primitives", "asset_nodes", "alias_table", "instances",
                                       "instance_nodes", "materials", "emissive_nodes", "emissives")]


class hk_mesh_index(C.Structure):
    """include/hk_types.h hk_mesh_index (GpuMeshIndex: a mesh's slices of the vertex, primitive and asset-node arrays)."""
    _fields_ = [("vertex", C.c_uint32), ("primitive", C.c_uint32), ("node", C.c_uint32 * 2)]


class hk_mesh_update(C.Structure):
    """include/hikari_amd.h hk_mesh_update (one deformed mesh of hk_update_meshes)."""
    _fields_ = [("mesh", hk_mesh_index), ("vertex_count", C.c_uint32), ("positions", C.c_void_p),
                ("normals", C.c_void_p)]


class hk_mesh_desc(C.Structure):
    """include/hikari_amd.h hk_mesh_desc (one new mesh of hk_add_meshes, as hks_add_mesh takes it)."""
    _fields_ = [("positions", C.c_void_p), ("normals", C.c_void_p), ("uvs", C.c_void_p), ("vertex_count", C.c_uint32),
                ("indices", C.c_void_p), ("index_count", C.c_uint32), ("topology", C.c_uint32)]


class hk_mesh_entry(C.Structure):
    """include/hikari_amd.h hk_mesh_entry (one entry of hk_set_meshes' list: a new mesh, or a kept slice)."""
    _fields_ = [("source", C.POINTER(hk_mesh_desc)), ("keep", hk_mesh_index), ("vertex_count", C.c_uint32)]


class hk_mesh_skin(C.Structure):
    """include/hikari_amd.h hk_mesh_skin (one mesh's bind pose and rig for hk_set_mesh_skins)."""
    _fields_ = [("mesh", hk_mesh_index), ("vertex_count", C.c_uint32), ("positions", C.c_void_p),
                ("normals", C.c_void_p), ("joint_indices", C.c_void_p), ("joint_weights", C.c_void_p),
                ("joint_count", C.c_uint32)]


class hk_skin_pose(C.Structure):
    """include/hikari_amd.h hk_skin_pose (one mesh's joint palette for hk_skin_meshes)."""
    _fields_ = [("mesh", hk_mesh_index), ("joints", C.c_void_p), ("joint_count", C.c_uint32)]


class hk_mesh_morph(C.Structure):
    """include/hikari_amd.h hk_mesh_morph (one mesh's base and target-major deltas for hk_set_mesh_morphs)."""
    _fields_ = [("mesh", hk_mesh_index), ("vertex_count", C.c_uint32), ("positions", C.c_void_p),
                ("normals", C.c_void_p), ("target_count", C.c_uint32), ("position_deltas", C.c_void_p),
                ("normal_deltas", C.c_void_p)]


class hk_morph_pose(C.Structure):
    """include/hikari_amd.h hk_morph_pose (one mesh's target weights, and its joint palette or NULL, for hk_morph_meshes)."""
    _fields_ = [("mesh", hk_mesh_index), ("weights", C.c_void_p), ("target_count", C.c_uint32), ("joints", C.c_void_p),
                ("joint_count", C.c_uint32)]


HK_MORPH_MAX_TARGETS = 256
HK_INSTANCE_NEW = 0xFFFFFFFF


class hk_instance_desc(C.Structure):
    """include/hikari_amd.h hk_instance_desc (one instance of hk_set_instances' new set)."""
    _fields_ = [("mesh", hk_mesh_index), ("material", C.c_uint32), ("previous", C.c_uint32)]


class hk_texture(C.Structure):
    """include/hikari_amd.h hk_texture (one GpuImage level 0 + its sampler)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("address_u", C.c_uint32),
                ("address_v", C.c_uint32), ("filter", C.c_uint32), ("rgba8", C.c_void_p)]


TEXTURE_RGBA8_SRGB, TEXTURE_RGBA8_UNORM = 0, 1
ADDRESS_CLAMP_TO_EDGE, ADDRESS_REPEAT, ADDRESS_MIRROR_REPEAT = 0, 1, 2
FILTER_NEAREST, FILTER_LINEAR = 0, 1


class hk_settings(C.Structure):
    _fields_ = [
        ("direct_validate_interval", C.c_uint32),
        ("emissive_validate_interval", C.c_uint32),
        ("max_temporal_reuse_count", C.c_uint32),
        ("max_spatial_reuse_count", C.c_uint32),
        ("max_reservoir_lifetime", C.c_float),
        ("solar_angle", C.c_float),
        ("indirect_bounces", C.c_uint32),
        ("max_indirect_luminance", C.c_float),
        ("clear_color", C.c_float * 4),
        ("temporal_reuse", C.c_uint32),
        ("emissive_spatial_reuse", C.c_uint32),
        ("indirect_spatial_reuse", C.c_uint32),
        ("denoise", C.c_uint32),
        ("taa", C.c_uint32),
        ("upscale_ratio", C.c_float),
        ("upscale", C.c_uint32),
    ]


class hk_view(C.Structure):
    _fields_ = [
        ("world_position", C.c_float * 3),
        ("_pad0", C.c_float),
        ("view_proj", C.c_float * 16),
        ("inverse_view_proj", C.c_float * 16),
        ("projection", C.c_float * 16),
    ]


class hk_lights(C.Structure):
    _fields_ = [
        ("directional_color", C.c_float * 4),
        ("direction_to_light", C.c_float * 3),
        ("_pad0", C.c_float),
        ("ambient_color", C.c_float * 4),
    ]


JITTER_NONE, JITTER_TAA, JITTER_TAA_SMAA = 0, 1, 2


class hk_frame_inputs(C.Structure):
    _fields_ = [("frame_number", C.c_uint32), ("jitter", C.c_uint32), ("has_previous_view", C.c_uint32),
                ("_pad", C.c_uint32), ("view", hk_view), ("lights", hk_lights),
                ("previous_view_proj", C.c_float * 16)]


PRESENT_RGBA8_SRGB, PRESENT_BGRA8_SRGB, PRESENT_RGBA16F = 0, 1, 2


class hk_present_target(C.Structure):
    """include/hikari_amd.h hk_present_target (the view target of hk_present)."""
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("pitch", C.c_uint32),
                ("format", C.c_uint32), ("vp_x", C.c_uint32), ("vp_y", C.c_uint32), ("vp_w", C.c_uint32),
                ("vp_h", C.c_uint32), ("input", C.c_int32)]


class hk_tree_cost(C.Structure):
    """include/hikari_amd.h hk_tree_cost (hk_tree_costs, hks_tree_cost; the rule: include/hk_cost.h)."""
    _fields_ = [("inner", C.c_uint64), ("leaf", C.c_uint64), ("root_half_area", C.c_float), ("entries", C.c_uint32)]


class hk_counters(C.Structure):
    _fields_ = [("traverse_top", C.c_uint64), ("traverse_emitter", C.c_uint64), ("primary", C.c_uint64),
                ("primary_reused", C.c_uint64)]


# std430 record sizes (include/hk_types.h)
SIZEOF = {"vertex": 32, "primitive": 48, "node": 32, "alias": 8, "instance": 176, "material": 80, "emissive": 64,
          "reservoir": 64}


class HikariError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load libhikari_amd.so (built by `make -C bevy-hikari_amd`). Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise HikariError(f"{LIB_PATH} is missing: build it with `make -C bevy-hikari_amd` "
                          "(no CPU fallback exists for the integrator)")
    L = C.CDLL(str(LIB_PATH))
    vp, i32, u32 = C.c_void_p, C.c_int, C.c_uint32
    sig = {
        "hk_abi_version": (i32, []),
        "hk_create": (i32, [i32, C.POINTER(vp)]),
        "hk_destroy": (None, [vp]),
        "hk_last_error": (C.c_char_p, [vp]),
        "hk_settings_default": (None, [C.POINTER(hk_settings)]),
        "hk_set_option": (i32, [vp, C.c_char_p, C.c_double]),
        "hk_get_option": (i32, [vp, C.c_char_p, C.POINTER(C.c_double)]),
        "hk_option_name": (C.c_char_p, [i32]),
        "hk_scene_upload": (i32, [vp, C.POINTER(hk_scene_desc)]),
        "hk_scene_stage_bytes": (i32, [C.POINTER(hk_scene_desc), i32, C.POINTER(u32), C.POINTER(u32)]),
        "hk_scene_indirect_lds": (i32, [C.POINTER(hk_scene_desc), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "hk_scene_gbuffer_stack": (i32, [C.POINTER(hk_scene_desc), C.POINTER(u32), C.POINTER(u32)]),
        "hk_set_noise": (i32, [vp, vp, u32, u32]),
        "hk_texture_upload": (i32, [vp, vp, u32]),
        "hk_resize": (i32, [vp, u32, u32, C.c_float, u32, u32]),
        "hk_set_band_halo": (i32, [vp, u32]),
        "hk_resize_striped": (i32, [vp, u32, u32, u32, u32]),
        "hk_band_info": (i32, [vp] + [C.POINTER(C.c_int32)] * 4),
        "hk_band_window_grow": (i32, [vp, C.POINTER(hk_settings), vp, i32]),
        "hk_resize_tile": (i32, [vp, u32, u32, u32, u32, u32, u32]),
        "hk_tile_info": (i32, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "hk_copy_output_rect": (i32, [vp, i32, u32, u32, u32, u32, vp, C.c_size_t, i32, vp]),
        "hk_reservoir_rows": (i32, [vp, i32, C.c_int32, C.c_int32, vp, i32, vp]),
        "hk_copy_output_rows": (i32, [vp, i32, u32, u32, vp, i32, vp]),
        "hk_render_gbuffer": (i32, [vp, C.POINTER(hk_frame_inputs), vp]),
        "hk_set_gbuffer_plane": (i32, [vp, i32, vp, C.c_size_t, i32, vp]),
        "hk_render_frame": (i32, [vp, C.POINTER(hk_settings), C.POINTER(hk_frame_inputs), vp]),
        "hk_denoise": (i32, [vp, C.POINTER(hk_settings), C.POINTER(hk_frame_inputs), vp]),
        "hk_tone_sum": (i32, [vp, C.POINTER(hk_settings), vp]),
        "hk_accumulate": (i32, [vp, i32, vp]),
        "hk_post_process": (i32, [vp, C.POINTER(hk_settings), C.POINTER(hk_frame_inputs), vp]),
        "hk_set_fsr1_sharpness": (i32, [vp, C.c_float]),
        "hk_present": (i32, [vp, C.POINTER(hk_settings), C.POINTER(hk_present_target), vp]),
        "hk_present_info": (i32, [vp] + [C.POINTER(u32)] * 4),
        "hk_get_present": (i32, [vp, vp, C.c_size_t, i32, vp]),
        "hk_update_instances": (i32, [vp, vp, vp, u32, vp]),
        "hk_update_meshes": (i32, [vp, C.POINTER(hk_mesh_update), u32, vp, vp, u32, vp]),
        "hk_set_instances": (i32, [vp, C.POINTER(hk_instance_desc), vp, vp, u32, vp, vp]),
        "hk_scene_counts": (i32, [vp, C.POINTER(u32)]),
        "hk_add_meshes": (i32, [vp, C.POINTER(hk_mesh_desc), u32, C.POINTER(hk_mesh_index), vp]),
        "hk_add_meshes_counts": (i32, [C.POINTER(u32), C.POINTER(hk_mesh_desc), u32, C.POINTER(hk_mesh_index),
                                       C.POINTER(u32)]),
        "hk_add_meshes_counts_error": (C.c_char_p, []),
        "hk_scene_capacity": (i32, [vp, C.POINTER(u32)]),
        "hk_set_meshes": (i32, [vp, C.POINTER(hk_mesh_entry), u32, C.POINTER(hk_mesh_index),
                                C.POINTER(hk_instance_desc), vp, vp, u32, vp, vp]),
        "hk_set_meshes_counts": (i32, [C.POINTER(u32), C.POINTER(hk_mesh_entry), u32, C.POINTER(hk_mesh_index),
                                       C.POINTER(u32)]),
        "hk_set_meshes_counts_error": (C.c_char_p, []),
        "hk_set_mesh_skins": (i32, [vp, C.POINTER(hk_mesh_skin), u32, vp]),
        "hk_skin_meshes": (i32, [vp, C.POINTER(hk_skin_pose), u32, vp, vp, u32, vp]),
        "hk_refit_meshes": (i32, [vp, C.POINTER(hk_mesh_update), u32, vp, vp, u32, vp]),
        "hk_skin_meshes_refit": (i32, [vp, C.POINTER(hk_skin_pose), u32, vp, vp, u32, vp]),
        "hk_refit_instances": (i32, [vp, vp, vp, u32, vp]),
        "hk_refit_meshes_all": (i32, [vp, C.POINTER(hk_mesh_update), u32, vp, vp, u32, vp]),
        "hk_skin_meshes_refit_all": (i32, [vp, C.POINTER(hk_skin_pose), u32, vp, vp, u32, vp]),
        "hk_set_mesh_morphs": (i32, [vp, C.POINTER(hk_mesh_morph), u32, vp]),
        "hk_morph_meshes": (i32, [vp, C.POINTER(hk_morph_pose), u32, vp, vp, u32, vp]),
        "hk_morph_meshes_refit": (i32, [vp, C.POINTER(hk_morph_pose), u32, vp, vp, u32, vp]),
        "hk_morph_meshes_refit_all": (i32, [vp, C.POINTER(hk_morph_pose), u32, vp, vp, u32, vp]),
        "hk_tree_costs": (i32, [vp, C.POINTER(u32), u32] + [C.POINTER(hk_tree_cost)] * 3 + [vp]),
        "hk_scene_shared_transform": (i32, [vp, C.POINTER(i32)]),
        "hk_instance_set_counts": (i32, [C.POINTER(hk_scene_desc), C.POINTER(hk_instance_desc), u32, vp, C.POINTER(u32)]),
        "hk_read_scene_array": (i32, [vp, i32, vp, C.c_size_t]),
        "hk_resolve_accumulation": (i32, [vp, vp]),
        "hk_output_info": (i32, [vp, i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "hk_get_output": (i32, [vp, i32, vp, C.c_size_t, i32, vp]),
        "hk_output_device_ptr": (vp, [vp, i32]),
        "hk_sync": (i32, [vp, vp]),
        "hk_set_wavefront": (i32, [vp, i32]),
        "hk_lane_stats": (i32, [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), i32]),
        "hk_dump_reservoirs": (i32, [vp, i32, vp, C.c_size_t, vp]),
        "hk_load_reservoirs": (i32, [vp, i32, vp, C.c_size_t, vp]),
        "hk_reset_counters": (i32, [vp, vp]),
        "hk_read_counters": (i32, [vp, C.POINTER(hk_counters), vp]),
        "hk_enable_kernel_timing": (i32, [vp, i32]),
        "hk_kernel_timing": (i32, [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]),
        "hk_set_kernel_timing_interval": (i32, [vp, u32]),
        "hk_trace": (i32, [vp, vp, vp, vp, vp, u32, vp, i32, vp]),
        "hk_selftest_f16": (i32, [vp, vp, u32, vp]),
        "hk_selftest_div": (i32, [vp, C.c_float, u32, u32, C.POINTER(C.c_uint64)]),
        "hk_selftest_rcp": (i32, [vp, u32, u32, C.POINTER(C.c_uint64)]),
        "hk_selftest_count": (i32, [vp, vp, u32, C.POINTER(C.c_uint64)]),
        "hk_selftest_texture": (i32, [vp, u32, vp, u32, vp]),
        "hk_selftest_math": (i32, [vp, i32, vp, vp, u32, vp, vp]),
        "hks_create": (vp, []),
        "hks_destroy": (None, [vp]),
        "hks_last_error": (C.c_char_p, [vp]),
        "hks_add_mesh": (i32, [vp, vp, vp, vp, u32, vp, u32, i32]),
        "hks_add_material": (i32, [vp, vp]),
        "hks_add_instance": (i32, [vp, u32, u32, vp]),
        "hks_build": (i32, [vp, i32]),
        "hks_get_desc": (i32, [vp, C.POINTER(hk_scene_desc)]),
        "hks_shared_transform": (i32, [vp, u32]),
        "hks_instance_bounds": (i32, [vp, vp, u32, C.POINTER(C.c_double)]),
        "hks_screen_bounds": (i32, [C.POINTER(C.c_double), C.POINTER(hk_view), u32, u32, u32, C.POINTER(i32)]),
        "hk_tile_skip_info": (i32, [vp, C.POINTER(u32), C.POINTER(i32), C.POINTER(i32)]),
        "hk_tone_skip_info": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(i32)]),
        "hks_tone_rect": (i32, [C.POINTER(i32), C.POINTER(i32), i32, u32, C.POINTER(i32)]),
        "hks_keep_tiles": (i32, [C.POINTER(i32), C.POINTER(i32), i32, u32, C.POINTER(u32)]),
        "hks_skin_vertices": (i32, [vp, vp, vp, vp, u32, vp, u32, vp, vp, vp]),
        "hks_morph_vertices": (i32, [vp, vp, vp, vp, u32, vp, u32, vp, vp, vp]),
        "hks_refit_nodes": (i32, [vp, u32, vp, u32]),
        "hks_refit_boxes": (i32, [vp, u32, vp, u32]),
        "hks_tree_cost": (i32, [vp, u32, C.POINTER(hk_tree_cost)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


# symbols include/*.h declare (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "hk_abi_version", "hk_create", "hk_destroy", "hk_last_error", "hk_settings_default", "hk_set_option",
    "hk_get_option", "hk_option_name", "hk_scene_upload", "hk_scene_stage_bytes", "hk_scene_indirect_lds",
    "hk_scene_gbuffer_stack",
    "hk_set_noise", "hk_texture_upload", "hk_resize", "hk_resize_striped", "hk_set_band_halo", "hk_band_info", "hk_band_window_grow", "hk_reservoir_rows", "hk_resize_tile", "hk_tile_info", "hk_copy_output_rect", "hk_copy_output_rows", "hk_render_gbuffer", "hk_set_gbuffer_plane", "hk_render_frame",
    "hk_denoise", "hk_tone_sum", "hk_update_instances", "hk_update_meshes", "hk_set_instances", "hk_scene_counts", "hk_instance_set_counts", "hk_read_scene_array", "hk_post_process", "hk_set_fsr1_sharpness", "hk_present", "hk_present_info", "hk_get_present", "hk_accumulate", "hk_resolve_accumulation", "hk_output_info", "hk_get_output", "hk_output_device_ptr", "hk_sync", "hk_set_wavefront", "hk_lane_stats", "hk_dump_reservoirs",
    "hk_load_reservoirs", "hk_reset_counters", "hk_read_counters", "hk_enable_kernel_timing", "hk_kernel_timing", "hk_set_kernel_timing_interval",
    "hk_trace", "hk_selftest_f16", "hk_selftest_div", "hk_selftest_rcp", "hk_selftest_count", "hk_selftest_texture", "hk_selftest_math", "hks_create", "hks_destroy", "hks_last_error", "hks_add_mesh", "hks_add_material",
    "hks_add_instance", "hks_build", "hks_get_desc", "hk_scene_shared_transform", "hks_shared_transform",
    "hks_instance_bounds", "hks_screen_bounds", "hk_tile_skip_info", "hk_tone_skip_info", "hks_tone_rect", "hks_keep_tiles",
    "hk_add_meshes", "hk_add_meshes_counts", "hk_add_meshes_counts_error", "hk_scene_capacity",
    "hk_set_meshes", "hk_set_meshes_counts", "hk_set_meshes_counts_error",
    "hk_set_mesh_skins", "hk_skin_meshes", "hks_skin_vertices",
    "hk_refit_meshes", "hk_skin_meshes_refit", "hks_refit_nodes",
    "hk_refit_instances", "hk_refit_meshes_all", "hk_skin_meshes_refit_all", "hks_refit_boxes",
    "hk_tree_costs", "hks_tree_cost",
    "hk_set_mesh_morphs", "hk_morph_meshes", "hk_morph_meshes_refit", "hk_morph_meshes_refit_all", "hks_morph_vertices",
]


def gpu_visible() -> bool:
    """True when a HIP device may be present (never initialises the GPU itself)."""
    return bool(os.environ.get("HIP_VISIBLE_DEVICES", "x")) and Path("/dev/kfd").exists()
