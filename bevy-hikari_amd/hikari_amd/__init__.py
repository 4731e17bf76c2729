"""hikari_amd — MI355X-native drop-in for bevy-hikari's per-pixel integrator + SVGF denoiser.

Python host mirror of the reference's plugin API over the C ABI of libhikari_amd.so
(include/hikari_amd.h).  See DESIGN.md for the path, boundary and kernel layout.
"""
from . import _abi
from ._abi import HikariError
from .plugin import (HikariPlugin, HikariRenderer, PLAN_GBUFFER, PLAN_LIGHT, RESERVOIR_DTYPE, add_meshes_counts,
                     instance_descs, instance_set_counts, scene_gbuffer_stack, scene_indirect_lds, scene_stage_bytes,
                     set_meshes_counts, shared_transform)
from .scene import (AmbientLight, Camera, DirectionalLight, Mesh, Morph, Scene, Skin, StandardMaterial, Texture, Transform,
                    frame_inputs, jitter_mode, load_glb, load_noise, make_lights, plane_mesh, refit_boxes, refit_nodes, skin_vertices, morph_vertices,
                    texture_array,
                    uv_sphere_mesh)
from .cost import RefitPolicy, TreeCost, tree_cost
from .settings import HikariSettings, HikariUniversalSettings, PresentFormat, Taa, Upscale

__all__ = [
    "HikariError", "HikariPlugin", "HikariRenderer", "RESERVOIR_DTYPE", "AmbientLight", "Camera", "DirectionalLight",
    "Mesh", "Scene", "Skin", "skin_vertices", "Morph", "morph_vertices", "refit_nodes", "refit_boxes", "TreeCost", "tree_cost", "RefitPolicy", "StandardMaterial", "Texture", "texture_array", "Transform", "frame_inputs", "jitter_mode", "load_glb", "load_noise", "make_lights",
    "plane_mesh", "uv_sphere_mesh", "scene_stage_bytes", "scene_indirect_lds", "scene_gbuffer_stack", "shared_transform", "instance_descs", "instance_set_counts", "add_meshes_counts", "set_meshes_counts", "PLAN_LIGHT", "PLAN_GBUFFER", "HikariSettings", "HikariUniversalSettings", "PresentFormat", "Taa", "Upscale", "_abi",
]
