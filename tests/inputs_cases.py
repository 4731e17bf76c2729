"""Inputs the suite otherwise never renders, shared by tests/test_gpu_inputs.py (GPU against the oracle) and
tests/test_inputs_independent.py (the oracle against independent restatements, and the non-vacuity of every
settings case): fractional upscale ratios, orthographic cameras and HikariSettings at their edges."""
from __future__ import annotations

import math

# ------------------------------------------------------------------ orthographic cameras
# Vertical extents (world units; ScalingMode::FixedVertical, near 0, far 1000) that frame each example scene from
# its own camera position: cornell's box (2 x 2 around (0, 1, 0)) with a margin of background on every side, so
# that the silhouette and background pixels are in the frame; scene.rs's ground plane with the sphere and the
# small proxy buildings around the origin (its perspective camera sees little but the ground at this size).
ORTHO_HEIGHT = {"cornell": 2.4, "scene": 6.0}


def orthographic_camera(scene_fn: str, camera):
    """The example's camera (its Transform) with an orthographic projection framing the scene."""
    from hikari_amd import Camera
    return Camera.orthographic(camera.transform, ORTHO_HEIGHT[scene_fn])


# ------------------------------------------------------------------ settings at their edges
EDGE_BASE = dict(emissive_spatial_reuse=True, indirect_bounces=3, denoise=True)
EDGE_SCENES = ("scene", "cornell")  # scene.rs has the directional light
EDGE_SIZE = (48, 32)
EDGE_FRAMES = 5
# id -> HikariSettings fields over EDGE_BASE.  max_reservoir_lifetime = 0.0 is not here: spatial_reuse replaces a
# limit <= 1 by F32_MAX (light.wgsl:1570-1574 `select(max_reservoir_lifetime, F32_MAX, max_reservoir_lifetime <=
# 1.0)`), which no lifetime exceeds, exactly as the default 100 is never exceeded within a few frames (a
# reservoir's lifetime grows by one per frame), so 0.0 renders the base frames; 2.0 is exceeded from frame 2 on.
EDGE_CASES = {
    "validate_intervals_0": dict(direct_validate_interval=0, emissive_validate_interval=0),
    "temporal_count_0": dict(max_temporal_reuse_count=0),
    "temporal_count_1": dict(max_temporal_reuse_count=1),
    "spatial_count_0": dict(max_spatial_reuse_count=0),
    "spatial_count_1": dict(max_spatial_reuse_count=1),
    "indirect_luminance_0": dict(max_indirect_luminance=0.0),
    "indirect_luminance_small": dict(max_indirect_luminance=0.05),
    "reservoir_lifetime_2": dict(max_reservoir_lifetime=2.0),
    "bounces_0_spatial": dict(indirect_bounces=0, indirect_spatial_reuse=True),
    "bounces_8": dict(indirect_bounces=8),
    "solar_angle_0": dict(solar_angle=0.0),
    "solar_angle_1": dict(solar_angle=1.0),
    "clear_black": dict(clear_color=(0.0, 0.0, 0.0, 1.0)),
    "clear_orange": dict(clear_color=(1.0, 0.5, 0.25, 1.0)),
    "no_temporal_reuse": dict(temporal_reuse=False, emissive_spatial_reuse=True),
}
# the cases whose kernel variant the host picks per frame (validation_frame) or whose clamps run every frame:
# also rendered with the fused and the separate direct / emissive launches forced
EDGE_LAUNCH_CASES = ("validate_intervals_0", "temporal_count_0", "spatial_count_0")
EDGE_LAUNCH_OPTIONS = ({"fuse_min_px": 0, "merge": 0}, {"fuse": 0, "direct_w4_min_px": 0})

ORBIT_2_DEGREES = math.radians(2.0)


def edge_settings(case: str | None):
    from hikari_amd import HikariSettings, Upscale
    fields = dict(EDGE_BASE)
    if case is not None:
        fields.update(EDGE_CASES[case])
    return HikariSettings(upscale=Upscale.SMAA_TU_1_0, **fields)
