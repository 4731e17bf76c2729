"""A ladder of small scenes whose sizes sit on the edges of the kernels' LDS scene staging, shared by
tests/test_scene_ladder.py (CPU: every rung's position from hk_scene_stage_bytes, the emitter conditions from the
oracle), tests/test_gpu_scene_sizes.py (GPU parity on every rung) and the independent restatements.

L = the bytes the light passes stage (PLAN_LIGHT: all nine scene arrays), G = the bytes the G-buffer walk stages
(PLAN_GBUFFER: vertices, primitives, instances and the two wide node layouts), each array rounded up to 16 bytes.
stage_scene copies 4 x 256 chunks of 16 bytes per round (16384 bytes), a plan is staged up to LDS_SCENE_MAX = 32768
bytes, and the G-buffer's LDS stack follows a staged scene only while G + levels * 2048 <= 49152.

Every scene is a floor and a back wall (two instances of one plane mesh), a few boxes (examples.box_grid_mesh),
N emissive slabs above them (triangle strips tilted towards the camera, with different colours, positions and
triangle counts), and what moves a size without changing the picture much: the last box's triangle count (past its
grid, L 240 and G 336 bytes per triangle), unused
materials (L 80 bytes each) and small extra instances of the first box ("chips": L 272, G 368 bytes each).  The
camera is cornell.rs's; there is no directional light.  The counts below were found by a search over these three
axes against hk_scene_stage_bytes and are exact: no rung is off its target size.
"""
from __future__ import annotations

import math

import numpy as np

from parity import canon_frame, passes

SEED = 0x4C414444  # "LADD"

# rung -> emitters: triangles per slab; boxes: triangles per box (the last one is the size axis); materials: unused
# extra materials; chips: extra instances of box 0; strip: triangles of a fence of geometrically growing triangles
# (a deep BLAS).  The sizes hk_scene_stage_bytes must report for each: tests/test_scene_ladder.py EXPECTED
RUNGS = {
    # no emissive material: alias_table, emissive_nodes and emissives are empty (bytes[3] = bytes[7] = bytes[8] = 0)
    "no_emitters": dict(emitters=[], boxes=[12, 20], materials=0, chips=0),
    # one emitter of 5 triangles: a 40-byte alias table, the last non-empty array before a padded chunk
    "odd_alias": dict(emitters=[5], boxes=[12, 20], materials=0, chips=0),
    # light BVH with inner nodes, alias offsets 0, 3 and 8
    "emitters_3": dict(emitters=[3, 5, 7], boxes=[12, 16], materials=0, chips=0),
    # one instance of a one-triangle emissive mesh: 1-node TLAS, 1-node BLAS (no floor, wall or box)
    "one_triangle": dict(emitters=[1], boxes=[], materials=0, chips=0, floor=False),
    # L == 16384: exactly 1024 chunks, the last chunk of stage_scene's first round
    "round_edge": dict(emitters=[4, 6], boxes=[12, 20, 16], materials=0, chips=5),
    # L == 16384 + 16: one chunk in the second round
    "two_rounds": dict(emitters=[4, 6], boxes=[12, 20, 18], materials=1, chips=3),
    # L = 24016: 16384 < L < 32768 and L / 16 = 1501 (no multiple of 256), a partial second round
    "mid": dict(emitters=[3, 5, 7], boxes=[20, 24, 34], materials=1, chips=1),
    # L == 32768, the last staged size, and one chunk more, the first unstaged one (G is above its limit in both)
    "light_at_limit": dict(emitters=[3, 5, 7], boxes=[24, 30, 20, 42], materials=1, chips=0),
    "light_over_limit": dict(emitters=[3, 5, 7], boxes=[24, 30, 20, 39], materials=0, chips=3),
    # G == 32768 with L = 32800 above its limit (only the G-buffer plan stages); G == 32768 + 16 with L = 24400
    # (only the light plan stages)
    "gbuffer_at_limit": dict(emitters=[3, 5, 7], boxes=[20, 24, 17], materials=104, chips=18),
    "gbuffer_over_limit": dict(emitters=[3, 5, 7], boxes=[20, 24, 28], materials=0, chips=8),
    # G = 29712 staged, stack bound 13 <= 16 levels, 29712 + 13 * 2048 = 56336 > 49152: the staged walk without an LDS stack
    "gbuffer_no_stack_room": dict(emitters=[3], boxes=[12, 30], materials=0, chips=0, strip=40),
}


def _slab_mesh(triangles: int, hx: float, hz: float):
    """A triangle strip of `triangles` triangles between the rails z = -hz and z = +hz over x in [-hx, hx], in the
    plane y = 0 with the normal -y (an emitter shining down), as a triangle list."""
    from hikari_amd import Mesh
    n = triangles + 2
    cols = (n + 1) // 2
    pos = np.zeros((n, 3), np.float32)
    for k in range(n):
        pos[k] = [-hx + 2.0 * hx * (k // 2) / max(1, cols - 1), 0.0, -hz if k % 2 == 0 else hz]
    idx = []
    for k in range(triangles):
        idx += [k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2]
    nrm = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (n, 1))
    uv = np.stack([(pos[:, 0] + hx) / (2 * hx), (pos[:, 2] + hz) / (2 * hz)], axis=1).astype(np.float32)
    return Mesh(pos, nrm, uv, np.array(idx, np.uint32))


def _fence_mesh(triangles: int, ratio: float):
    """`triangles` upright triangles side by side along x in [-1.1, 1.1] on the floor, each `ratio` times as wide as
    the one before: binned SAH peels a few off the wide end per split, so the BLAS is deep for its size."""
    from hikari_amd import Mesh
    edges = np.cumsum([0.0] + [ratio ** i for i in range(triangles)])
    edges = -1.1 + 2.2 * edges / edges[-1]
    pos, idx = [], []
    for i in range(triangles):
        k = len(pos)
        pos += [[edges[i], 0.0, 0.6], [edges[i + 1], 0.0, 0.6], [0.5 * (edges[i] + edges[i + 1]), 0.45, 0.6]]
        idx += [k, k + 1, k + 2]
    n = len(pos)
    return Mesh(np.array(pos, np.float32), np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n, 1)),
                np.tile(np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]], np.float32), (triangles, 1)),
                np.array(idx, np.uint32))


BOX_SLOTS = [(-0.55, -0.30, 0.28, 0.9), (0.50, -0.45, 0.25, 1.1), (-0.10, 0.35, 0.22, 0.5), (0.70, 0.40, 0.2, 0.6)]
EMITTER_SLOTS = [(-0.60, 1.75, -0.20), (0.05, 1.95, 0.10), (0.62, 1.70, -0.30), (0.0, 1.45, -0.75)]
EMITTER_COLOURS = [(1.0, 0.85, 0.6, 0.3), (0.5, 0.7, 1.0, 0.35), (1.0, 0.4, 0.3, 0.4), (0.6, 1.0, 0.6, 0.3)]
EMITTER_TILT = 0.7  # radians about x: the slabs' undersides face down and towards the camera
FENCE_RATIO = 1.35


def build(name: str, emissive: bool = True):
    """(scene, camera, lights) of a rung, as examples.SCENES' functions return them.  emissive=False: the same
    geometry with the emissive materials made non-emissive (the unlit control of the emitter check)."""
    from hikari_amd import Camera, Scene, StandardMaterial, Transform, examples, make_lights, plane_mesh
    from hikari_amd.scene import quat_from_axis_angle
    spec = RUNGS[name]
    rng = np.random.default_rng(SEED + list(RUNGS).index(name))
    scene = Scene()
    camera = Camera(Transform.from_xyz(0.0, 1.0, 4.0).looking_at((0.0, 1.0, 0.0)))
    if spec.get("floor", True):
        floor = scene.add_mesh(plane_mesh(1.0))
        fm = scene.add_material(StandardMaterial(base_color=(0.7, 0.7, 0.65, 1.0), perceptual_roughness=0.9))
        scene.add_instance(floor, fm, Transform(np.zeros(3), scale=np.array([8.0, 1.0, 8.0])).matrix())
        wm = scene.add_material(StandardMaterial(base_color=(0.75, 0.6, 0.5, 1.0), perceptual_roughness=0.8))
        wall = Transform(np.array([0.0, 1.1, -1.2]), quat_from_axis_angle([1, 0, 0], 0.5 * math.pi),
                         np.array([5.0, 1.0, 2.2]))
        scene.add_instance(floor, wm, wall.matrix())
    box_mesh = []
    for k, tris in enumerate(spec["boxes"]):
        x, z, half, height = BOX_SLOTS[k]
        mesh = scene.add_mesh(examples.box_grid_mesh((-half, 0.0, -half), (half, height, half), tris, rng))
        mat = scene.add_material(StandardMaterial(base_color=(0.3 + 0.6 * rng.random(), 0.3 + 0.6 * rng.random(),
                                                              0.3 + 0.6 * rng.random(), 1.0),
                                                  perceptual_roughness=0.4 + 0.5 * rng.random(), metallic=0.1 * k))
        t = Transform(np.array([x, 0.0, z]), quat_from_axis_angle([0, 1, 0], rng.uniform(-0.5, 0.5)))
        scene.add_instance(mesh, mat, t.matrix())
        box_mesh.append((mesh, mat))
    if spec.get("strip"):
        mesh = scene.add_mesh(_fence_mesh(spec["strip"], FENCE_RATIO))
        mat = scene.add_material(StandardMaterial(base_color=(0.8, 0.5, 0.2, 1.0), perceptual_roughness=0.7))
        scene.add_instance(mesh, mat, np.eye(4))
    for k, tris in enumerate(spec["emitters"]):
        e = EMITTER_COLOURS[k] if emissive else (0.0, 0.0, 0.0, 1.0)
        mat = scene.add_material(StandardMaterial(base_color=(1.0, 1.0, 1.0, 1.0), emissive=e))
        if not spec.get("floor", True):  # one_triangle: the emissive triangle alone, facing the camera
            mesh = scene.add_mesh(_slab_mesh(tris, 0.5, 0.4))
            t = Transform(np.array([0.1, 1.1, 0.0]), quat_from_axis_angle([1, 0, 0], 0.5 * math.pi))
        else:
            mesh = scene.add_mesh(_slab_mesh(tris, 0.22 + 0.04 * k, 0.16))
            t = Transform(np.array(EMITTER_SLOTS[k]), quat_from_axis_angle([1, 0, 0], EMITTER_TILT))
        scene.add_instance(mesh, mat, t.matrix())
    for _ in range(spec["chips"]):
        mesh, mat = box_mesh[0]
        t = Transform(np.array([rng.uniform(-1.0, 1.0), 0.0, rng.uniform(0.6, 1.1)]),
                      quat_from_axis_angle([0, 1, 0], rng.uniform(-1.0, 1.0)), np.full(3, rng.uniform(0.1, 0.2)))
        scene.add_instance(mesh, mat, t.matrix())
    for _ in range(spec["materials"]):
        scene.add_material(StandardMaterial(base_color=(rng.random(), rng.random(), rng.random(), 1.0)))
    return scene, camera, make_lights(None)


def emitter_instances(scene) -> list:
    """Instance indices (upload order) whose material is emissive, as the builder decides it (instance.rs:377-386)."""
    out = []
    for k, (_, mat, _) in enumerate(scene.instances):
        e = scene.materials[mat].emissive
        if 255.0 * e[3] * math.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2) > 0.0:
            out.append(k)
    return out


# ------------------------------------------------------------------ shared by the tests
SIZE = (64, 48)
FRAMES = 6  # frame numbers 0, 3 and 5: both validation intervals
LIT_RUNGS = [n for n, spec in RUNGS.items() if spec["emitters"]]
MULTI_EMITTER_RUNGS = [n for n, spec in RUNGS.items() if len(spec["emitters"]) > 1]
GBUFFER_RUNGS = ["gbuffer_at_limit", "gbuffer_over_limit", "gbuffer_no_stack_room"]
VARIANT_RUNGS = ["emitters_3", "two_rounds", "light_at_limit", "light_over_limit"]
# launch variants (hk_set_option) of the light passes over lds_scene = 2; "wavefront": hk_set_wavefront;
# "bounces_2": HikariSettings.indirect_bounces
LAUNCH_VARIANTS = {
    "merge=1": dict(merge=1),
    "merge=0": dict(merge=0),
    "fused": dict(fuse_min_px=0),
    "fused_w4": dict(fuse_min_px=0, direct_w4_min_px=0),
    "separate_w4": dict(fuse=0, direct_w4_min_px=0),
    "persistent": dict(persistent_indirect=1),
    "compact": dict(compact_emitter=1, compact_shadow=1),
    "no_view_planes": dict(spatial_view_planes=0),
    "bounces_2": dict(),
    "wavefront": dict(),
    # two launches the staging setting 2 keeps away from a staged rung, under the setting that reaches them: the
    # merged launch needs an unstaged direct role (lds_scene 1: only its indirect role stages, the IndStash behind the
    # scene), and the compacted fused kernels are the unstaged family (long and short emitter walks: the 7-triangle
    # slab's BLAS has 19 nodes, above CW_LONG_NODES)
    "merged_staged_indirect": dict(merge=1, lds_scene=1),
    "compact_fused_unstaged": dict(compact_emitter=1, compact_shadow=1, fuse_min_px=0, merge=0, lds_scene=0),
}

_built = {}
_reference = {}


def built(name: str, emissive: bool = True):
    """(scene, camera, lights) of a rung with scene.desc built, once per process."""
    key = (name, emissive)
    if key not in _built:
        scene, camera, lights = build(name, emissive)
        scene.build()
        _built[key] = (scene, camera, lights)
    return _built[key]


def ladder_settings(bounces: int = 1):
    from hikari_amd import HikariSettings, Upscale
    return HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=True, emissive_spatial_reuse=True,
                          denoise=True, indirect_bounces=bounces)


def reference(name: str, bounces: int = 1, emissive: bool = True, frames: int = FRAMES):
    """The oracle's frames of a rung at SIZE under ladder_settings, computed once per process and shared by every
    test that compares against them: per frame the canonical words of planes 0..16 and of the ten reservoir buffers,
    and after the last frame the ray counters."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    key = (name, bounces, emissive, frames)
    if key not in _reference:
        scene, cam, lights = built(name, emissive)
        w, h = SIZE
        o = Oracle(scene.desc, load_noise(), w, h, 1.0)
        s = ladder_settings(bounces).to_c()
        out = []
        for f in range(frames):
            passes(o, s, frame_inputs(f, cam, lights, w, h))
            out.append(canon_frame(o))
        _reference[key] = (out, o.counters())
        o.close()
    return _reference[key]


def example_or_rung(name: str):
    """(scene, camera, lights) of an examples.SCENES entry or of a ladder rung (the independent restatements run both)."""
    from hikari_amd import examples
    return examples.SCENES[name]() if name in examples.SCENES else build(name)
