"""Cases for the GPU instance-set rebuild (hk_set_instances, csrc/hk_dynamic.hip), shared by
tests/test_instance_set_cases.py (CPU: the host builder alone proves that every case sits where its name says, and
hk_instance_set_counts gives the host build's counts) and tests/test_gpu_instance_set.py (GPU: the rebuilt arrays byte
for byte against the host builder's, frames against the oracle).

A case is a sequence of two or three scenes ("steps") over ONE asset pool: the same meshes and materials in the same
order, and another instance list per step.  Step 0 is what is uploaded; step k is the host builder's scene for the
k-th hk_set_instances call and the source of its instance descs, models and local AABBs.  An instance is an entity
(key, mesh, material, model): an entity that is in two consecutive steps is the same entity, with the same key, and
`previous` is derived from the keys.  The scenes are small: the shared quad of tests/dynamic_cases.py, its flat emitter
strips, the ladder's rung for stage_edge and one deep triangle soup of tests/mesh_cases.py.  Everything is seeded.

What each case exercises:
  despawn_middle        5 -> 4 instances, an emitter behind the removed one: every later index and em.instance shifts
  spawn_copies          4 -> 6: the alias table, instances, TLAS, light BVH and emissives all grow past their capacity
  spawn_pooled          the first instance of a mesh no instance used at upload: registration
  emitter_off / _on     an instance's material index swapped to / from an emissive one: 1 -> 0 and 0 -> 1 emitters
  materials_replaced    the material records replaced: emissive to 0, from 0, alpha 0, a NaN component
  emitters_3_5_7        emitters of 3, 5 and 7 triangles; the middle one removed, then one of 4 added in front
  wave_edge, chunk_edge 70 / 300 instances with emitters at 63, 64 / 255, 256: k_compact_emitters' wave and chunk carries
  to_one, from_one_129  down to a lone-leaf TLAS; 1 -> 129, where coop_split is entered at the root
  lds_build_edge        1280 -> 1281 -> 1280: k_build_bvh<true> / <false> by the new count
  stage_edge            the ladder's light_at_limit rung, one more instance (out of LDS staging), and back
  deeper_blas           the only instance of a deep mesh spawned (stack bound 17) and despawned (<= 16)
  there_and_back        A -> B -> A on grown, dirty scratch
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import dynamic_cases as dc
from dynamic_cases import BVH_LDS_SHAPES, COOP_MIN, EMITTER_COLOURS, FRAME_SIZE, GB_STACK_LDS, QUAD_HALF  # noqa: F401

SEED = 0x53455449  # "SETI"

Entity = namedtuple("Entity", "key mesh material model")
Case = namedtuple("Case", "scenes previous materials")  # previous[k]: step k's map into step k - 1 (previous[0]: None)

# the pool's materials: grey, the four emitter colours of dynamic_cases, and one whose emissive colour is black
GREY, LIT, DARK = 0, (1, 2, 3, 4), 5
QUAD = 0  # mesh 0 of every pool
BIG = dict(scale=(3.0, 5.0))  # the quads of the small cases: a few of them fill a tenth of the view


def _materials():
    from hikari_amd import StandardMaterial
    return ([StandardMaterial(base_color=(0.7, 0.65, 0.6, 1.0), perceptual_roughness=0.8)] +
            [StandardMaterial(base_color=(1.0, 1.0, 1.0, 1.0), emissive=e) for e in EMITTER_COLOURS] +
            [StandardMaterial(base_color=(0.9, 0.9, 0.9, 1.0), emissive=(0.0, 0.0, 0.0, 1.0))])


def _scene(meshes, materials, entities, textures=()):
    """A Scene over the pool's meshes and materials (the lists are shared between a case's steps) with these
    entities as its instance list."""
    from hikari_amd import Scene
    s = Scene()
    s.meshes, s.materials, s.textures = list(meshes), list(materials), list(textures)
    s.instances = [(e.mesh, e.material, np.asarray(e.model, np.float64)) for e in entities]
    s.keys = [e.key for e in entities]
    return s


def _steps(meshes, steps, materials=None, per_step_materials=None, textures=()):
    """The Case of these entity lists: one scene per list, `previous` from the keys."""
    mats = materials if materials is not None else _materials()
    scenes = tuple(_scene(meshes, per_step_materials[k] if per_step_materials else mats, ents, textures)
                   for k, ents in enumerate(steps))
    previous = [None]
    for a, b in zip(scenes, scenes[1:]):
        where = {key: i for i, key in enumerate(a.keys)}
        previous.append([where.get(key) for key in b.keys])
    return Case(scenes, previous, per_step_materials is not None)


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


def _quad_mesh():
    from hikari_amd import plane_mesh
    return plane_mesh(2.0 * QUAD_HALF)


def _quads(n: int, rng, first_key: int = 0, **kw) -> list:
    """n grey quads with seeded models (dynamic_cases._plain_models), keys first_key .."""
    return [Entity(first_key + k, QUAD, GREY, m) for k, m in enumerate(dc._plain_models(n, rng, **kw))]


def _strip(triangles: int, rng):
    return dc._strip_mesh(dc._seeded_widths(triangles, rng, 0.3))


def _without(entities, *keys):
    return [e for e in entities if e.key not in keys]


# ------------------------------------------------------------------ the cases
def _despawn_middle(name):
    rng = _rng(name)
    meshes = [_quad_mesh(), _strip(3, rng), _strip(5, rng)]
    e = _quads(5, rng, **BIG)
    e[1] = e[1]._replace(mesh=1, material=LIT[0])
    e[3] = e[3]._replace(mesh=2, material=LIT[1])
    return _steps(meshes, [e, _without(e, 2)])


def _spawn_copies(name, back=False):
    rng = _rng(name)
    meshes = [_quad_mesh(), _strip(4, rng)]
    e = _quads(6, rng, **BIG)
    e[1] = e[1]._replace(mesh=1, material=LIT[0])
    e[5] = e[5]._replace(mesh=1, material=LIT[2])  # a second instance of the strip: a copy that is an emitter too
    first = e[:4]
    return _steps(meshes, [first, e, first] if back else [first, e])


def _spawn_pooled(name):
    rng = _rng(name)
    # the pooled mesh lies between two instanced ones in the vertex, primitive and node arrays
    meshes = [_quad_mesh(), _strip(6, rng), _strip(3, rng)]
    e = _quads(5, rng, **BIG)
    e[2] = e[2]._replace(mesh=2, material=LIT[0])
    e[4] = e[4]._replace(mesh=1, material=LIT[3])
    return _steps(meshes, [e[:4], e])


def _emitter(on: bool):
    def make(name):
        rng = np.random.default_rng([SEED, 1000])  # emitter_off and emitter_on are one pair, reversed
        meshes = [_quad_mesh(), _strip(5, rng)]
        e = _quads(4, rng, **BIG)
        lit = list(e)
        lit[2] = e[2]._replace(mesh=1, material=LIT[1])
        dark = list(e)
        dark[2] = e[2]._replace(mesh=1, material=GREY)
        return _steps(meshes, [dark, lit] if on else [lit, dark])
    return make


def _materials_replaced(name):
    from hikari_amd import StandardMaterial
    rng = _rng(name)
    meshes = [_quad_mesh(), _strip(3, rng), _strip(4, rng), _strip(2, rng)]
    nan = float("nan")
    # (emissive at upload, emissive after): to 0, from 0, alpha to 0, a NaN component after, a NaN component on both
    # sides, one that stays an emitter
    emissive = [((1.0, 0.8, 0.6, 0.3), (0.0, 0.0, 0.0, 0.3)), ((0.0, 0.0, 0.0, 1.0), (0.5, 0.7, 1.0, 0.35)),
                ((1.0, 0.4, 0.3, 0.4), (1.0, 0.4, 0.3, 0.0)), ((0.6, 1.0, 0.6, 0.3), (0.6, nan, 0.6, 0.3)),
                ((nan, 0.2, 0.2, 0.3), (0.2, 0.2, 0.2, nan)), ((0.9, 0.9, 0.5, 0.3), (0.9, 0.9, 0.5, 0.3))]
    per_step = [[StandardMaterial(base_color=(0.7, 0.65, 0.6, 1.0), perceptual_roughness=0.8)] +
                [StandardMaterial(base_color=(1.0, 1.0, 1.0, 1.0), emissive=pair[k]) for pair in emissive] for k in (0, 1)]
    e = _quads(len(emissive) + 2, rng)
    for j in range(len(emissive)):
        e[1 + j] = e[1 + j]._replace(mesh=1 + j % 3, material=1 + j)
    return _steps(meshes, [e, e], per_step_materials=per_step)


EMITTERS_FRONT = 4  # triangles of the emitter added in front in the last step of emitters_3_5_7


def _emitters_3_5_7(name):
    rng = _rng(name)
    meshes = [_quad_mesh(), _strip(3, rng), _strip(5, rng), _strip(7, rng), _strip(EMITTERS_FRONT, rng)]
    e = _quads(6, rng, first_key=1, **BIG)
    for j, at in enumerate((0, 2, 4)):
        e[at] = e[at]._replace(mesh=1 + j, material=LIT[j])
    front = Entity(0, 4, LIT[3], dc._plain_models(1, rng, **BIG)[0])
    return _steps(meshes, [e, _without(e, 3), [front] + _without(e, 3)])


def _carry_edge(n: int, at: int):
    """Step 0: n + 1 instances with emitters at `at` + 1 and `at` + 2; step 1: without instance 0, so the emitters sit
    at `at` and `at` + 1 (63 | 64: the last lane of a wave and the first of the next; 255 | 256: the same across two
    chunks), and one more emitter near the end, whose rank and alias offset need both carries."""
    def make(name):
        rng = _rng(name)
        meshes = [_quad_mesh(), _strip(3, rng), _strip(5, rng), _strip(2, rng)]
        e = _quads(n + 1, rng)
        e[at + 1] = e[at + 1]._replace(mesh=1, material=LIT[0])
        e[at + 2] = e[at + 2]._replace(mesh=2, material=LIT[1])
        e[n - 1] = e[n - 1]._replace(mesh=3, material=LIT[2])
        return _steps(meshes, [e, _without(e, 0)])
    return make


def _to_one(name):
    rng = _rng(name)
    meshes = [_quad_mesh(), _strip(3, rng)]
    e = _quads(3, rng, scale=(3.0, 5.0))
    e[1] = e[1]._replace(mesh=1, material=LIT[0])
    return _steps(meshes, [e, [e[1]]])


def _from_one_129(name):
    rng = _rng(name)
    meshes = [_quad_mesh(), _strip(3, rng)]
    e = _quads(COOP_MIN + 1, rng)
    e[40] = e[40]._replace(mesh=1, material=LIT[0])
    return _steps(meshes, [[e[40]], e])


def _lds_build_edge(name):
    rng = _rng(name)
    meshes = [_quad_mesh(), _strip(2, rng)]
    e = _quads(BVH_LDS_SHAPES + 1, rng)
    e[640] = e[640]._replace(mesh=1, material=LIT[0])
    return _steps(meshes, [e[:-1], e, e[:-1]])


def _stage_edge(name):
    """The ladder's light_at_limit rung (its light plan stages exactly 32768 bytes), then with one more instance of
    its first box (an instance record of 176 bytes and three TLAS nodes of 32: 272 more bytes, past the limit), then
    the rung again."""
    import scene_ladder as sl
    from hikari_amd import Transform
    from hikari_amd.scene import quat_from_axis_angle
    rung, _, _ = sl.build("light_at_limit")
    e = [Entity(k, mesh, mat, m) for k, (mesh, mat, m) in enumerate(rung.instances)]
    box_mesh, box_mat, _ = rung.instances[2]  # (0, 1: the floor and the wall)
    chip = Transform(np.array([0.3, 0.0, 0.9]), quat_from_axis_angle([0, 1, 0], 0.4), np.full(3, 0.15)).matrix()
    more = e + [Entity(len(e), box_mesh, box_mat, chip)]
    return _steps(rung.meshes, [e, more, e], materials=rung.materials, textures=rung.textures)


DEEP_TRIS = 15  # mesh_cases._deep_soup(15): 14 inner levels; with the TLAS's 3 over these four instances the bound is 17


def _deeper_blas(name):
    import mesh_cases as mc
    rng = _rng(name)
    meshes = [_quad_mesh(), mc._deep_soup(DEEP_TRIS), _strip(3, rng)]
    e = _quads(3, rng, scale=(3.0, 5.0))
    e[1] = e[1]._replace(mesh=2, material=LIT[0])
    deep = Entity(3, 1, GREY, dc._trs(mc.CENTRE, mc.FACE, np.ones(3)))
    return _steps(meshes, [e, e + [deep], e])


CASES = {
    "despawn_middle": _despawn_middle, "spawn_copies": _spawn_copies, "spawn_pooled": _spawn_pooled,
    "emitter_off": _emitter(False), "emitter_on": _emitter(True), "materials_replaced": _materials_replaced,
    "emitters_3_5_7": _emitters_3_5_7, "wave_edge": _carry_edge(70, 63), "chunk_edge": _carry_edge(300, 255),
    "to_one": _to_one, "from_one_129": _from_one_129, "lds_build_edge": _lds_build_edge, "stage_edge": _stage_edge,
    "deeper_blas": _deeper_blas, "there_and_back": lambda name: _spawn_copies("spawn_copies", back=True),
}
CARRY = {"wave_edge": (70, 63), "chunk_edge": (300, 255)}
FRAME_CASES = ["despawn_middle", "spawn_pooled", "emitter_on", "emitters_3_5_7", "chunk_edge", "stage_edge",
               "deeper_blas"]
STACK_OPTIONS = [{}, {"gbuffer_stack_full": 1}, {"gbuffer_deep": 1}]
STAGE_OPTIONS = [{"lds_scene": 0}, {"lds_scene": 1}, {"lds_scene": 2}]


def camera_for(name: str):
    """(camera, lights) of a case's frames: the ladder's camera for its rung, else dynamic_cases' in front of the box
    the instances fill."""
    if name == "stage_edge":
        import scene_ladder as sl
        _, cam, lights = sl.build("light_at_limit")
        return cam, lights
    return dc.camera_for(name)


_made = {}


def case(name: str) -> Case:
    """The Case of a name, made once per process; step 0 is built (scenes[0].desc)."""
    if name not in _made:
        c = CASES[name](name)
        c.scenes[0].build()
        _made[name] = c
    return _made[name]


def built(name: str, k: int):
    """Step k's host-built desc, once per process."""
    s = case(name).scenes[k]
    return s.desc if s.desc is not None else s.build()


def steps(name: str) -> range:
    return range(len(case(name).scenes))


def local_aabbs(scene) -> np.ndarray:
    """(n, 6) Bevy `Aabb` of each instance's mesh as the host builder folds it (mesh_cases.local_aabbs: a zero bound
    with the sign of the last vertex that has a zero there; the pool's meshes are flat)."""
    import mesh_cases as mc
    return mc.local_aabbs(scene)


def desc_counts(desc) -> list:
    from parity import SCENE_ARRAYS
    return [getattr(desc, a).count for a in SCENE_ARRAYS]


def emissive_records(desc) -> np.ndarray:
    """(m, 16) uint32 words of a host-built scene's hk_emissive records: word 8 the instance, 10 and 11 the alias
    range."""
    from parity import host_scene_array
    return np.frombuffer(host_scene_array(desc, 8, np.dtype((np.void, 64))).tobytes(), np.uint32).reshape(-1, 16)


# ------------------------------------------------------------------ applying a step to a HikariRenderer
def apply(r, name: str, k: int, **kw):
    """Step k's hk_set_instances on `r` (kw: models, local_aabbs or stream in place of the step's own)."""
    c = case(name)
    scene = c.scenes[k]
    kw.setdefault("local_aabbs", local_aabbs(scene))
    r.set_instances(scene, previous=c.previous[k], materials=c.materials, **kw)
