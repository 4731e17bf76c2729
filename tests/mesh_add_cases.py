"""Cases for the GPU mesh append (hk_add_meshes, csrc/hk_dynamic.hip k_assemble_meshes), shared by
tests/test_mesh_add_cases.py (CPU: the host builder alone proves that every case sits on the edge its name says, and
hk_add_meshes_counts gives the host build's slices and counts) and tests/test_gpu_mesh_add.py (GPU: the appended
vertices, primitives and BLAS byte for byte against the host builder's, frames against the oracle).

A case is a base scene (step 0: what is uploaded) and one or more steps.  Step k adds the meshes new[k] in one
hk_add_meshes call and then sets the instance list of scenes[k], the host builder's scene for that step: the pool so
far with the new meshes added last, and the step's entities.  add_only(name, k) is the host's scene between the two
calls: step k's pool under step k - 1's entities.  An entity that is in two consecutive steps keeps its key, as in
tests/instance_set_cases.py, whose pool materials (grey, four emitter colours, a dark one) the cases use.

The new meshes are those of tests/mesh_cases.py: seeded grids in the plane z = 0 in front of its camera, their vertices
moved far enough that the BLAS is no regular tree.  Every base scene has a grey wall behind that plane and one emissive
quad, so the frames are lit.  Everything is seeded.

  tris_1, tris_2            a lone leaf, and one split
  tris_128 / tris_129       the per-thread split alone, and coop_split entered at the root (COOP_MIN)
  tris_256 / tris_257       one and two 256-chunks of the ballot ranking
  tris_1280 / tris_1281     the LDS-staged and the global build (BVH_LDS_SHAPES)
  tris_2600                 the global build with several levels of big segments
  strip_even / strip_odd    strips of 6 and 7 indices, second in their call behind a mesh of an odd triangle count: both
                            windings, a mesh-local odd last triangle, and a global triangle id of the other parity
  non_indexed               indices == NULL
  shared_vertices           an indexed grid
  degenerate, neg_zero      as in mesh_cases
  many_meshes               40 meshes in one call, lists, strips and non-indexed in turn, sizes on both sides of 1280
  three_calls               small, then large enough to reallocate all three arrays, then small into spare capacity
  emissive_new              a new mesh spawned with an emissive material
  deep_new                  a new mesh whose instancing takes the stack bound from <= 16 to 17
  stage_edge_add            the ladder's light_at_limit rung plus a one-triangle mesh: past the limit by the add alone
  then_update               hk_update_meshes on an added mesh
  pool_tail                 a base scene whose last meshes no instance uses
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import instance_set_cases as ic
import mesh_cases as mc
from dynamic_cases import BVH_LDS_SHAPES, COOP_MIN, FRAME_SIZE, GB_STACK_LDS, _rot, _trs  # noqa: F401
from instance_set_cases import GREY, LIT, Entity

SEED = 0x4D414444  # "MADD"

# scenes[k], new[k]: see above (new[0] is empty); previous[k]: step k's map into step k - 1; update: None, or
# (scene, mesh ids) for an hk_update_meshes call after the last step
Case = namedtuple("Case", "scenes new previous update")

LIGHT_MODEL = _trs((1.7, 2.3, 2.0), _rot([1, 0, 0], -0.75 * math.pi), np.ones(3))
WALL_MODEL = _trs((0.0, 1.0, -0.6), _rot([1, 0, 0], 0.5 * math.pi), np.full(3, 6.0))
QUAD = 0  # mesh 0 of every pool but the ladder's


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


def _base_entities():
    """The emissive quad of mesh_cases' scenes and a grey wall behind the plane the new meshes lie in."""
    return [Entity("light", QUAD, LIT[0], LIGHT_MODEL), Entity("wall", QUAD, GREY, WALL_MODEL)]


def _case(pool0, steps, entities0=None, materials=None, textures=(), update=None):
    """The Case of a base pool and steps [(new meshes, entities after)]."""
    from hikari_amd import plane_mesh
    mats = materials if materials is not None else ic._materials()
    pool = list(pool0) if pool0 is not None else [plane_mesh(0.6)]
    ents = entities0 if entities0 is not None else _base_entities()
    scenes, new = [], [[]]
    lists = [ents] + [e for _, e in steps]
    for k, e in enumerate(lists):
        if k:
            new.append(list(steps[k - 1][0]))
            pool = pool + new[k]
        s = ic._scene(pool, mats, e, textures)
        s.entities = list(e)
        scenes.append(s)
    previous = [None]
    for a, b in zip(scenes, scenes[1:]):
        where = {key: i for i, key in enumerate(a.keys)}
        previous.append([where.get(key) for key in b.keys])
    return Case(tuple(scenes), new, previous, update)


def _spawned(entities, first_mesh, count, material=GREY, model=None, key="new"):
    """`entities` and one instance of each of the `count` meshes from pool index `first_mesh` on."""
    return list(entities) + [Entity(f"{key}{k}", first_mesh + k, material, mc._centred() if model is None else model)
                             for k in range(count)]


# ------------------------------------------------------------------ meshes
def _grid(tris: int, rng, **kw):
    return mc._grid_mesh(tris, rng, 2.5, True, **kw)


def _unindexed(mesh):
    """The triangle list with its own three vertices per triangle and no index buffer."""
    from hikari_amd import Mesh
    ix = np.asarray(mesh.indices)
    return Mesh(mesh.positions[ix].copy(), mesh.normals[ix].copy(), mesh.uvs[ix].copy(), None)


def _strip(tris: int, rng, width: float = mc.WIDTH, height: float = 1.2, indexed: bool = True):
    """A TriangleStrip of tris + 2 vertices zig-zagging along x, seeded; indexed: the vertices stored in a seeded
    order and the index buffer naming them in strip order (the indices are read, not assumed to be 0 .. n - 1)."""
    from hikari_amd import Mesh
    n = tris + 2
    x = (np.arange(n) // 2) / max(1, (n + 1) // 2 - 1) - 0.5
    pos = np.stack([x * width, (np.arange(n) % 2 - 0.5) * height, np.zeros(n)], axis=1)
    pos += rng.normal(size=pos.shape) * np.array([width / n, 0.1 * height, 0.02])[None, :]
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    uv = np.stack([x + 0.5, np.arange(n) % 2], axis=1)
    if not indexed:
        return Mesh(pos.astype(np.float32), nrm.astype(np.float32), uv.astype(np.float32), None, 1)
    perm = rng.permutation(n)  # vertex storage order shuffled: index i names vertex perm[i]
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return Mesh(pos[inv].astype(np.float32), nrm[inv].astype(np.float32), uv[inv].astype(np.float32),
                perm.astype(np.uint32), 1)


# ------------------------------------------------------------------ the cases
def _one(mesh_of, material=GREY):
    def make(name):
        rng = _rng(name)
        base = _base_entities()
        return _case(None, [([mesh_of(rng)], _spawned(base, 1, 1, material))])
    return make


def _tris(n: int):
    return _one(lambda rng: _grid(n, rng))


STRIP_FIRST_TRIS = 5  # the mesh in front of the strip in its call: an odd count, so the strip's first global id is odd


def _strip_case(indices: int):
    def make(name):
        rng = _rng(name)
        base = _base_entities()
        first = _grid(STRIP_FIRST_TRIS, rng, width=0.8, height=0.6)
        ents = base + [Entity("new0", 1, GREY, _trs((-0.9, 1.0, 0.0), mc.FACE, np.ones(3))),
                       Entity("new1", 2, GREY, _trs((0.4, 1.0, 0.0), mc.FACE, np.ones(3)))]
        return _case(None, [([first, _strip(indices - 2, rng, width=1.6)], ents)])
    return make


def _from_mesh_cases(which: str):
    def make(name):
        return _case(None, [([mc.case(which)[1].meshes[0]], _spawned(_base_entities(), 1, 1))])
    return make


MANY_KINDS = ("list", "strip", "non_indexed")


def _many_meshes(name):
    rng = _rng(name)
    meshes, ents = [], _base_entities()
    for k, n in enumerate(mc.MANY_SIZES):
        kind = MANY_KINDS[k % 3]
        if kind == "strip":
            m = _strip(n, rng, width=1.0, height=1.0, indexed=k % 2 == 0)
        else:
            m = _grid(n, rng, width=1.0, height=1.0)
            m = _unindexed(m) if kind == "non_indexed" else m
        meshes.append(m)
        at = (-1.4 + 0.4 * (k % mc.MANY_COLS), 0.2 + 0.4 * (k // mc.MANY_COLS), 0.0)
        ents.append(Entity(f"new{k}", 1 + k, GREY, _trs(at, mc.FACE, np.full(3, 0.36))))
    return _case(None, [(meshes, ents)])


THREE_CALLS = (1000, 10, 600, 3)  # triangles: the base scene's grid, then the three calls' meshes


def _three_calls(name):
    """The base holds a grid of 1000 triangles, so its capacities are about 1000: the first call (10 triangles) grows
    each array to 1.5 times that, the second (600) passes it and grows again to 1.5 times, the third (3) fits."""
    from hikari_amd import plane_mesh
    rng = _rng(name)
    base = _base_entities() + [Entity("grid", 1, GREY, _trs((0.0, 1.0, -0.3), mc.FACE, np.ones(3)))]
    pool0 = [plane_mesh(0.6), _grid(THREE_CALLS[0], rng)]
    steps, ents = [], base
    for k, n in enumerate(THREE_CALLS[1:]):
        ents = ents + [Entity(f"new{k}", 2 + k, GREY, _trs((-0.8 + 0.8 * k, 1.0, 0.0), mc.FACE, np.full(3, 0.3)))]
        steps.append(([_grid(n, rng)], ents))
    return _case(pool0, steps, entities0=base)


DEEP_NEW_TRIS = 16  # mesh_cases._deep_soup(16): 15 inner levels; the TLAS over the three instances adds 2


def _deep_new(name):
    return _case(None, [([mc._deep_soup(DEEP_NEW_TRIS)], _spawned(_base_entities(), 1, 1))])


def _stage_edge_add(name):
    """The ladder's light_at_limit rung (its light plan stages exactly 32768 bytes); one more triangle's three
    vertices, primitive and node put the plan past the limit before any instance carries it."""
    import scene_ladder as sl
    rung, _, _ = sl.build("light_at_limit")
    e = [Entity(k, mesh, mat, m) for k, (mesh, mat, m) in enumerate(rung.instances)]
    _, box_mat, _ = rung.instances[2]
    tri = mc._soup([[[-0.2, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.35, 0.0]]])
    more = e + [Entity("new0", len(rung.meshes), box_mat, _trs((0.3, 0.4, 1.0), mc.FACE, np.ones(3)))]
    return _case(rung.meshes, [([tri], more)], entities0=e, materials=rung.materials, textures=rung.textures)


THEN_UPDATE_TRIS = 150


def _then_update(name):
    import copy
    rng = _rng(name)
    m0, m1 = mc._grid_pair(THEN_UPDATE_TRIS, rng)
    c = _case(None, [([m0], _spawned(_base_entities(), 1, 1))])
    last = c.scenes[-1]
    deformed = copy.copy(last)
    deformed._h, deformed.desc = None, None
    deformed.meshes = list(last.meshes)
    deformed.meshes[1] = m1
    return c._replace(update=(deformed, [1]))


def _pool_tail(name):
    from hikari_amd import plane_mesh
    rng = _rng(name)
    pool0 = [plane_mesh(0.6), ic._strip(3, rng), _grid(20, rng)]  # meshes 1 and 2: in the arrays, carried by nobody
    return _case(pool0, [([_grid(30, rng)], _spawned(_base_entities(), 3, 1))])


SIZES = {f"tris_{n}": n for n in (1, 2, 128, 129, 256, 257, 1280, 1281, 2600)}
STRIPS = {"strip_even": 6, "strip_odd": 7}  # index counts
EMISSIVE_TRIS = 65
CASES = {
    **{name: _tris(n) for name, n in SIZES.items()},
    **{name: _strip_case(n) for name, n in STRIPS.items()},
    "non_indexed": _one(lambda rng: _unindexed(_grid(45, rng))),
    "shared_vertices": _one(lambda rng: _grid(60, rng)),
    "degenerate": _from_mesh_cases("degenerate"), "neg_zero": _from_mesh_cases("neg_zero"),
    "many_meshes": _many_meshes, "three_calls": _three_calls,
    "emissive_new": _one(lambda rng: _grid(EMISSIVE_TRIS, rng, width=1.2, height=1.0), material=LIT[1]),
    "deep_new": _deep_new, "stage_edge_add": _stage_edge_add, "then_update": _then_update, "pool_tail": _pool_tail,
}
FRAME_CASES = ["emissive_new", "many_meshes", "strip_odd", "tris_1281", "stage_edge_add"]
NO_COLLAPSE_CASES = ["tris_1281", "strip_odd"]  # also under leaf_collapse 0
WAVEFRONT_CASE = "emissive_new"
STAGE_OPTIONS = ic.STAGE_OPTIONS
STACK_OPTIONS = ic.STACK_OPTIONS


def camera_for(name: str):
    if name == "stage_edge_add":
        import scene_ladder as sl
        _, cam, lights = sl.build("light_at_limit")
        return cam, lights
    return mc.camera_for(name)


_made = {}


def case(name: str) -> Case:
    """The Case of a name, made once per process; step 0 is built (scenes[0].desc)."""
    if name not in _made:
        c = CASES[name](name)
        c.scenes[0].build()
        _made[name] = c
    return _made[name]


def steps(name: str) -> range:
    return range(len(case(name).scenes))


def built(name: str, k: int):
    """Step k's host-built desc, once per process."""
    s = case(name).scenes[k]
    return s.desc if s.desc is not None else s.build()


_add_only = {}


def add_only(name: str, k: int):
    """The host's scene after step k's hk_add_meshes and before its hk_set_instances, built once per process: step k's
    pool, step k - 1's entities."""
    if (name, k) not in _add_only:
        c = case(name)
        now, before = c.scenes[k], c.scenes[k - 1]
        s = ic._scene(now.meshes, now.materials, before.entities, now.textures)
        s.build()
        _add_only[(name, k)] = s
    return _add_only[(name, k)]


_updated = {}


def built_update(name: str):
    """The host-built desc of a case's `update` scene."""
    if name not in _updated:
        _updated[name] = case(name).update[0].build()
    return _updated[name]


def local_aabbs(scene) -> np.ndarray:
    return mc.local_aabbs(scene)


def new_slices(name: str, k: int) -> list:
    """The host builder's (vertex, primitive, node0, node_count) of the meshes step k adds."""
    c = case(name)
    first = len(c.scenes[k].meshes) - len(c.new[k])
    return [c.scenes[k].mesh_index(i) for i in range(first, len(c.scenes[k].meshes))]


# ------------------------------------------------------------------ applying a step to a HikariRenderer
def add(r, name: str, k: int, stream=None) -> list:
    """Step k's hk_add_meshes on `r`: the slices it returns."""
    return r.add_meshes(case(name).new[k], stream=stream)


def spawn(r, name: str, k: int, stream=None):
    """Step k's hk_set_instances on `r`, after its add."""
    c = case(name)
    scene = c.scenes[k]
    r.set_instances(scene, previous=c.previous[k], local_aabbs=local_aabbs(scene), stream=stream)


def added_so_far(name: str, k: int) -> list:
    """The slices of every mesh that steps 1..k added: registered on the device, instanced or not."""
    return [s for j in range(1, k + 1) for s in new_slices(name, j)]
