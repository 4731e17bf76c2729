"""Cases for a new mesh asset list on the GPU (hk_set_meshes, csrc/hk_dynamic.hip k_move_mesh_slices), shared by
tests/test_mesh_set_cases.py (CPU: the host builder alone proves that every case sits on the edge its name says, and
hk_set_meshes_counts gives the host build's slices and counts) and tests/test_gpu_mesh_set.py (GPU: all nine arrays byte
for byte against the host builder's, frames against the oracle).

A case is a base scene (step 0: what is uploaded) and steps.  Step k is one hk_set_meshes call: a new mesh list and a
new entity list; scenes[k] is the host builder's scene for them, the ground truth.  A mesh of step k's list that is (the
same object) in step k - 1's list is a kept entry, its slice that of step k - 1; any other is a new mesh.  An entity that
is in two consecutive steps keeps its key, as in tests/instance_set_cases.py, whose pool materials the cases use.

The room is tests/mesh_add_cases.py's: a grey wall behind the plane z = 0 the meshes lie in, one emissive quad, its
camera and FRAME_SIZE.  Everything is seeded.

  drop_first / _middle / _last   pools of four meshes of different sizes, one dropped and un-instanced in the same step
  drop_all_but_one               everything but the quad goes
  swap_two                       two kept meshes of different sizes exchange places: the source and destination ranges
                                 overlap, which is what makes an in-place move wrong
  identity                       the same list and set
  insert_front / insert_middle   a new mesh ahead of kept ones (the BTreeMap's order)
  replace_more / replace_fewer   an instanced mesh replaced at its position by one of another triangle count, its
                                 instance keeping its key (`previous`) and moving in the same step
  replace_across_lds             1280 -> 1281 triangles and 1281 -> 1280 in one call: both build variants
  one_triangle_kept              a mesh of one node between larger ones
  chunk_edges                    kept slices that begin at a lane other than 0 inside a wave and exactly on a workgroup
                                 boundary of k_move_mesh_slices
  trailing_vertices              a kept mesh with vertices no primitive references: vertex_count > vertex_need
  pooled_kept / pooled_dropped   a base pool with meshes no instance ever used: one kept (and so registered by the
                                 call), one dropped as a gap nobody registered
  many_meshes                    40 meshes, every second one dropped, five new ones interleaved
  emissive_moved                 an emitter's mesh moves to another offset
  deep_dropped                   dropping the mesh that holds the G-buffer stack bound at 17 brings it to <= 16
  stage_edge_drop                the ladder's rung one triangle past the LDS staging limit; the drop puts it within
  shrink_then_grow               a drop, then a larger list that fits the old capacity
  then_add / then_update / then_set_instances   hk_add_meshes, hk_update_meshes on a moved mesh, hk_set_instances after
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import instance_set_cases as ic
import mesh_add_cases as ac
import mesh_cases as mc
from dynamic_cases import BVH_LDS_SHAPES, FRAME_SIZE, GB_STACK_LDS, _trs  # noqa: F401
from instance_set_cases import GREY, LIT, Entity

SEED = 0x4D534554  # "MSET"

# scenes[k], previous[k]: as above; after: None, or what follows the last step: ("add", new meshes, scene),
# ("update", scene, mesh ids) or ("set", scene, previous)
Case = namedtuple("Case", "scenes previous after")

Item = namedtuple("Item", "key mesh")        # a mesh of a pool
Inst = namedtuple("Inst", "key mesh material slot")  # an entity: its mesh by key, its place in the room by slot


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


def _slot_model(slot: int, scale: float = 0.3):
    """Place `slot` of a 5-wide rack in the plane z = 0 in front of the camera."""
    return _trs((-1.2 + 0.6 * (slot % 5), 0.4 + 0.6 * (slot // 5), 0.0), mc.FACE, np.full(3, scale))


def _quad():
    from hikari_amd import plane_mesh
    return Item("quad", plane_mesh(0.6))


def _entities(pool, insts):
    at = {item.key: k for k, item in enumerate(pool)}
    room = [Entity("light", at["quad"], LIT[0], ac.LIGHT_MODEL), Entity("wall", at["quad"], GREY, ac.WALL_MODEL)]
    return room + [Entity(i.key, at[i.mesh], i.material, _slot_model(i.slot)) for i in insts]


def _previous(scenes):
    previous = [None]
    for a, b in zip(scenes, scenes[1:]):
        where = {key: i for i, key in enumerate(a.keys)}
        previous.append([where.get(key) for key in b.keys])
    return previous


def _case(steps, after=None):
    """The Case of [(pool, insts)]: pool a list of Item (one keyed "quad"), insts a list of Inst."""
    mats = ic._materials()
    scenes = []
    for pool, insts in steps:
        ents = _entities(pool, insts)
        s = ic._scene([item.mesh for item in pool], mats, ents)
        s.entities = ents
        scenes.append(s)
    return Case(tuple(scenes), _previous(scenes), after)


def _all(pool, material=GREY, skip=()):
    """One grey instance of every mesh of the pool but the quad and `skip`, its slot fixed by its key."""
    return [Inst("e_" + item.key, item.key, material, int(item.key[1:]) if item.key[1:].isdigit() else 0)
            for item in pool if item.key != "quad" and item.key not in skip]


def _grid(tris: int, rng):
    return ac._grid(tris, rng, width=1.6, height=1.4)


def _pool(sizes, rng, first: int = 0):
    return [Item(f"m{first + k}", _grid(n, rng)) for k, n in enumerate(sizes)]


# ------------------------------------------------------------------ the cases
DROP_SIZES = (7, 20, 33)


def _drop(which):
    def make(name):
        rng = _rng(name)
        a, b, c = _pool(DROP_SIZES, rng)
        q = _quad()
        base = [a, q, b, c] if which == "first" else [q, a, b, c]
        gone = {"first": ("m0",), "middle": ("m1",), "last": ("m2",), "all": ("m0", "m1", "m2")}[which]
        kept = [item for item in base if item.key not in gone]
        return _case([(base, _all(base)), (kept, _all(kept))])
    return make


SWAP_SIZES = (10, 50)


def _swap_two(name):
    rng = _rng(name)
    a, b = _pool(SWAP_SIZES, rng)
    q = _quad()
    return _case([([q, a, b], _all([a, b])), ([q, b, a], _all([a, b]))])


def _identity(name):
    rng = _rng(name)
    pool = [_quad()] + _pool((9, 26), rng)
    return _case([(pool, _all(pool)), (pool, _all(pool))])


INSERT_TRIS = 15


def _insert(front: bool):
    def make(name):
        rng = _rng(name)
        a, b = _pool((12, 21), rng)
        q = _quad()
        n = Item("m2", _grid(INSERT_TRIS, rng))
        pool = [n, q, a, b] if front else [q, a, n, b]
        return _case([([q, a, b], _all([a, b])), (pool, _all(pool))])
    return make


REPLACE = {"replace_more": (20, 35), "replace_fewer": (35, 12)}


def _replace(name):
    """The instance of the replaced mesh keeps its key, so it carries `previous`, and moves to another slot in the same
    step: its motion vectors span the replacement."""
    rng = _rng(name)
    n0, n1 = REPLACE[name]
    q = _quad()
    old, new, b = Item("m0", _grid(n0, rng)), Item("m0", _grid(n1, rng)), Item("m1", _grid(18, rng))
    before = [Inst("e_m0", "m0", GREY, 0), Inst("e_m1", "m1", GREY, 1)]
    moved = [Inst("e_m0", "m0", GREY, 5), Inst("e_m1", "m1", GREY, 1)]
    return _case([([q, old, b], before), ([q, new, b], moved)])


def _replace_across_lds(name):
    rng = _rng(name)
    q = _quad()
    a0, b0 = Item("m0", _grid(BVH_LDS_SHAPES, rng)), Item("m1", _grid(BVH_LDS_SHAPES + 1, rng))
    a1, b1 = Item("m0", _grid(BVH_LDS_SHAPES + 1, rng)), Item("m1", _grid(BVH_LDS_SHAPES, rng))
    insts = [Inst("e_m0", "m0", GREY, 0), Inst("e_m1", "m1", GREY, 2)]
    return _case([([q, a0, b0], insts), ([q, a1, b1], insts)])


def _one_triangle_kept(name):
    rng = _rng(name)
    q = _quad()
    x, a, b = _pool((5, 40, 30), rng)
    t = Item("m3", mc._soup([[[-0.4, -0.3, 0.0], [0.4, -0.3, 0.0], [0.0, 0.4, 0.0]]]))
    base = [q, x, a, t, b]
    kept = [q, a, t, b]
    return _case([(base, _all(base)), (kept, _all(kept))])


def _padded(mesh, extra: int):
    """The mesh with `extra` vertices appended that no primitive references."""
    from hikari_amd import Mesh
    pad = np.zeros((extra, 3), np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (extra, 1))
    return Mesh(np.concatenate([mesh.positions, pad + 0.25]), np.concatenate([mesh.normals, nrm]),
                np.concatenate([mesh.uvs, np.zeros((extra, 2), np.float32)]), mesh.indices, mesh.topology)


# chunk_edges' new list: the quad (4 vertices), 40 soup triangles and 4 loose vertices (124), 10 soup triangles (30), 6
CHUNK_SOUPS = ((40, 4), (10, 0), (6, 0))


def _chunk_edges(name):
    """After the drop the kept meshes begin at vertices 0, 4, 128, 158: threads 0, 8 (a lane inside the first wave), 256
    (the first lane of the second workgroup) and 316 (lane 60 of a wave) of the vertices' chunks."""
    q = _quad()
    soups = [Item(f"m{k}", _padded(mc._row_soup(n, 1.6, 0.4), extra) if extra else mc._row_soup(n, 1.6, 0.4))
             for k, (n, extra) in enumerate(CHUNK_SOUPS)]
    d = Item("m3", mc._row_soup(3, 1.0, 0.3))
    base = [d, q] + soups
    kept = [q] + soups
    return _case([(base, _all(base)), (kept, _all(kept))])


TRAILING = 5


def _trailing_vertices(name):
    rng = _rng(name)
    q = _quad()
    x, b = _pool((6, 14), rng)
    t = Item("m2", _padded(_grid(22, rng), TRAILING))
    base = [q, x, t, b]
    kept = [q, t, b]
    return _case([(base, _all(base)), (kept, _all(kept))])


def _pooled_kept(name):
    """m1 and m2 are in the base arrays and nobody carries them; the step keeps m1 ahead of m0, and instances it, and
    drops m2."""
    rng = _rng(name)
    q = _quad()
    a, u1, u2 = _pool((16, 11, 23), rng)
    return _case([([q, a, u1, u2], _all([a])), ([q, u1, a], _all([u1, a]))])


def _pooled_dropped(name):
    rng = _rng(name)
    q = _quad()
    u1, a = _pool((11, 16), rng)
    return _case([([q, u1, a], _all([a])), ([q, a], _all([a]))])


MANY_NEW = (4, 1290, 31, 2, 140)  # triangles of the five new meshes


def _many_meshes(name):
    rng = _rng(name)
    q = _quad()
    base = [q] + [Item(f"m{k}", ac._grid(n, rng, width=1.0, height=1.0)) for k, n in enumerate(mc.MANY_SIZES)]
    kept = [q] + [item for item in base[1:] if int(item.key[1:]) % 2 == 0]
    for j, n in enumerate(MANY_NEW):
        kept.insert(1 + 4 * j, Item(f"m{41 + 2 * j}", ac._grid(n, rng, width=1.0, height=1.0)))

    def insts(pool):
        return [Inst("e_" + i.key, i.key, GREY, int(i.key[1:]) % 25) for i in pool if i.key != "quad"]
    return _case([(base, insts(base)), (kept, insts(kept))])


EMISSIVE_TRIS = 65


def _emissive_moved(name):
    rng = _rng(name)
    q = _quad()
    x, e = _pool((9, EMISSIVE_TRIS), rng)
    glow = [Inst("e_m1", "m1", LIT[1], 1)]
    return _case([([q, x, e], _all([x]) + glow), ([q, e], glow)])


DEEP_TRIS = 15  # mesh_cases._deep_soup(15): 14 inner levels; the TLAS over the four instances adds 3


def _deep_dropped(name):
    rng = _rng(name)
    q = _quad()
    deep, a = Item("m0", mc._deep_soup(DEEP_TRIS)), Item("m1", _grid(10, rng))
    spot = [Entity("e_m0", 1, GREY, mc._centred())]

    def scene(pool, extra):
        ents = _entities(pool, _all([a])) + extra
        s = ic._scene([item.mesh for item in pool], ic._materials(), ents)
        s.entities = ents
        return s
    scenes = (scene([q, deep, a], spot), scene([q, a], []))
    return Case(scenes, _previous(scenes), None)


def _stage_edge_drop(name):
    """mesh_add_cases' stage_edge_add backwards: the ladder's light_at_limit rung with a one-triangle mesh nobody
    carries (its three vertices, primitive and node put the light plan past the limit), then without it."""
    import scene_ladder as sl
    rung, _, _ = sl.build("light_at_limit")
    e = [Entity(k, mesh, mat, m) for k, (mesh, mat, m) in enumerate(rung.instances)]
    tri = mc._soup([[[-0.2, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.35, 0.0]]])
    scenes = []
    for pool in (list(rung.meshes) + [tri], list(rung.meshes)):
        s = ic._scene(pool, rung.materials, e, rung.textures)
        s.entities = e
        scenes.append(s)
    return Case(tuple(scenes), _previous(scenes), None)


SHRINK_GROW = (100, 60, 50)


def _shrink_then_grow(name):
    rng = _rng(name)
    q = _quad()
    a, b = _pool(SHRINK_GROW[:2], rng)
    n = Item("m2", _grid(SHRINK_GROW[2], rng))
    return _case([([q, a, b], _all([a, b])), ([q, a], _all([a])), ([q, a, n], _all([a, n]))])


def _moved_pair(name):
    """[quad, m0, m1, m2] -> [quad, m2, m1]: m0 dropped, m1 and m2 moved."""
    rng = _rng(name)
    q = _quad()
    a, b, c = _pool((8, 150, 27), rng)
    return rng, q, a, b, c, _case([([q, a, b, c], _all([a, b, c])), ([q, c, b], _all([c, b]))])


def _then_add(name):
    rng, q, a, b, c, case = _moved_pair(name)
    n = Item("m3", _grid(19, rng))
    pool = [q, c, b, n]
    ents = _entities(pool, _all([c, b, n]))
    s = ic._scene([i.mesh for i in pool], ic._materials(), ents)
    s.entities = ents
    return case._replace(after=("add", [n.mesh], s))


def _then_update(name):
    rng = _rng(name)
    q = _quad()
    a, c = Item("m0", _grid(8, rng)), Item("m2", _grid(27, rng))
    m0, m1 = mc._grid_pair(150, rng, width=1.6, height=1.4)
    b = Item("m1", m0)
    case = _case([([q, a, b, c], _all([a, b, c])), ([q, c, b], _all([c, b]))])
    ents = case.scenes[1].entities
    s = ic._scene([q.mesh, c.mesh, m1], ic._materials(), ents)
    s.entities = ents
    return case._replace(after=("update", s, [2]))


def _then_set_instances(name):
    rng, q, a, b, c, case = _moved_pair(name)
    pool = [q, c, b]
    ents = _entities(pool, _all([b]) + [Inst("e_twin", "m2", LIT[2], 7), Inst("e_m2", "m2", GREY, 3)])
    s = ic._scene([i.mesh for i in pool], ic._materials(), ents)
    s.entities, s.keys = ents, [e.key for e in ents]
    where = {key: i for i, key in enumerate(case.scenes[1].keys)}
    return case._replace(after=("set", s, [where.get(k) for k in s.keys]))


CASES = {
    "drop_first": _drop("first"), "drop_middle": _drop("middle"), "drop_last": _drop("last"),
    "drop_all_but_one": _drop("all"), "swap_two": _swap_two, "identity": _identity,
    "insert_front": _insert(True), "insert_middle": _insert(False),
    "replace_more": _replace, "replace_fewer": _replace, "replace_across_lds": _replace_across_lds,
    "one_triangle_kept": _one_triangle_kept, "chunk_edges": _chunk_edges, "trailing_vertices": _trailing_vertices,
    "pooled_kept": _pooled_kept, "pooled_dropped": _pooled_dropped, "many_meshes": _many_meshes,
    "emissive_moved": _emissive_moved, "deep_dropped": _deep_dropped, "stage_edge_drop": _stage_edge_drop,
    "shrink_then_grow": _shrink_then_grow, "then_add": _then_add, "then_update": _then_update,
    "then_set_instances": _then_set_instances,
}
FRAME_CASES = ["swap_two", "replace_more", "replace_fewer", "many_meshes", "emissive_moved", "insert_front"]
NO_COLLAPSE_CASES = ["replace_across_lds"]  # also under leaf_collapse 0
WAVEFRONT_CASE = "emissive_moved"
STAGE_OPTIONS = ic.STAGE_OPTIONS
STACK_OPTIONS = ic.STACK_OPTIONS


def camera_for(name: str):
    if name == "stage_edge_drop":
        return ac.camera_for("stage_edge_add")
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


_after = {}


def built_after(name: str):
    """The host-built desc of the scene that a case's `after` call leaves."""
    if name not in _after:
        c = case(name)
        scene = c.after[2] if c.after[0] == "add" else c.after[1]
        _after[name] = scene.build()
    return _after[name]


def kept_in(name: str, k: int) -> list:
    """Per mesh of step k's list: its index in step k - 1's list (the same object), or None for a new mesh."""
    c = case(name)
    before = c.scenes[k - 1].meshes
    return [next((j for j, o in enumerate(before) if o is m), None) for m in c.scenes[k].meshes]


def entries(name: str, k: int) -> list:
    """Step k's list as HikariRenderer.set_meshes takes it: a Mesh for a new mesh, (slice in step k - 1's layout, vertex
    count) for a kept one."""
    c = case(name)
    before = c.scenes[k - 1]
    return [m if j is None else (before.mesh_index(j), len(m.positions))
            for m, j in zip(c.scenes[k].meshes, kept_in(name, k))]


def slices(name: str, k: int) -> list:
    """The host builder's (vertex, primitive, node0, node_count) of every mesh of step k."""
    s = case(name).scenes[k]
    return [s.mesh_index(i) for i in range(len(s.meshes))]


def local_aabbs(scene) -> np.ndarray:
    return mc.local_aabbs(scene)


# ------------------------------------------------------------------ applying a step to a HikariRenderer
def step(r, name: str, k: int, stream=None) -> list:
    """Step k's hk_set_meshes on `r`: the slices it returns."""
    c = case(name)
    scene = c.scenes[k]
    return r.set_meshes(scene, entries(name, k), previous=c.previous[k], local_aabbs=local_aabbs(scene), stream=stream)


def host_slices(name: str, k: int) -> list:
    """slices(name, k) as tuples of Python ints, as HikariRenderer.set_meshes returns them."""
    return [tuple(int(x) for x in s) for s in slices(name, k)]
