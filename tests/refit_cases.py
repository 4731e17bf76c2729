"""Cases for the BLAS refit (hk_refit_meshes / hk_skin_meshes_refit, csrc/hk_dynamic.hip k_refit_small and
k_refit_large; hikari_scene.h hks_refit_nodes), shared by tests/test_refit_cases.py (CPU: every case proven to sit on the
edge its name says, the oracle on the refitted scene) and tests/test_gpu_refit.py (GPU: the arrays after a refit byte
for byte against Scene.refitted, frames against the oracle on it).

A case is a pair (scene0, scene1) as in tests/mesh_cases.py: scene0 is uploaded and gives the topology, scene1 the
vertices the refit takes.  Most pairs are mesh_cases' own, by import; the rest are made here with its builders.

The limit the sizes straddle is REFIT_SMALL in hk_dynamic.hip (restated here; tests/test_refit_cases.py reads it back
from the source): an entry node i with exit - i <= REFIT_SMALL is refit by its own thread, a larger one by a workgroup.
exit - i is 3p - 1 for a subtree of p primitives, so the spans that exist either side of the limit are 32 (p = 11) and
35 (p = 12): small_32 has no large node, small_35 has the root's two children and nothing else.

  tris_1, tris_2            no entry node; the two entry nodes of one split
  small_32, small_35        the largest range is exactly REFIT_SMALL / the next one that exists
  tris_1281, tris_2600      several large nodes on several levels
  deep_17, deep_65          chain-shaped trees of 17 and 65 inner levels: small subtrees nested inside large ones
                            (deep_17: mesh_cases._deep_soup; 65 levels at its ratio of 4 pass float32's range, so
                            deep_65 is mesh_cases._axes_soup, as its too_deep case)
  many_meshes               40 slices in one call, with and without large nodes
  one_of_three              the unlisted slices keep their bytes
  shared_mesh, emissive_mesh, strip, keep_normals, neg_zero, coincident_300    as in mesh_cases
  folded                    a grid folded over itself along x = 0: sibling boxes overlap
"""
from __future__ import annotations

import numpy as np

import mesh_cases as mc

REFIT_SMALL = 32
SEED = 0x52454654  # "REFT"
SMALL_TRIS = {"small_32": 22, "small_35": 23}  # mesh_cases._row_soup sizes whose root splits 11 + 11 / 12 + 11
DEEP = {"deep_17": ("_deep_soup", 18), "deep_65": ("_axes_soup", 131)}
FOLDED_TRIS = 600
FROM_MESH_CASES = ["tris_1", "tris_2", "tris_1281", "tris_2600", "many_meshes", "one_of_three", "shared_mesh",
                   "emissive_mesh", "strip", "keep_normals", "neg_zero", "coincident_300"]


def _rng(name: str):
    return np.random.default_rng([SEED, sorted(OWN).index(name)])


def _jitter(mesh, rng, amount: float):
    """A soup with every triangle scaled about its first corner by a seeded factor in 1 +- amount and moved by up to
    `amount` of its own size: the same topology, other boxes, the order of magnitude of every triangle kept."""
    from hikari_amd import Mesh
    p = np.asarray(mesh.positions, np.float64).reshape(-1, 3, 3)
    size = np.abs(p - p[:, :1]).max(axis=(1, 2), keepdims=True)
    q = p[:, :1] + (p - p[:, :1]) * rng.uniform(1.0 - amount, 1.0 + amount, (len(p), 1, 1))
    q = q + size * rng.uniform(-amount, amount, (len(p), 1, 3)) * np.array([1.0, 1.0, 0.0])
    return Mesh(q.reshape(-1, 3).astype(np.float32), mesh.normals, mesh.uvs, mesh.indices)


def _small(name):
    m0 = mc._row_soup(SMALL_TRIS[name])
    return mc._pair([(m0, _jitter(m0, _rng(name), 0.3))], [(0, mc._centred())])


def _deep(name):
    maker, n = DEEP[name]
    m0 = getattr(mc, maker)(n)
    return mc._pair([(m0, _jitter(m0, _rng(name), 0.2))], [(0, mc._centred())])


def _folded(name):
    """scene1: scene0's grid with x -> |x| - WIDTH / 4: the left half lies on the right one."""
    from hikari_amd import Mesh
    rng = _rng(name)
    m0 = mc._grid_mesh(FOLDED_TRIS, rng, 0.25, False)
    p = m0.positions.copy()
    p[:, 0] = np.abs(p[:, 0]) - np.float32(mc.WIDTH / 4)
    p[:, 2] += np.where(m0.positions[:, 0] < 0, np.float32(0.05), np.float32(0.0))  # (in front, not coplanar)
    return mc._pair([(m0, Mesh(p, m0.normals, m0.uvs, m0.indices))], [(0, mc._centred(1.5))])


OWN = {"small_32": _small, "small_35": _small, "deep_17": _deep, "deep_65": _deep, "folded": _folded}
CASES = FROM_MESH_CASES + list(OWN)
ARRAY_CASES = list(CASES)
FRAME_CASES = ["tris_1281", "many_meshes", "emissive_mesh", "shared_mesh", "neg_zero", "keep_normals", "folded"]
VARIANT_CASES = FRAME_CASES[:3]  # also under lds_scene 0 / 1 / 2 and leaf_collapse 0
REPEAT_CASES = ["small_35", "tris_1281", "many_meshes"]
FRAME_SIZE = mc.FRAME_SIZE

_made = {}
_refitted = {}


def listed(name: str) -> list:
    return mc.listed(name)


def case(name: str):
    """(scene0, scene1), made once per process; scene0 is built."""
    if name in FROM_MESH_CASES:
        return mc.case(name)
    if name not in _made:
        scene0, scene1 = OWN[name](name)
        scene0.build()
        _made[name] = (scene0, scene1)
    return _made[name]


def built1(name: str):
    """scene1's host-built desc (the REBUILT scene: what hk_update_meshes gives): the scene's own current one, built
    once.  A desc's pointers die with the next build of its scene, so none is kept here past the scene's."""
    scene1 = case(name)[1]
    return scene1.desc if scene1.desc is not None else scene1.build()


def update_source(name: str, which: int = 1):
    return mc.update_source(name, which) if name in FROM_MESH_CASES else case(name)[which]


def refitted(name: str):
    """The expected scene of the case's refit: Scene.refitted(scene0's desc, scene1, the listed meshes), made once for
    the two scenes' current builds."""
    from hikari_amd import Scene
    scene0, scene1 = case(name)
    built = (scene0.desc, built1(name))
    if name not in _refitted or any(a is not b for a, b in zip(_refitted[name][0], built)):
        _refitted[name] = (built, Scene.refitted(scene0.desc, scene1, listed(name)))
    return _refitted[name][1]


def camera_for(name: str):
    return mc.camera_for(name)


def spans(nodes) -> np.ndarray:
    """exit - i of every entry node of a slice (parity.NODE_DT records)."""
    inner = nodes["entry"] < 0x80000000
    return (nodes["exit"].astype(np.int64) - np.arange(len(nodes)))[inner]
