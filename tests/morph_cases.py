"""Cases for morph targets (hk_set_mesh_morphs / hk_morph_meshes, csrc/hk_dynamic.hip k_morph_vertices and
k_skin_bounds), shared by tests/test_morph_cases.py (CPU: the host builder alone proves that every case sits on the edge
its name says) and tests/test_gpu_morph.py (GPU: the posed arrays byte for byte against the host builder's, frames
against the oracle).

A case is a base scene (what is uploaded), the meshes whose morphs (and skins) are registered, and one or two poses
{mesh id: weights} or {mesh id: (weights, joints)}.  The host scene of pose k is Scene.morphed(poses[k]):
hks_morph_vertices' output (then hks_skin_vertices') in the posed meshes.  The meshes are those of tests/skin_cases.py
and tests/mesh_cases.py (their helpers are imported, not edited) with seeded target-major deltas: every vertex of every
target moves on its own by a few cells, so the posed triangles' centroids reorder and the rebuilt BLAS is another tree,
not the base's refitted.  Every posed vertex is finite (NaN is exercised at the rule level, tests/test_morph_independent.py).
Everything is seeded.

The sizes straddle the edges of the per-vertex kernel and of the bounds reduction (vertex counts 3, 63, 64, 65, 256, 257)
and of the kernel's batched loop over the active list: active counts 0, 1, B - 1, B, B + 1.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import mesh_cases as mc
import skin_cases as sc
from dynamic_cases import BVH_LDS_SHAPES, _trs  # noqa: F401
from skin_cases import caller_aabbs, cell_of  # noqa: F401

SEED = 0x4D4F5250  # "MORP"
FRAME_SIZE = (64, 48)
B = 4  # csrc/hk_launch.h MORPH_BATCH: the targets whose loads k_morph_vertices issues before a batch's first add
VERTEX_SIZES = sc.VERTEX_SIZES
ACTIVE_COUNTS = (0, 1, B - 1, B, B + 1)
ACTIVE_TARGETS = 8
BIG_TRIS = BVH_LDS_SHAPES + 1
MANY_TRIS = sc.MANY_TRIS
MANY_TARGETS = [1, 2, 7, 16]


@dataclass
class Case:
    scene0: object                 # hikari_amd.Scene, the base, built
    morphed: list                  # mesh ids whose morphs are registered
    poses: list                    # [{mesh id: weights (targets,) f32, or (weights, joints (joint_count, 16) f32)}]
    skinned: list = field(default_factory=list)  # mesh ids whose skins are registered too
    keep_normals: tuple = ()       # mesh ids registered with normals = NULL
    _posed: dict = field(default_factory=dict)


# ------------------------------------------------------------------ targets and weights
def targets(mesh, rng, count: int, cell: float, amp: float = 2.5, normal_deltas: bool = True):
    """Seeded target-major deltas: every vertex of every target moves by up to `amp` cells in the plane, a tenth of it
    out; the normal deltas up to 0.4 per component."""
    from hikari_amd import Morph
    n = len(mesh.positions)
    dp = rng.uniform(-1.0, 1.0, (count, n, 3)) * cell * amp * np.array([1.0, 1.0, 0.1])
    dn = rng.uniform(-0.4, 0.4, (count, n, 3)).astype(np.float32) if normal_deltas else None
    mesh.morph = Morph(dp.astype(np.float32), dn)
    return mesh


def weights(rng, count: int, active=None) -> np.ndarray:
    """(count,) f32: the targets in `active` (default: all) weigh 0.4 .. 1.0 with a seeded sign, the others are zeros of
    alternating sign."""
    w = np.zeros(count, np.float32)
    w[1::2] = -0.0
    on = range(count) if active is None else active
    for t in on:
        w[t] = rng.uniform(0.4, 1.0) * rng.choice([-1.0, 1.0])
    return w


def active_of(w) -> list:
    return [t for t, x in enumerate(np.asarray(w, np.float32)) if x != 0]


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


_scene = sc._scene


# ------------------------------------------------------------------ the cases
def _verts(n: int):
    def make(name):
        rng = _rng(name)
        m = targets(sc._band_mesh(n, rng), rng, 3, mc.WIDTH / max(2, n // 2), amp=1.5)
        return Case(_scene([m], [(0, mc._centred())]), [0], [{0: weights(rng, 3)}, {0: weights(rng, 3)}])
    return make


def _active(k: int):
    def make(name):
        rng = _rng(name)
        m = mc._grid_mesh(150, rng, 0.25, True)
        m = targets(m, rng, ACTIVE_TARGETS, cell_of(m), amp=1.5)
        on = sorted(rng.choice(ACTIVE_TARGETS, k, replace=False).tolist())
        return Case(_scene([m], [(0, mc._centred())]), [0], [{0: weights(rng, ACTIVE_TARGETS, on)}])
    return make


def _targets_256(name):
    rng = _rng(name)
    m = mc._grid_mesh(40, rng, 0.25, True)
    m = targets(m, rng, 256, cell_of(m))
    return Case(_scene([m], [(0, mc._centred())]), [0], [{0: weights(rng, 256, [9, 130, 255])}])


def _big(name):
    rng = _rng(name)
    m = mc._grid_mesh(BIG_TRIS, rng, 0.25, True)
    m = targets(m, rng, 3, cell_of(m), amp=2.0)
    return Case(_scene([m], [(0, mc._centred())]), [0], [{0: weights(rng, 3)}, {0: weights(rng, 3, [0, 2])}])


def _many_morphs(name):
    rng = _rng(name)
    meshes, inst = [], []
    for k, tris in enumerate(MANY_TRIS):
        m = mc._grid_mesh(tris, rng, 0.25, True, width=1.0, height=1.0)
        meshes.append(targets(m, rng, MANY_TARGETS[k % len(MANY_TARGETS)], cell_of(m), amp=1.5, normal_deltas=k % 3 != 1))
        at = (-1.25 + 0.5 * (k % sc.MANY_COLS), 0.5 + 0.8 * (k // sc.MANY_COLS), 0.0)
        inst.append((k, _trs(at, mc.FACE, np.full(3, 0.42))))

    def pose():
        out = {}
        for k, m in enumerate(meshes):
            t = m.morph.target_count
            on = None if t <= 2 else sorted(rng.choice(t, min(t, 2 + k % 5), replace=False).tolist())
            out[k] = weights(rng, t, on)
        return out
    return Case(_scene(meshes, inst), list(range(len(meshes))), [pose(), pose()])


def _one_of_three(name):
    rng = _rng(name)
    left = mc._grid_mesh(100, rng, 0.25, False, width=0.8)   # morphed, not posed
    left = targets(left, rng, 2, cell_of(left))
    mid = mc._grid_mesh(150, rng, 0.25, True, width=0.8)     # morphed and posed
    mid = targets(mid, rng, 5, cell_of(mid))
    right = mc._grid_mesh(120, rng, 0.25, True, width=0.8)   # no morph
    inst = [(k, _trs((-0.9 + 0.9 * k, 1.0, 0.0), mc.FACE, np.ones(3))) for k in range(3)]
    return Case(_scene([left, mid, right], inst), [0, 1], [{1: weights(rng, 5, [0, 2, 3])}])


def _shared_mesh(name):
    rng = _rng(name)
    m = mc._grid_mesh(200, rng, 0.25, True)
    m = targets(m, rng, 4, cell_of(m))
    inst = []
    for k in range(5):
        r = sc._rot([0, 1, 0], rng.uniform(-0.6, 0.6)) @ sc._rot([0, 0, 1], rng.uniform(-1.0, 1.0))
        inst.append((0, _trs((-1.2 + 0.6 * k, 0.5 + 0.25 * k, -0.3 * (k % 2)), r, np.full(3, rng.uniform(0.35, 0.6)))))
    return Case(_scene([m], inst), [0], [{0: weights(rng, 4, [1, 3])}])


def _emissive_morph(name):
    rng = _rng(name)
    wall = mc._grid_mesh(60, rng, 0.25, False, width=3.2, height=2.4)
    m = mc._grid_mesh(sc.EMISSIVE_TRIS, rng, 0.25, True)
    m = targets(m, rng, 3, cell_of(m), amp=2.0)
    inst = [(0, _trs((0.0, 1.0, -0.6), mc.FACE, np.ones(3))), (1, _trs((0.0, 1.0, 0.0), mc.FACE, np.full(3, 0.4)))]
    return Case(_scene([wall, m], inst, lit=(1,)), [1], [{1: weights(rng, 3)}])


def _flat_zero(name):
    """A grid whose base z is -0 where the vertex's x and y are positive and +0 elsewhere, shifted by (3, 3) in the plane;
    every target's z delta is -0, and the weights are positive, so z' = z + w * -0 keeps the base's sign (-0 + -0 = -0,
    +0 + -0 = +0): triangles, sibling boxes and the mesh's bounds hold zeros of both signs, while x and y move as in the
    other cases.  The instance's model is skin_cases.flat_zero's (a mirror in z whose z row is all negative zeros), so
    the sign the bounds rule gives the Aabb centre's z shows in the instance record and the TLAS."""
    rng = _rng(name)
    m = mc._grid_mesh(sc.FLAT_TRIS, rng, 0.25, True)
    neg = (m.positions[:, 0] > 0) & (m.positions[:, 1] > 0)
    m.positions[:, 2] = np.where(neg, np.float32(-0.0), np.float32(0.0))
    m = targets(m, rng, 3, cell_of(m), amp=1.0)
    m.positions[:, :2] += 3.0
    m.morph.position_deltas[:, :, 2] = -0.0
    model = _trs((-3.0, -2.0, 0.0), mc.FACE, np.ones(3))
    model[2] = [-0.0, -0.0, -1.0, -0.0]
    return Case(_scene([m], [(0, model)]), [0], [{0: np.abs(weights(rng, 3))}])


def _keep_normals(name):
    rng = _rng(name)
    m = mc._grid_mesh(150, rng, 0.25, True)
    m = targets(m, rng, 3, cell_of(m))
    return Case(_scene([m], [(0, mc._centred())]), [0], [{0: weights(rng, 3)}], keep_normals=(0,))


def _no_normal_deltas(name):
    rng = _rng(name)
    m = mc._grid_mesh(150, rng, 0.25, True)
    m = targets(m, rng, 3, cell_of(m), normal_deltas=False)
    return Case(_scene([m], [(0, mc._centred())]), [0], [{0: weights(rng, 3)}])


def _skin_65(name):
    rng = _rng(name)
    m = sc.rig(sc._band_mesh(65, rng), rng, 4)
    cell = mc.WIDTH / 32
    m = targets(m, rng, 5, cell, amp=1.0)
    poses = [{0: (weights(rng, 5, [0, 1, 2, 4]), sc.palette(rng, 4, cell, amp=1.5))} for _ in range(2)]
    return Case(_scene([m], [(0, mc._centred())]), [0], poses, skinned=[0])


def _skin_scaled(name):
    """Joints with a non-uniform scale of up to 3 : 1 under a rotation, over morphed normals: the inverse transpose is
    applied to the morphed normal, and the picture shows which one was used."""
    rng = _rng(name)
    m = sc.rig(mc._grid_mesh(150, rng, 0.25, True), rng, 5)
    m = targets(m, rng, 4, cell_of(m), amp=1.0)
    pose = {0: (weights(rng, 4, [1, 2]), sc.palette(rng, 5, cell_of(m), amp=1.0, scale=(0.5, 1.6)))}
    return Case(_scene([m], [(0, mc._centred())]), [0], [pose], skinned=[0])


CASES = {
    **{f"verts_{n}": _verts(n) for n in VERTEX_SIZES},
    **{f"active_{k}": _active(k) for k in ACTIVE_COUNTS},
    "targets_256": _targets_256, "tris_1281": _big, "many_morphs": _many_morphs, "one_of_three": _one_of_three,
    "shared_mesh": _shared_mesh, "emissive_morph": _emissive_morph, "flat_zero": _flat_zero,
    "keep_normals": _keep_normals, "no_normal_deltas": _no_normal_deltas, "skin_65": _skin_65,
    "skin_scaled": _skin_scaled,
}
SECOND_POSE_CASES = ["verts_257", "tris_1281", "many_morphs", "skin_65"]
FRAME_CASES = ["emissive_morph", "skin_scaled"]  # one morph-only case, one morph under a skin
REFIT_CASES = ["verts_3", "tris_1281"]           # the smallest and the largest slices

camera_for = mc.camera_for
_made = {}


def case(name: str) -> Case:
    """The case, made once per process; scene0 is built (scene0.desc)."""
    if name not in _made:
        c = CASES[name](name)
        c.scene0.build()
        _made[name] = c
    return _made[name]


def posed(name: str, k: int = 0):
    """(host scene of pose k, its built desc), once per process."""
    c = case(name)
    if k not in c._posed:
        s = c.scene0.morphed(c.poses[k], c.keep_normals)
        c._posed[k] = (s, s.build())
    return c._posed[k]


def parts(pose):
    """(weights, joints or None) of one mesh's pose."""
    return pose if isinstance(pose, tuple) else (pose, None)
