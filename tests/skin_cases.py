"""Cases for skinned meshes (hk_set_mesh_skins / hk_skin_meshes, csrc/hk_dynamic.hip k_skin_vertices and k_skin_bounds),
shared by tests/test_skin_cases.py (CPU: the host builder alone proves that every case sits on the edge its name says)
and tests/test_gpu_skin.py (GPU: the posed arrays byte for byte against the host builder's, frames against the oracle).

A case is a scene in its bind pose (what is uploaded), the meshes whose skins are registered, and one or two poses
{mesh id: joint palette}.  The host scene of pose k is Scene.posed(poses[k]): hks_skin_vertices' output in the posed
meshes.  The meshes are the deformed grids of tests/mesh_cases.py (its helpers are imported, not edited) rigged with
seeded joint indices and weights: every vertex follows its own four joints, and the joints move by a few cells, so the
posed triangles' centroids reorder and the rebuilt BLAS is another tree, not the bind pose's refitted.  Everything is
seeded.

The sizes straddle the edges of the per-vertex kernels and of the bounds reduction: vertex counts 3, 63, 64, 65 (a
wave), 256, 257 (a workgroup, one stride of k_skin_bounds' loop); 1,281 triangles for the global-memory BLAS build
(BVH_LDS_SHAPES = 1280) fed from a device source.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import mesh_cases as mc
from dynamic_cases import BVH_LDS_SHAPES, FRAME_SIZE, _rot, _trs  # noqa: F401

SEED = 0x534B494E  # "SKIN"
VERTEX_SIZES = (3, 63, 64, 65, 256, 257)
BIG_TRIS = BVH_LDS_SHAPES + 1
MANY_TRIS = [8, 40, 130, 600, 17, 64, 129, 257, 5, 90, 200, 33]
MANY_JOINTS = [1, 2, 7, 256]
MANY_COLS = 6


@dataclass
class Case:
    scene0: object                 # hikari_amd.Scene in its bind pose, built
    skinned: list                  # mesh ids whose skins are registered
    poses: list                    # [{mesh id: (joint_count, 16) float32}], one or two
    keep_normals: tuple = ()       # mesh ids registered with normals = NULL
    _posed: dict = field(default_factory=dict)


# ------------------------------------------------------------------ rigs and palettes
def col_major(m) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(m, np.float64).T.reshape(16).astype(np.float32))


def rig(mesh, rng, joints: int):
    """Seeded Uint16x4 indices below `joints` and Float32x4 weights that sum to about 1; with 256 joints, index 255 is
    used."""
    from hikari_amd import Skin
    n = len(mesh.positions)
    ix = rng.integers(0, joints, (n, 4)).astype(np.uint16)
    if joints == 256:
        ix[0, 0] = 255
    mesh.skin = Skin(ix, rng.dirichlet(np.ones(4), n).astype(np.float32), joints)
    return mesh


def cell_of(mesh) -> float:
    p = np.asarray(mesh.positions, np.float64)
    ext = p.max(axis=0) - p.min(axis=0)
    return math.sqrt(max(ext[0] * ext[1], 1e-6) / max(len(p), 1))


def palette(rng, joints: int, cell: float, amp: float = 2.5, scale=(1.0, 1.0)) -> np.ndarray:
    """(joints, 16) column-major: each joint a rotation of up to 0.6 rad about a seeded axis through the mesh's origin,
    a seeded scale per axis from `scale`, and a translation of up to `amp` cells in the plane, a tenth of it out."""
    out = []
    for _ in range(joints):
        lin = _rot(rng.normal(size=3), rng.uniform(-0.6, 0.6)) @ np.diag(rng.uniform(scale[0], scale[1], 3))
        t = rng.uniform(-1.0, 1.0, 3) * cell * amp * np.array([1.0, 1.0, 0.1])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = lin, t
        out.append(col_major(m))
    return np.stack(out)


def _band_mesh(n: int, rng):
    """n vertices in two rows (as mesh_cases._strip places them), an indexed triangle LIST of the n - 2 triangles
    (i, i + 1, i + 2) that share them: any vertex count from 3."""
    from hikari_amd import Mesh
    half = max(1, (n + 1) // 2 - 1)
    x = (np.arange(n) // 2) / half - 0.5
    pos = np.stack([x * mc.WIDTH, (np.arange(n) % 2 - 0.5) * 1.2, np.zeros(n)], axis=1)
    pos += rng.normal(size=pos.shape) * np.array([mc.WIDTH / (half + 1), 0.1, 0.02])[None, :] * 0.1
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    uv = np.stack([x + 0.5, np.arange(n) % 2], axis=1)
    idx = np.stack([np.arange(n - 2), np.arange(n - 2) + 1, np.arange(n - 2) + 2], axis=1).reshape(-1)
    return Mesh(pos.astype(np.float32), nrm.astype(np.float32), uv.astype(np.float32), idx.astype(np.uint32))


def _scene(meshes, instances, lit=()):
    """mesh_cases._pair's scene (grey instances, the emitters in `lit`, and the emissive quad last) of these meshes."""
    return mc._pair([(m, m) for m in meshes], instances, lit)[0]


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


# ------------------------------------------------------------------ the cases
def _verts(n: int):
    def make(name):
        rng = _rng(name)
        m = rig(_band_mesh(n, rng), rng, 4)
        cell = mc.WIDTH / max(2, n // 2)
        return Case(_scene([m], [(0, mc._centred())]), [0], [{0: palette(rng, 4, cell)}, {0: palette(rng, 4, cell)}])
    return make


def _big(name):
    rng = _rng(name)
    m = rig(mc._grid_mesh(BIG_TRIS, rng, 0.25, True), rng, 12)
    return Case(_scene([m], [(0, mc._centred())]), [0], [{0: palette(rng, 12, cell_of(m))}, {0: palette(rng, 12, cell_of(m))}])


def _many_skins(name):
    rng = _rng(name)
    meshes, inst = [], []
    for k, tris in enumerate(MANY_TRIS):
        joints = MANY_JOINTS[k % len(MANY_JOINTS)]
        meshes.append(rig(mc._grid_mesh(tris, rng, 0.25, True, width=1.0, height=1.0), rng, joints))
        at = (-1.25 + 0.5 * (k % MANY_COLS), 0.5 + 0.8 * (k // MANY_COLS), 0.0)
        inst.append((k, _trs(at, mc.FACE, np.full(3, 0.42))))
    poses = [{k: palette(rng, m.skin.joint_count, cell_of(m), scale=(0.8, 1.3)) for k, m in enumerate(meshes)}
             for _ in range(2)]
    return Case(_scene(meshes, inst), list(range(len(meshes))), poses)


def _one_of_three(name):
    rng = _rng(name)
    left = rig(mc._grid_mesh(100, rng, 0.25, False, width=0.8), rng, 3)   # skinned, not posed
    mid = rig(mc._grid_mesh(150, rng, 0.25, True, width=0.8), rng, 5)     # skinned and posed
    right = mc._grid_mesh(120, rng, 0.25, True, width=0.8)                # no skin
    inst = [(k, _trs((-0.9 + 0.9 * k, 1.0, 0.0), mc.FACE, np.ones(3))) for k in range(3)]
    return Case(_scene([left, mid, right], inst), [0, 1], [{1: palette(rng, 5, cell_of(mid))}])


def _shared_mesh(name):
    rng = _rng(name)
    m = rig(mc._grid_mesh(200, rng, 0.25, True), rng, 6)
    inst = []
    for k in range(5):
        r = _rot([0, 1, 0], rng.uniform(-0.6, 0.6)) @ _rot([0, 0, 1], rng.uniform(-1.0, 1.0))
        inst.append((0, _trs((-1.2 + 0.6 * k, 0.5 + 0.25 * k, -0.3 * (k % 2)), r, np.full(3, rng.uniform(0.35, 0.6)))))
    return Case(_scene([m], inst), [0], [{0: palette(rng, 6, cell_of(m))}])


EMISSIVE_TRIS = 65


def _emissive_skin(name):
    rng = _rng(name)
    wall = mc._grid_mesh(60, rng, 0.25, False, width=3.2, height=2.4)
    m = rig(mc._grid_mesh(EMISSIVE_TRIS, rng, 0.25, True), rng, 4)
    inst = [(0, _trs((0.0, 1.0, -0.6), mc.FACE, np.ones(3))), (1, _trs((0.0, 1.0, 0.0), mc.FACE, np.full(3, 0.4)))]
    return Case(_scene([wall, m], inst, lit=(1,)), [1], [{1: palette(rng, 4, cell_of(m), scale=(0.7, 1.5))}])


def _scaled_joint(name):
    """Joints with a non-uniform scale of up to 3 : 1 under a rotation: mat3(M) and its inverse transpose send the
    normals to different places, and the picture shows which one was used."""
    rng = _rng(name)
    m = rig(mc._grid_mesh(150, rng, 0.25, True), rng, 5)
    return Case(_scene([m], [(0, mc._centred())]), [0], [{0: palette(rng, 5, cell_of(m), amp=1.5, scale=(0.5, 1.6))}])


FLAT_TRIS = 96  # 8 x 6 cells: a column at x = 0 and a row at y = 0


def _flat_zero(name):
    """A grid in the plane z = +0 exactly, posed by joints whose z row is (-0, -0, -s, -0): z' is -0 where the vertex's
    x and y are positive and +0 elsewhere (one +0 term wins the sum), so triangles, sibling boxes and the mesh's bounds
    hold zeros of both signs; x and y move as in the other cases and then by (3, 3), so the posed Aabb's centre has
    positive x and y.  The instance's model has the same z row (a mirror in z, brought back in front of the camera):
    the world centre's z is ((-0 cx + -0 cy) + -1 cz) + -0, which is +0 for the rule's cz = -0 (the last vertex's zero)
    and -0 for the +0 a sign-blind minimum and maximum would centre on, and the record's min.z and max.z are -0 plus
    that: the sign rule of the device's bounds reduction shows in the instance record and the TLAS."""
    rng = _rng(name)
    m = mc._grid_mesh(FLAT_TRIS, rng, 0.25, True)
    m.positions[:, 2] = 0.0
    m = rig(m, rng, 3)
    pal = palette(rng, 3, cell_of(m), amp=1.0)
    for j in pal:
        s = rng.uniform(0.5, 1.5)
        j[[2, 6, 10, 14]] = [-0.0, -0.0, -s, -0.0]   # row z of the columns
        j[[8, 9]] = 0.0                               # z does not reach x and y
        j[[12, 13]] += 3.0
    model = _trs((-3.0, -2.0, 0.0), mc.FACE, np.ones(3))
    model[2] = [-0.0, -0.0, -1.0, -0.0]
    return Case(_scene([m], [(0, model)]), [0], [{0: pal}])


def _keep_normals(name):
    rng = _rng(name)
    m = rig(mc._grid_mesh(150, rng, 0.25, True), rng, 4)
    return Case(_scene([m], [(0, mc._centred())]), [0], [{0: palette(rng, 4, cell_of(m))}], keep_normals=(0,))


CASES = {
    **{f"verts_{n}": _verts(n) for n in VERTEX_SIZES},
    "tris_1281": _big, "many_skins": _many_skins, "one_of_three": _one_of_three, "shared_mesh": _shared_mesh,
    "emissive_skin": _emissive_skin, "scaled_joint": _scaled_joint, "flat_zero": _flat_zero,
    "keep_normals": _keep_normals,
}
SECOND_POSE_CASES = ["verts_257", "tris_1281", "many_skins"]
FRAME_CASES = ["scaled_joint", "emissive_skin", "shared_mesh"]

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
        s = c.scene0.posed(c.poses[k], c.keep_normals)
        c._posed[k] = (s, s.build())
    return c._posed[k]


# ------------------------------------------------------------------ the caller's boxes
WRONG_BOX = np.array([9.0, -7.0, 5.0, 123.0, 0.5, 77.0], np.float32)


def caller_aabbs(scene, posed_meshes) -> np.ndarray:
    """mesh_cases.local_aabbs of the scene as given (the bind pose), with WRONG_BOX in the rows the library derives:
    hk_skin_meshes ignores the caller's box of a posed mesh's instances."""
    a = mc.local_aabbs(scene)
    for i, (mesh, _, _) in enumerate(scene.instances):
        if mesh in posed_meshes:
            a[i] = WRONG_BOX
    return a
