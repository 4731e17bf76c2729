"""Cases for the GPU mesh rebuild (hk_update_meshes, csrc/hk_dynamic.hip), shared by tests/test_mesh_cases.py (CPU: the
host builder alone proves that every case sits on the edge its name says) and tests/test_gpu_mesh_update.py (GPU: the
rebuilt arrays byte for byte against the host builder's, frames against the oracle).

A case is a pair (scene0, scene1) with identical topology, instances and materials: scene0 is what is uploaded,
scene1 has other vertex positions (and, but for keep_normals, other normals) in the meshes LISTED[name] names: the host
builder's scene for the update and the source of the positions and normals that update_meshes sends.  The deformed
meshes are grids in the plane z = 0 in front of the camera, indexed triangle lists that share their vertices, whose
vertices a seeded field moves by a few cells: far enough to reorder the triangles' centroids, so the rebuilt BLAS is
another tree (tests/test_mesh_cases.py), not the old one refitted.  Every scene has one small emissive quad, so the
frames are lit.  Everything is seeded.

The limits the sizes straddle are counts of shapes in hk_dynamic.hip, as in tests/dynamic_cases.py: COOP_MIN = 128,
256 (one chunk of the ballot ranking), BVH_LDS_SHAPES = 1280 (k_build_mesh_bvh<true> up to it, <false> above).
"""
from __future__ import annotations

import math

import numpy as np

from dynamic_cases import BVH_LDS_SHAPES, COOP_MIN, FRAME_SIZE, GB_STACK, GB_STACK_LDS, _rot, _trs  # noqa: F401

SEED = 0x4D455348  # "MESH"
WIDTH, HEIGHT = 2.6, 2.0  # extent of a deformed grid, centred on (0, 1, 0): about a third of the camera's view


# ------------------------------------------------------------------ meshes
def _grid_shape(tris: int):
    cells = (tris + 1) // 2
    cols = max(1, int(math.ceil(math.sqrt(cells * WIDTH / HEIGHT))))
    return cols, int(math.ceil(cells / cols))


def _grid_indices(tris: int) -> np.ndarray:
    """The first `tris` triangles of a cols x rows grid of cells, two per cell, counter-clockwise seen from +z; vertex
    (r, c) is r * (cols + 1) + c.  An odd count leaves the last cell half covered."""
    cols, rows = _grid_shape(tris)
    idx = []
    for r in range(rows):
        for c in range(cols):
            a, b = r * (cols + 1) + c, (r + 1) * (cols + 1) + c
            idx += [a, a + 1, b + 1, a, b + 1, b]
    return np.array(idx[: 3 * tris], np.uint32)


def _grid_mesh(tris: int, rng, amp: float, bend: bool, width: float = WIDTH, height: float = HEIGHT):
    """The grid with every vertex moved by a normal field of `amp` cells in the plane and 0.1 amp cells out of it; bend:
    seeded normals that lean up to about 30 degrees off +z (else +z)."""
    from hikari_amd import Mesh
    cols, rows = _grid_shape(tris)
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, cols + 1) * width, np.linspace(-0.5, 0.5, rows + 1) * height)
    pos = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)
    cell = np.array([width / cols, height / rows, min(width / cols, height / rows) * 0.1])
    pos += rng.normal(size=pos.shape) * cell[None, :] * amp
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]]), (len(pos), 1))
    if bend:
        nrm[:, :2] += rng.uniform(-0.5, 0.5, (len(pos), 2))
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    uv = np.stack([x.ravel() / width + 0.5, 0.5 - y.ravel() / height], axis=1)
    return Mesh(pos.astype(np.float32), nrm.astype(np.float32), uv.astype(np.float32), _grid_indices(tris))


def _grid_pair(tris: int, rng, **kw):
    """(mesh0, mesh1): the grid mildly and strongly deformed."""
    return _grid_mesh(tris, rng, 0.25, False, **kw), _grid_mesh(tris, rng, 2.5, True, **kw)


def _soup(corners):
    """A triangle list with its own three vertices per triangle: corners (n, 3, 3)."""
    from hikari_amd import Mesh
    pos = np.asarray(corners, np.float32).reshape(-1, 3)
    n = len(pos) // 3
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3 * n, 1))
    uv = np.tile(np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]], np.float32), (n, 1))
    return Mesh(pos, nrm, uv, np.arange(3 * n, dtype=np.uint32))


def _row_soup(n: int, width: float = WIDTH, hy: float = 0.5):
    """n equal triangles side by side along x: a shallow tree."""
    e = np.linspace(-0.5, 0.5, n + 1) * width
    return _soup([[[e[i], -hy, 0.0], [e[i + 1], -hy, 0.0], [0.5 * (e[i] + e[i + 1]), hy, 0.0]] for i in range(n)])


def _deep_soup(n: int, ratio: float = 4.0, first: int = -8):
    """n triangles at distances d = ratio^(first + i) along +x with half extent 0.45 d: the binned SAH peels the
    largest off per split, so the tree has n - 1 inner levels (checked against the host builder)."""
    out = []
    for i in range(n):
        d = ratio ** (first + i)
        h = 0.45 * d
        out.append([[d - h, -h, 0.0], [d + h, -h, 0.0], [d, h, 0.0]])
    return _soup(out)


TOO_DEEP_TRIS = 129
AXES = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)]


def _axes_soup(n: int, ratio: float = 4.0, bottom: float = 2e-6, half: float = 0.3):
    """Triangle k at the distance d = bottom * ratio^(k // 4) from the origin along +x, -x, +y, -y in turn, with half
    extent half * d, as dynamic_cases._deep places instances: about one inner level per two triangles, within float32's
    range at 64 levels (count found by search against the host builder)."""
    out = []
    for k in range(n):
        d = bottom * ratio ** (k // 4)
        h, (ax, ay) = half * d, AXES[k % 4]
        out.append([[d * ax - h, d * ay - h, 0.0], [d * ax + h, d * ay - h, 0.0], [d * ax, d * ay + h, 0.0]])
    return _soup(out)


# ------------------------------------------------------------------ scenes
FACE = np.eye(3)
CENTRE = (0.0, 1.0, 0.0)
LIGHT = (1.0, 0.9, 0.7, 0.4)


def _pair(mesh_pairs, instances, lit=()):
    """(scene0, scene1): mesh k is mesh_pairs[k][0] / [1]; instances: [(mesh, model)], grey but for the instance
    indices in `lit`, which are emitters; and last the light: an emissive quad above and in front of the meshes, facing
    them."""
    from hikari_amd import Scene, StandardMaterial, plane_mesh
    scenes = []
    for which in (0, 1):
        s = Scene()
        for pair in mesh_pairs:
            s.add_mesh(pair[which])
        quad = s.add_mesh(plane_mesh(0.6))
        grey = s.add_material(StandardMaterial(base_color=(0.7, 0.65, 0.6, 1.0), perceptual_roughness=0.8))
        glow = s.add_material(StandardMaterial(base_color=(1.0, 1.0, 1.0, 1.0), emissive=LIGHT))
        for k, (mesh, model) in enumerate(instances):
            s.add_instance(mesh, glow if k in lit else grey, model)
        s.add_instance(quad, glow, _trs((1.7, 2.3, 2.0), _rot([1, 0, 0], -0.75 * math.pi), np.ones(3)))
        scenes.append(s)
    return tuple(scenes)


def _centred(scale: float = 1.0):
    return _trs(CENTRE, FACE, np.full(3, scale))


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


def _tris(n: int):
    def make(name):
        return _pair([_grid_pair(n, _rng(name))], [(0, _centred())])
    return make


MANY_SIZES = [3, 17, 130, 1281, 64, 1, 257, 40, 2, 700, 1400, 12, 129, 90, 5, 300, 1700, 33, 128, 8,
              256, 70, 1280, 21, 2000, 150, 4, 500, 65, 11, 1300, 27, 200, 9, 1000, 45, 6, 350, 80, 19]
MANY_COLS = 8


def _many_meshes(name):
    rng = _rng(name)
    pairs = [_grid_pair(n, rng, width=1.0, height=1.0) for n in MANY_SIZES]
    inst = []
    for k in range(len(pairs)):
        at = (-1.4 + 0.4 * (k % MANY_COLS), 0.2 + 0.4 * (k // MANY_COLS), 0.0)
        inst.append((k, _trs(at, FACE, np.full(3, 0.36))))
    return _pair(pairs, inst)


def _one_of_three(name):
    rng = _rng(name)
    left, right = _grid_mesh(100, rng, 0.25, False, width=0.8), _grid_mesh(120, rng, 0.25, True, width=0.8)
    inst = [(k, _trs((-0.9 + 0.9 * k, 1.0, 0.0), FACE, np.ones(3))) for k in range(3)]
    return _pair([(left, left), _grid_pair(150, rng, width=0.8), (right, right)], inst)


def _shared_mesh(name):
    rng = _rng(name)
    inst = []
    for k in range(5):
        r = _rot([0, 1, 0], rng.uniform(-0.6, 0.6)) @ _rot([0, 0, 1], rng.uniform(-1.0, 1.0))
        inst.append((0, _trs((-1.2 + 0.6 * k, 0.5 + 0.25 * k, -0.3 * (k % 2)), r, np.full(3, rng.uniform(0.35, 0.6)))))
    return _pair([_grid_pair(200, rng)], inst)


EMISSIVE_TRIS = 65


def _emissive_mesh(name):
    rng = _rng(name)
    wall = _grid_mesh(60, rng, 0.25, False, width=3.2, height=2.4)
    inst = [(0, _trs((0.0, 1.0, -0.6), FACE, np.ones(3))), (1, _trs((0.0, 1.0, 0.0), FACE, np.full(3, 0.4)))]
    return _pair([(wall, wall), _grid_pair(EMISSIVE_TRIS, rng)], inst, lit=(1,))


def _coincident(n: int):
    def make(name):
        rng = _rng(name)
        # scene1: triangle i has the corners (-s, -s), (s, -s), (-s, s) with a seeded s: every box is centred on 0 exactly
        s = rng.uniform(0.2, 1.0, n)
        nested = _soup([[[-v, -v, 0.0], [v, -v, 0.0], [-v, v, 0.0]] for v in s])
        return _pair([(_row_soup(n), nested)], [(0, _centred())])
    return make


def _degenerate(name):
    rng = _rng(name)
    m0, m1 = _grid_pair(30, rng)
    p = m1.positions
    ix = m1.indices.reshape(-1, 3)
    p[ix[7]] = p[ix[7][0]]                   # a triangle of three equal corners
    a, b, c = ix[12]
    p[c] = 0.5 * (p[a] + p[b])               # three corners on a line (zero area up to rounding)
    p[ix[20][1]] = p[ix[20][0]]              # two vertices at one place
    return _pair([(m0, m1)], [(0, _centred())])


def _neg_zero(name):
    """An even grid has a column at x = 0 and a row at y = 0, and the whole mesh has z = 0: those coordinates get a
    seeded sign, vertex by vertex, so triangles and sibling boxes hold zeros of both signs; the others move as usual."""
    rng = _rng(name)
    tris = 96  # 8 x 6 cells
    cols, rows = _grid_shape(tris)
    assert cols % 2 == 0 and rows % 2 == 0
    pair = []
    for amp, bend in ((0.25, False), (0.4, True)):
        m = _grid_mesh(tris, rng, amp, bend)
        p = m.positions.reshape(rows + 1, cols + 1, 3)
        p[:, cols // 2, 0] = 0.0
        p[rows // 2, :, 1] = 0.0
        p[:, :, 2] = 0.0
        flat = m.positions
        zero = flat == 0.0
        flat[zero & (rng.random(flat.shape) < 0.5)] = -0.0
        pair.append(m)
    return _pair([tuple(pair)], [(0, _centred())])


STRIP_TRIS = 40


def _strip(name):
    from hikari_amd import Mesh
    rng = _rng(name)
    n = STRIP_TRIS + 2
    pair = []
    for amp in (0.1, 1.5):
        x = (np.arange(n) // 2) / (n // 2 - 1) - 0.5
        pos = np.stack([x * WIDTH, (np.arange(n) % 2 - 0.5) * 1.2, np.zeros(n)], axis=1)
        pos += rng.normal(size=pos.shape) * np.array([WIDTH / (n // 2), 0.1, 0.02])[None, :] * amp
        nrm = np.tile(np.array([[0.0, 0.0, 1.0]]), (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3)) * amp
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        uv = np.stack([x + 0.5, np.arange(n) % 2], axis=1)
        pair.append(Mesh(pos.astype(np.float32), nrm.astype(np.float32), uv.astype(np.float32),
                         np.arange(n, dtype=np.uint32), 1))
    return _pair([tuple(pair)], [(0, _centred())])


def _keep_normals(name):
    rng = _rng(name)
    m0 = _grid_mesh(150, rng, 0.25, True)
    m1 = _grid_mesh(150, rng, 2.5, False)
    m1.normals = m0.normals.copy()  # the host's scene1 carries the normals the update leaves alone
    return _pair([(m0, m1)], [(0, _centred())])


# (triangles of the deep mesh): its BLAS has one inner level less; the TLAS over the mesh and the light adds one
DEEPEN = {"deepen_16": 16, "deepen_17": 17}
SHALLOWER = (11, 6)  # triangles of the mesh that becomes shallow and of the one that stays as deep as it is


def _deepen(name):
    n = DEEPEN[name]
    return _pair([(_row_soup(n), _deep_soup(n))], [(0, _centred())])


def _too_deep(name):
    """scene1's BLAS has 64 inner levels: with the TLAS's one the bound is 65, one past what the G-buffer walk takes."""
    n = TOO_DEEP_TRIS
    return _pair([(_row_soup(n, hy=0.9), _axes_soup(n))], [(0, _centred())])  # (scene0: a sixth of the view)


def _shallower(name):
    a, b = SHALLOWER
    keep = _deep_soup(b)
    inst = [(0, _trs((0.0, 1.4, 0.0), FACE, np.ones(3))), (1, _trs((0.0, 0.6, 0.0), FACE, np.ones(3)))]
    return _pair([(_deep_soup(a), _row_soup(a, hy=0.3)), (keep, keep)], inst)


SIZES = {f"tris_{n}": n for n in (1, 2, 128, 129, 256, 257, 1280, 1281, 2600)}
CASES = {
    **{name: _tris(n) for name, n in SIZES.items()},
    "many_meshes": _many_meshes, "one_of_three": _one_of_three, "shared_mesh": _shared_mesh,
    "emissive_mesh": _emissive_mesh, "coincident_100": _coincident(100), "coincident_300": _coincident(300),
    "degenerate": _degenerate, "neg_zero": _neg_zero, "strip": _strip, "keep_normals": _keep_normals,
    "deepen_16": _deepen, "deepen_17": _deepen, "shallower": _shallower, "too_deep": _too_deep,
}
# the meshes an update lists (default: mesh 0)
LISTED = {"many_meshes": list(range(len(MANY_SIZES))), "one_of_three": [1], "emissive_mesh": [1]}
COINCIDENT = {"coincident_100": 100, "coincident_300": 300}
ARRAY_CASES = list(CASES)
SECOND_UPDATE_CASES = ["tris_257", "tris_1281", "many_meshes"]
FRAME_CASES = ["tris_129", "tris_1281", "many_meshes", "emissive_mesh", "shared_mesh", "neg_zero", "keep_normals"]
VARIANT_CASES = FRAME_CASES[:3]  # also under lds_scene 0 / 1 / 2 and leaf_collapse 0


def listed(name: str) -> list:
    return LISTED.get(name, [0])


def camera_for(name: str):
    """(camera, lights) of a case's frames: in front of the plane z = 0 the meshes lie in, looking at their centre."""
    from hikari_amd import Camera, Transform, make_lights
    return Camera(Transform.from_xyz(0.0, 1.0, 4.0).looking_at(CENTRE)), make_lights(None)


_made = {}


def case(name: str):
    """(scene0, scene1) of a case, made once per process; scene0 is built (scene0.desc)."""
    if name not in _made:
        scene0, scene1 = CASES[name](name)
        scene0.build()
        _made[name] = (scene0, scene1)
    return _made[name]


_built1 = {}


def built1(name: str):
    """scene1's host-built desc, once per process."""
    if name not in _built1:
        _built1[name] = case(name)[1].build()
    return _built1[name]


def update_source(name: str, which: int = 1):
    """The scene update_meshes takes the case's new positions and normals from: scene `which` of the pair; for
    keep_normals a copy whose meshes have no normals (normals = NULL: the uploaded ones stay)."""
    scene = case(name)[which]
    if name != "keep_normals":
        return scene
    from hikari_amd import Mesh, Scene
    s = Scene()
    s.meshes = [Mesh(m.positions, None, m.uvs, m.indices, m.topology) for m in scene.meshes]
    s.materials, s.instances = scene.materials, scene.instances
    return s


def local_aabbs(scene) -> np.ndarray:
    """(n, 6) Bevy `Aabb` of each instance's mesh as the host builder folds it (hks_add_mesh: std::fmin / std::fmax over
    the vertices in order, which keep the second of two equal operands): Scene.instance_local_aabbs() with a bound of
    0 taking the sign of the mesh's last vertex that has a zero there."""
    out = np.empty((len(scene.instances), 6), np.float32)
    for i, (mesh, _, _) in enumerate(scene.instances):
        p = np.asarray(scene.meshes[mesh].positions, np.float32)
        mn, mx = p.min(axis=0), p.max(axis=0)
        for k in range(3):
            zeros = p[p[:, k] == 0.0, k]
            if mn[k] == 0.0:
                mn[k] = zeros[-1]
            if mx[k] == 0.0:
                mx[k] = zeros[-1]
        out[i] = np.concatenate([(mn + mx) * np.float32(0.5), (mx - mn) * np.float32(0.5)])
    return out


# ------------------------------------------------------------------ reading the built arrays
def mesh_slices(desc) -> list:
    """[(vertex, primitive, node0, node_count)] of every instance of a host-built scene (hk_instance.mesh)."""
    from parity import host_scene_array
    inst = np.frombuffer(host_scene_array(desc, 4, np.dtype((np.void, 176))).tobytes(), np.uint32).reshape(-1, 44)
    return [tuple(int(v) for v in row[40:44]) for row in inst]


def mesh_nodes(desc, index):
    """The BLAS of the mesh with hk_mesh_index `index` in a host-built scene (parity.NODE_DT records)."""
    from parity import NODE_DT, host_scene_array
    return host_scene_array(desc, 2, NODE_DT)[index[2]: index[2] + index[3]]
