"""Cases for the GPU instance rebuild (hk_update_instances, csrc/hk_dynamic.hip), shared by tests/test_dynamic_cases.py
(CPU: the host builder alone proves that every case sits on the edge its name says) and tests/test_gpu_dynamic_sizes.py
(GPU: the rebuilt arrays byte for byte against the host builder's, frames against the oracle).

A case is a pair (scene0, scene1): scene0 is what is uploaded; scene1 has the same meshes, materials and instance
order with new model matrices: the host builder's scene for the update, and the source of instance_models() /
instance_local_aabbs().  Every scene is tiny in bytes: the non-emissive instances share one flat quad (two
triangles, half extents 0.08 x 0 x 0.08), the emitters are flat strips (_strip_mesh) with exactly the triangle
counts below.  Everything is seeded.

The limits the sizes straddle are counts of shapes in hk_dynamic.hip: COOP_MIN = 128 (a segment above it is split
by the whole block), 256 (one chunk of the ballot ranking), BVH_LDS_SHAPES = 1280 (the LDS build up to it, the
global-memory build above), BIG_MAX = 64 (big segments per tree level), 64 (one wave chunk of the alias over / under
compaction), ALIAS_LDS = 3072 (alias stacks in LDS up to it, in global scratch above).
"""
from __future__ import annotations

import math

import numpy as np

SEED = 0x44594E43  # "DYNC"

COOP_MIN, BALLOT_CHUNK, BVH_LDS_SHAPES, BIG_MAX, WAVE, ALIAS_LDS = 128, 256, 1280, 64, 64, 3072
GB_STACK_LDS, GB_STACK = 16, 64  # G-buffer walk: LDS stack levels, and the deepest scene it takes at all

QUAD_HALF = 0.08
BIG_OVERFLOW_N = 20000


# ------------------------------------------------------------------ meshes
def _strip_mesh(widths, hz: float = 0.06):
    """One triangle per entry of `widths`, side by side along x in the plane y = 0 (a triangle list with its own three
    vertices per triangle): triangle i has the area widths[i] * hz, so the areas are the case's to choose; a width of
    0 is a zero-area triangle.  The strip is centred on x = 0."""
    from hikari_amd import Mesh
    widths = np.asarray(widths, np.float64)
    edges = np.concatenate([[0.0], np.cumsum(widths)])
    edges -= 0.5 * edges[-1]
    n = len(widths)
    pos = np.zeros((3 * n, 3), np.float32)
    pos[0::3] = np.stack([edges[:-1], np.zeros(n), np.full(n, -hz)], axis=1)
    pos[1::3] = np.stack([edges[1:], np.zeros(n), np.full(n, -hz)], axis=1)
    pos[2::3] = np.stack([0.5 * (edges[:-1] + edges[1:]), np.zeros(n), np.full(n, hz)], axis=1)
    nrm = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (3 * n, 1))
    uv = np.tile(np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]], np.float32), (n, 1))
    return Mesh(pos, nrm, uv, np.arange(3 * n, dtype=np.uint32))


def _seeded_widths(triangles: int, rng, total: float = 0.4):
    """Unequal widths (0.5 .. 1.5 of their mean) adding up to `total`: areas on both sides of the mean."""
    w = rng.uniform(0.5, 1.5, triangles)
    return w * (total / w.sum())


# ------------------------------------------------------------------ transforms
def _rot(axis, angle) -> np.ndarray:
    from hikari_amd.scene import quat_from_axis_angle, quat_to_mat3
    return quat_to_mat3(quat_from_axis_angle(axis, angle))


def _trs(pos, rot3, scale) -> np.ndarray:
    m = np.eye(4)
    m[:3, :3] = rot3 * np.asarray(scale, np.float64)[None, :]
    m[:3, 3] = pos
    return m


def _plain_models(n: int, rng, lo=(-1.2, 0.2, -1.0), hi=(1.2, 1.8, 0.6), scale=(1.0, 2.4)) -> list:
    """n seeded models: positions uniform in the box lo..hi, a rotation of up to a radian about a seeded axis that
    leans the quads towards the camera, a uniform scale."""
    out = []
    for _ in range(n):
        axis = rng.normal(size=3)
        r = _rot([1, 0, 0], 0.5 * math.pi) @ _rot(axis, rng.uniform(-1.0, 1.0))
        out.append(_trs(rng.uniform(lo, hi), r, np.full(3, rng.uniform(*scale))))
    return out


def _square_models(n: int, rng, half: float = 1.6, scale: float = 0.12) -> list:
    """n models uniform in the square |x|, |y - 1| <= half of the plane z = 0, the quads facing the camera."""
    face = _rot([1, 0, 0], 0.5 * math.pi)
    return [_trs([rng.uniform(-half, half), 1.0 + rng.uniform(-half, half), 0.0], face, np.full(3, scale))
            for _ in range(n)]


# ------------------------------------------------------------------ scenes
EMITTER_COLOURS = [(1.0, 0.85, 0.6, 0.3), (0.5, 0.7, 1.0, 0.35), (1.0, 0.4, 0.3, 0.4), (0.6, 1.0, 0.6, 0.3)]


def _pair(models0, models1, emitters=None, quad_half=QUAD_HALF):
    """(scene0, scene1) with the given models (lists of 4 x 4 numpy matrices of one length).  emitters: {instance
    index: a hikari_amd Mesh or a list of triangle widths}; every other instance is the shared quad."""
    from hikari_amd import Scene, StandardMaterial, plane_mesh
    assert len(models0) == len(models1)
    emitters = emitters or {}
    scenes = []
    for models in (models0, models1):
        s = Scene()
        quad = s.add_mesh(plane_mesh(2.0 * quad_half))
        grey = s.add_material(StandardMaterial(base_color=(0.7, 0.65, 0.6, 1.0), perceptual_roughness=0.8))
        lit = [s.add_material(StandardMaterial(base_color=(1.0, 1.0, 1.0, 1.0), emissive=e)) for e in EMITTER_COLOURS]
        meshes = {}
        for k, m in enumerate(models):
            if k in emitters:
                spec = emitters[k]
                key = id(spec)
                if key not in meshes:
                    meshes[key] = s.add_mesh(spec if hasattr(spec, "positions") else _strip_mesh(spec))
                s.add_instance(meshes[key], lit[k % len(lit)], m)
            else:
                s.add_instance(quad, grey, m)
        scenes.append(s)
    return tuple(scenes)


def camera_for(name: str):
    """(camera, lights) of a case's frames: the ladder's camera in front of the box the instances fill; above the
    plane y = 0 for neg_zero, whose instances lie in it."""
    from hikari_amd import Camera, Transform, make_lights
    eye = (0.0, 3.0, 3.0) if name == "neg_zero" else (0.0, 1.0, 4.0)
    at = (0.0, 0.0, 0.0) if name == "neg_zero" else (0.0, 1.0, 0.0)
    return Camera(Transform.from_xyz(*eye).looking_at(at)), make_lights(None)


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


# ---- TLAS sizes
def _tlas(n: int):
    def make(name):
        rng = _rng(name)
        # n = 1 has no emitter (the rebuild's empty-emissive branch); the others one two-triangle emitter
        emitters = {n // 2: [0.2, 0.3]} if n > 1 else {}
        return _pair(_plain_models(n, rng), _plain_models(n, rng), emitters)
    return make


def _big_overflow(name):
    rng = _rng(name)
    n = BIG_OVERFLOW_N
    return _pair(_square_models(n, rng, scale=0.1), _square_models(n, rng, scale=0.1), {n // 2: [0.2, 0.3]})


# ---- light-BVH sizes
def _lights(m: int, n: int):
    def make(name):
        rng = _rng(name)
        where = sorted(rng.choice(n, m, replace=False).tolist())
        strips = [[0.1], [0.1, 0.15], [0.1, 0.05, 0.12]]  # one to three triangles
        emitters = {k: strips[j % 3] for j, k in enumerate(where)}
        return _pair(_plain_models(n, rng), _plain_models(n, rng), emitters)
    return make


# ---- alias sizes (triangles per emitter)
def _alias(widths_of):
    def make(name):
        rng = _rng(name)
        lists = widths_of(rng)
        emitters = {1 + 2 * j: w for j, w in enumerate(lists)}  # instances 1, 3, 5: upload order = list order
        n = 2 * len(lists) + 2
        return _pair(_plain_models(n, rng, scale=(5.0, 9.0)), _plain_models(n, rng, scale=(5.0, 9.0)), emitters)
    return make


def _skewed(rng):
    w = np.full(201, 0.002)
    w[77] = 2.0  # one triangle with 1000 times the area of each of the other 200
    return [w]


def _one_degenerate(rng):
    w = _seeded_widths(21, rng)
    w[9] = 0.0
    return [w]


# ---- coincidence
def _coincident(n: int, clusters: int = 1):
    def make(name):
        rng = _rng(name)
        centres = _plain_models(clusters, rng, scale=(1.0, 2.4) if clusters == 1 else (4.0, 7.0))
        return _pair(_plain_models(n, rng), [centres[k // (n // clusters)] for k in range(n)], {0: [0.2, 0.3]})
    return make


def _equal_spacing(name):
    rng = _rng(name)
    n = 200
    # identical quads of half extent 1 / 8 under pure translations k / 64 on x: every box coordinate, centroid and
    # extent is exact in float32, so mirror-image splits cost exactly the same
    line = []
    for k in range(n):
        m = np.eye(4)
        m[:3, 3] = [(k - n // 2) / 64.0, 1.0, 0.0]
        line.append(m)
    return _pair(_plain_models(n, rng), line, {}, quad_half=0.125)


# ---- transforms: 300 instances, 5 emitters
TRANSFORM_N, TRANSFORM_EMITTERS = 300, (7, 70, 150, 222, 299)
QUARTER_TURNS = [  # rotations by multiples of 90 degrees, written out
    [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
    [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]], [[0, 0, -1], [-1, 0, 0], [0, 1, 0]],
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 0, 1], [0, -1, 0], [1, 0, 0]]]


def _transformed(linear_of):
    """scene1's models: a seeded position and linear_of(rng, k) as the 3 x 3 part of instance k."""
    def make(name):
        rng = _rng(name)
        n = TRANSFORM_N
        m1 = []
        for k in range(n):
            m = np.eye(4)
            m[:3, :3] = linear_of(rng, k)
            m[:3, 3] = rng.uniform((-1.2, 0.2, -1.0), (1.2, 1.8, 0.6))
            m1.append(m)
        widths = [_seeded_widths(3 + 2 * j, rng, 0.3) for j in range(len(TRANSFORM_EMITTERS))]
        return _pair(_plain_models(n, rng), m1, dict(zip(TRANSFORM_EMITTERS, widths)))
    return make


def _mirrored(rng, k):
    s = rng.uniform(0.8, 1.6, 3)
    s[k % 3] *= -1.0
    return _rot([1, 0, 0], 0.5 * math.pi) @ _rot(rng.normal(size=3), rng.uniform(-1.0, 1.0)) * s[None, :]


def _non_uniform(rng, k):
    return _rot([1, 2, 3], rng.uniform(-math.pi, math.pi)) * np.array([0.05, 1.0, 20.0])[None, :]


def _sheared(rng, k):
    sh = np.eye(3)
    sh[0, 1], sh[0, 2], sh[1, 2] = rng.uniform(-1.5, 1.5, 3)
    return _rot(rng.normal(size=3), rng.uniform(-1.0, 1.0)) @ sh


def _quarter(rng, k):
    return np.array(QUARTER_TURNS[k % len(QUARTER_TURNS)], np.float64)


def _neg_zero(name):
    """Flat meshes (half extent 0 on y) under axis-aligned models whose off-diagonal entries and some translation
    components are zeros of seeded sign: the corner sums are zeros of both signs on the flat axis.  The matrices are
    assigned entry by entry, so no arithmetic normalises a sign away."""
    rng = _rng(name)
    n = TRANSFORM_N
    m1 = []
    for k in range(n):
        m = np.zeros((4, 4), np.float64)
        for r in range(3):
            for c in range(3):
                m[r, c] = -0.0 if rng.random() < 0.5 else 0.0
            m[r, r] = rng.uniform(0.8, 1.6) * (-1.0 if rng.random() < 0.5 else 1.0)
        m[0, 3], m[2, 3] = rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5)
        m[1, 3] = -0.0 if k % 2 else 0.0
        if k % 7 == 0:
            m[0, 3] = -0.0
        if k % 11 == 0:
            m[2, 3] = -0.0
        m[3, 3] = 1.0
        m1.append(m)
    widths = [_seeded_widths(3 + 2 * j, rng, 0.3) for j in range(len(TRANSFORM_EMITTERS))]
    return _pair(_plain_models(n, rng), m1, dict(zip(TRANSFORM_EMITTERS, widths)))


def _singular(name):
    rng = _rng(name)
    n = 40
    m1 = _plain_models(n, rng)
    m1[17][:3, 1] = 0.0  # a zero column: determinant exactly 0
    return _pair(_plain_models(n, rng), m1, {3: [0.2, 0.3]})


# ---- depth: scene0 a shallow grid; scene1 the same instances at distances and sizes that grow geometrically along
# one axis, or along +x, -x, +y and -y in turn, so the binned SAH peels one or two off the wide end per split.
# (count, ratio, nearest distance, axes) found by search against the host builder: the TLAS part of the stack
# bound, plus 1 for the quad's two-triangle BLAS
# (need: 16 = every LDS level, 17 = the first scene of the deep walk, 64 = the last it takes, 65 = the first refused)
DEPTH = {"deep_lds_edge": (16, 4.0, 2e-6, 1), "deep_over_lds": (17, 4.0, 2e-6, 1), "deep_at_limit": (129, 4.0, 2e-6, 4),
         "too_deep": (131, 4.0, 2e-6, 4)}
DEPTH_NEED = {"deep_lds_edge": 16, "deep_over_lds": 17, "deep_at_limit": 64, "too_deep": 65}
DEPTH_AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def _deep(name):
    n, ratio, bottom, axes = DEPTH[name]
    face = _rot([1, 0, 0], 0.5 * math.pi)
    cols = int(math.ceil(math.sqrt(n)))
    grid = [_trs([-1.0 + 2.0 * (k % cols) / max(1, cols - 1), 0.3 + 1.4 * (k // cols) / max(1, cols - 1), 0.0], face,
                 np.ones(3)) for k in range(n)]
    # instance k sits at the distance d = bottom * ratio^(k // axes) from (0, 1, 0) along axis k % axes of DEPTH_AXES,
    # its half extent 0.1 d: the centroids stay distinct in float32 near the centre
    line = []
    for k in range(n):
        d = bottom * ratio ** (k // axes)
        line.append(_trs(np.array([0.0, 1.0, 0.0]) + d * np.array(DEPTH_AXES[k % axes], np.float64), face,
                         np.full(3, 1.25 * d)))
    return _pair(grid, line, {})


CASES = {
    # TLAS sizes: 1 (a lone leaf), 2, COOP_MIN and one more, one ballot chunk and one more (the cursor carry),
    # BVH_LDS_SHAPES and one more (k_build_bvh<true> / <false>), a global build of two levels of big segments
    "tlas_1": _tlas(1), "tlas_2": _tlas(2), "tlas_128": _tlas(128), "tlas_129": _tlas(129), "tlas_256": _tlas(256),
    "tlas_257": _tlas(257), "tlas_1280": _tlas(1280), "tlas_1281": _tlas(1281), "tlas_2600": _tlas(2600),
    # more than BIG_MAX segments above COOP_MIN on one tree level
    "big_overflow": _big_overflow,
    # light-BVH sizes (emitters among n instances), and every instance an emitter
    "lights_1": _lights(1, 12), "lights_2": _lights(2, 12), "lights_129": _lights(129, 160),
    "lights_300": _lights(300, 330), "all_emitters": _lights(140, 140),
    # alias sizes
    "alias_1": _alias(lambda rng: [[0.3]]), "alias_64": _alias(lambda rng: [_seeded_widths(64, rng)]),
    "alias_65": _alias(lambda rng: [_seeded_widths(65, rng)]),
    "alias_3072": _alias(lambda rng: [_seeded_widths(3072, rng, 1.2)]),
    "alias_3073": _alias(lambda rng: [_seeded_widths(3073, rng, 1.2)]),
    "two_large": _alias(lambda rng: [_seeded_widths(3073, rng, 1.2), _seeded_widths(3100, rng, 1.2),
                                     _seeded_widths(5, rng)]),
    "skewed": _alias(_skewed), "regular": _alias(lambda rng: [np.full(16, 0.025)]),
    "one_degenerate": _alias(_one_degenerate),
    # coincident centroids
    "coincident_100": _coincident(100), "coincident_300": _coincident(300), "clustered": _coincident(400, 8),
    "equal_spacing": _equal_spacing,
    # transforms
    "mirrored": _transformed(_mirrored), "non_uniform": _transformed(_non_uniform), "sheared": _transformed(_sheared),
    "quarter_turns": _transformed(_quarter),
    "scale_1e-4": _transformed(lambda rng, k: _rot(rng.normal(size=3), rng.uniform(-1.0, 1.0)) * 1e-4),
    "scale_1e4": _transformed(lambda rng, k: _rot(rng.normal(size=3), rng.uniform(-1.0, 1.0)) * 1e4),
    "neg_zero": _neg_zero,
    # depth
    "deep_lds_edge": _deep, "deep_over_lds": _deep, "deep_at_limit": _deep, "too_deep": _deep,
    "singular": _singular,
}

TLAS_SIZES = {f"tlas_{n}": n for n in (1, 2, 128, 129, 256, 257, 1280, 1281, 2600)}
LIGHT_SIZES = {"lights_1": (1, 12), "lights_2": (2, 12), "lights_129": (129, 160), "lights_300": (300, 330),
               "all_emitters": (140, 140)}
ALIAS_SIZES = {"alias_1": [1], "alias_64": [64], "alias_65": [65], "alias_3072": [3072], "alias_3073": [3073],
               "two_large": [3073, 3100, 5], "skewed": [201], "regular": [16], "one_degenerate": [21]}
COINCIDENT = {"coincident_100": 100, "coincident_300": 300}
TRANSFORMS = ["mirrored", "non_uniform", "sheared", "quarter_turns", "scale_1e-4", "scale_1e4", "neg_zero"]
ARRAY_CASES = [n for n in CASES if n not in ("singular", "too_deep")]
SECOND_UPDATE_CASES = ["tlas_257", "tlas_1281", "two_large"]
FRAME_CASES = ["tlas_129", "tlas_1281", "big_overflow", "lights_129", "alias_3073", "clustered", "mirrored", "neg_zero"]
FRAME_SIZE = (32, 24)

_made = {}


def case(name: str):
    """(scene0, scene1) of a case, made once per process; scene0 is built (scene0.desc), scene1 is not: its host
    build is the caller's (it raises for `singular`)."""
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


# ------------------------------------------------------------------ reading a flat bvh 0.7.1 tree
def subtrees(nodes):
    """[(first node, shapes, inner nodes above it)] of every subtree of a flat tree (parity.NODE_DT records), the
    root first.  A subtree of k > 1 shapes starting at node a is the left child's box node a (exit q), the left
    child's subtree from a + 1, the right child's box node q and its subtree from q + 1; the box node at i with exit
    x heads a child of (x - i + 1) / 3 shapes."""
    n = (len(nodes) + 2) // 3
    out, todo = [], [(0, n, 0)]
    entry, exit_ = nodes["entry"], nodes["exit"]
    while todo:
        a, k, d = todo.pop()
        out.append((a, k, d))
        if k == 1:
            assert entry[a] >= 0x80000000
            continue
        q = int(exit_[a])
        assert entry[a] == a + 1 and (q - a + 1) % 3 == 0
        nl = (q - a + 1) // 3
        assert 0 < nl < k and entry[q] == q + 1 and exit_[q] == a + 3 * k - 2
        todo += [(q + 1, k - nl, d + 1), (a + 1, nl, d + 1)]
    return out


def inner_depth(nodes) -> int:
    """The most inner nodes on a root-to-leaf path: the depth of the deepest leaf."""
    return max(d for _, k, d in subtrees(nodes) if k == 1) if len(nodes) else 0


def stack_need(scene) -> int:
    """The G-buffer walk's stack bound of a built scene, read off its flat trees: the TLAS's inner depth plus the
    deepest instanced BLAS's."""
    from parity import NODE_DT, host_scene_array
    d = scene.desc
    blas = host_scene_array(d, 2, NODE_DT)
    inst = np.frombuffer(host_scene_array(d, 4, np.dtype((np.void, 176))).tobytes(), np.uint32).reshape(-1, 44)
    ranges = {(int(a), int(b)) for a, b in inst[:, mesh_node_words()]}
    return inner_depth(host_scene_array(d, 5, NODE_DT)) + max(inner_depth(blas[a: a + b]) for a, b in ranges)


def mesh_node_words():
    """The two words of hk_instance.mesh.node (first node, node count) in a 44-word instance record
    (include/hk_types.h: min, material, max, node_index, model, inverse_transpose_model, mesh)."""
    return [42, 43]
