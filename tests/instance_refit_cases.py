"""Cases for the instance refit (hk_refit_instances, csrc/hk_dynamic.hip k_refit_trees_small / k_refit_trees_large), shared
by tests/test_instance_refit_cases.py (CPU: the host builder alone proves that every case sits on the edge its name says)
and tests/test_gpu_instance_refit.py (GPU: the arrays after the call byte for byte Scene.refitted_instances(...), frames
against the oracle).

A case is a pair (scene0, scene1) in the style of tests/dynamic_cases.py, whose meshes, transforms and pair builder it
uses: scene0 is what is uploaded, and its TLAS and light BVH are the trees the refit KEEPS; scene1 has the same meshes,
materials and instance order with new models.  The non-emissive instances share one flat quad, the emitters are strips
of one to three triangles.  Everything is seeded.

The limit the sizes straddle is REFIT_SMALL = 32 in hk_dynamic.hip: an entry node whose range exit - i is at most 32 is
refit by its own thread, a wider one by a workgroup.  A subtree of p shapes spans 3p - 1 nodes, so the range sizes that
exist either side of the threshold are 32 (p = 11) and 35 (p = 12).  The widest range below the root belongs to the
larger child of the root; the counts below were found by search against the host builder (widest_range proves them).
"""
from __future__ import annotations

import math

import numpy as np

import dynamic_cases as dc

SEED = 0x49524654  # "IRFT"
REFIT_SMALL = 32
FRAME_SIZE = (64, 48)


def _rng(name: str):
    return np.random.default_rng([SEED, list(CASES).index(name)])


def _strips(m: int, n: int, rng) -> dict:
    """m emitters among n instances at seeded places, strips of one to three triangles."""
    where = sorted(rng.choice(n, m, replace=False).tolist())
    strips = [[0.1], [0.1, 0.15], [0.1, 0.05, 0.12]]
    return {k: strips[j % 3] for j, k in enumerate(where)}


def _nudged(models, rng, amount=0.05):
    """The models moved by up to `amount` on each axis and turned by up to 0.2 rad about y."""
    out = []
    for m in models:
        t = np.eye(4)
        t[:3, :3] = dc._rot([0, 1, 0], rng.uniform(-0.2, 0.2))
        t[:3, 3] = rng.uniform(-amount, amount, 3)
        out.append(t @ m)
    return out


def _plain(n: int, m: int, moved="fresh"):
    """n instances, m of them emitters.  scene1: `fresh` seeded models (far from scene0's), `nudged` ones, `same`."""
    def make(name):
        rng = _rng(name)
        m0 = dc._plain_models(n, rng)
        emitters = _strips(m, n, rng) if m else {}
        m1 = {"fresh": lambda: dc._plain_models(n, rng), "nudged": lambda: _nudged(m0, rng),
              "same": lambda: [x.copy() for x in m0], "swapped": lambda: m0[::-1],
              "coincident": lambda: [m0[0].copy() for _ in m0]}[moved]()
        return dc._pair(m0, m1, emitters)
    return make


def _neg_zero(name):
    """dynamic_cases' neg_zero pair (300 instances, 5 emitters): scene1's boxes have zeros of both signs on the flat axis,
    so entry-node bounds are zeros whose sign the unordered fold decides (-0 < +0)."""
    return dc.CASES["neg_zero"]("neg_zero")


def _deep(name):
    """scene0 is dynamic_cases' chain at the G-buffer stack's deepest level (deep_at_limit: the TLAS part 63, one more
    for the quad's BLAS), so the kept tree is the chain: every level an entry node over everything below it.  scene1
    moves the same instances onto a shallow grid, which a rebuild would give a shallow tree."""
    grid, line = dc.CASES["deep_at_limit"]("deep_at_limit")
    models = lambda s: [np.array(m, np.float64) for _, _, m in s.instances]
    return dc._pair(models(line), models(grid), {})


CASES = {
    # the edge sizes: a lone leaf with no light BVH and with a lone-leaf light BVH; one entry node pair
    "n1_m0": _plain(1, 0), "n1_m1": _plain(1, 1), "n2": _plain(2, 1),
    # the TLAS's widest range below the root exactly REFIT_SMALL (no large node) and the next size that exists
    "tlas_at_32": _plain(16, 1), "tlas_at_35": _plain(15, 1),
    # the same of the light BVH, the TLAS above it having large nodes anyway
    "lights_at_32": _plain(40, 20), "lights_at_35": _plain(40, 22),
    # no node reaches the large tier (nothing is listed, k_refit_trees_large is not launched) / hundreds do
    "no_large": _plain(11, 3), "many_large": _plain(2000, 120),
    # above one ballot chunk and above BVH_LDS_SHAPES: a refit that follows a device build of each kind
    "over_256": _plain(300, 5), "over_lds": _plain(1300, 9),
    "deep": _deep,
    "swapped": _plain(200, 7, "swapped"), "coincident": _plain(120, 4, "coincident"),
    "neg_zero": _neg_zero, "unchanged": _plain(150, 6, "same"),
    # a small moving scene for the frames: previous models and motion vectors
    "moving": _plain(40, 4, "nudged"),
}

COUNTS = {"n1_m0": (1, 0), "n1_m1": (1, 1), "n2": (2, 1), "tlas_at_32": (16, 1), "tlas_at_35": (15, 1),
          "lights_at_32": (40, 20), "lights_at_35": (40, 22), "no_large": (11, 3), "many_large": (2000, 120),
          "over_256": (300, 5), "over_lds": (1300, 9), "deep": (129, 0), "swapped": (200, 7), "coincident": (120, 4),
          "neg_zero": (300, 5), "unchanged": (150, 6), "moving": (40, 4)}
ARRAY_CASES = list(CASES)
REPEAT_CASES = ["n1_m1", "tlas_at_35", "many_large"]
BUILD_CASES = ["over_256", "over_lds"]
FRAME_CASES = ["moving", "lights_at_35", "swapped"]
VARIANT_CASE = "moving"

_made, _built1, _refitted = {}, {}, {}


def case(name: str):
    """(scene0, scene1) of a case, made once per process; scene0 is built."""
    if name not in _made:
        scene0, scene1 = CASES[name](name)
        scene0.build()
        _made[name] = (scene0, scene1)
    return _made[name]


def built1(name: str):
    """scene1's host-built desc, once per process."""
    if name not in _built1:
        _built1[name] = case(name)[1].build()
    return _built1[name]


def refitted(name: str):
    """The expected scene after hk_refit_instances on scene0 with scene1's models, once per process."""
    if name not in _refitted:
        from hikari_amd import Scene
        built1(name)
        _refitted[name] = Scene.refitted_instances(case(name)[0].desc, case(name)[1])
    return _refitted[name]


def camera_for(name: str):
    return dc.camera_for(name)


# ------------------------------------------------------------------ reading a flat tree
def ranges(nodes) -> np.ndarray:
    """exit - i of every entry node of a flat tree (parity.NODE_DT records)."""
    inner = np.flatnonzero(nodes["entry"] < 0x80000000)
    return nodes["exit"][inner].astype(np.int64) - inner


def widest_range(nodes) -> int:
    r = ranges(nodes)
    return int(r.max()) if len(r) else 0


def large_nodes(nodes) -> int:
    return int((ranges(nodes) > REFIT_SMALL).sum())
