"""hks_refit_nodes (csrc/hk_scene.cpp over include/hk_refit.h) against tests/refit_numpy.py, a restatement of the rule
written from its text that gathers every entry node's leaves instead of walking the tree bottom-up: every stored word
equal on deformed grids, coincident, degenerate and signed-zero meshes, a NaN corner, a mesh collapsed to a point and one
scaled by 1e30; four misreadings of the rule each shown to give other words; a refit over unchanged vertices; the
refusals; and what the boxes mean geometrically, checked without either implementation."""
import ctypes

import numpy as np
import pytest

import mesh_cases as mc
import refit_numpy as rn
from parity import host_scene_array

PRIM_DT = np.dtype((np.void, 48))
MESH_CASES = ["tris_1", "tris_2", "tris_129", "tris_257", "coincident_100", "degenerate", "neg_zero", "strip",
              "shared_mesh"]


def _slices(name, which):
    """(primitives, nodes) of the case's listed mesh in scene `which`: 48-byte records and refit_numpy.NODE_DT."""
    scene0, scene1 = mc.case(name)
    desc = scene0.desc if not which else scene1.desc if scene1.desc is not None else scene1.build()
    _, p0, n0, nc = scene0.mesh_index(mc.listed(name)[0])
    prims = host_scene_array(desc, 1, PRIM_DT)[p0: p0 + (nc + 2) // 3].copy()
    nodes = host_scene_array(desc, 2, rn.NODE_DT)[n0: n0 + nc].copy()
    return prims, nodes


def _with_corners(prims, corners):
    """The primitives with other corner positions (k, 3, 3); the vertex indices stay."""
    w = np.frombuffer(prims.tobytes(), np.float32).reshape(-1, 3, 4).copy()
    w[:, :, :3] = corners
    return np.frombuffer(w.tobytes(), PRIM_DT).copy()


def _host(prims, nodes, primitive_count=None, node_count=None):
    """(return code, nodes after) of hks_refit_nodes on copies."""
    from hikari_amd import _abi
    p, n = np.ascontiguousarray(prims).copy(), np.ascontiguousarray(nodes).copy()
    rc = _abi.lib().hks_refit_nodes(p.ctypes.data, len(p) if primitive_count is None else primitive_count,
                                    n.ctypes.data, len(n) if node_count is None else node_count)
    return rc, n


def _special(kind):
    """tris_129's tree with scene1's primitives changed: (primitives, nodes)."""
    prims, nodes = _slices("tris_129", 1)
    _, nodes = _slices("tris_129", 0)
    c = rn.corners_of(prims)
    if kind == "nan_corner":
        c[5, 1] = np.nan                                      # one whole corner
        c[40, 0, 2] = np.float32(np.nan)                      # one component of one corner
        lone = _parent_of_leaf(nodes)
        c[lone, :, 0] = np.nan                                # every x of a primitive that is alone in a range
    elif kind == "one_point":
        c[:] = np.array([0.25, -1.5, 3.0], np.float32)
    elif kind == "scaled_1e30":
        c *= np.float32(1e30)
    elif kind == "signed_nan":
        c[7, 2] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), np.float32)[0]  # a negative quiet NaN with a payload
        c[8, 0, 1] = np.frombuffer(np.uint32(0x7F800001).tobytes(), np.float32)[0]  # a signalling one
    return _with_corners(prims, c), nodes


def _parent_of_leaf(nodes) -> int:
    """The primitive of a leaf that is the only node in some entry node's range."""
    for i in range(len(nodes) - 1):
        if nodes["entry"][i] < rn.LEAF and nodes["exit"][i] == i + 2:
            return int(nodes["entry"][i + 1] - rn.LEAF)
    raise AssertionError("no entry node over a lone leaf")


SPECIAL = ["nan_corner", "one_point", "scaled_1e30", "signed_nan"]


def _inputs(label):
    if label in SPECIAL:
        return _special(label)
    prims, _ = _slices(label, 1)
    _, nodes = _slices(label, 0)
    return prims, nodes


@pytest.mark.parametrize("label", MESH_CASES + SPECIAL)
def test_every_stored_word_equals_the_restatement(label):
    """scene0's tree refit over scene1's primitives: the 8 words of every node, NaN for NaN, -0 for -0."""
    prims, nodes = _inputs(label)
    rc, got = _host(prims, nodes)
    assert rc == 0
    want = rn.refit(nodes, rn.corners_of(prims))
    bad = np.argwhere(rn.words(got) != rn.words(want))
    assert not len(bad), (label, bad[:5].tolist())
    leaf = nodes["entry"] >= rn.LEAF
    assert got[leaf].tobytes() == nodes[leaf].tobytes()  # every byte of a leaf stays
    assert np.array_equal(got["entry"], nodes["entry"]) and np.array_equal(got["exit"], nodes["exit"])
    if len(nodes) > 1:
        assert got.tobytes() != nodes.tobytes()  # and the refit did something


def test_a_component_whose_corners_are_all_nan_stays_empty():
    prims, nodes = _special("nan_corner")
    rc, got = _host(prims, nodes)
    lone = _parent_of_leaf(nodes)
    i = int(np.flatnonzero(nodes["entry"] == rn.LEAF + lone)[0]) - 1
    assert rc == 0 and nodes["exit"][i] == i + 2
    assert got["min"][i][0] == np.inf and got["max"][i][0] == -np.inf
    assert np.isfinite(got["min"][i][1:]).all() and np.isfinite(got["max"][i][1:]).all()
    assert not np.isnan(got["min"]).any() and not np.isnan(got["max"]).any()


@pytest.mark.parametrize("misreading, label", [("closed_range", "one_point"), ("positional", "neg_zero"),
                                               ("nan_propagates", "nan_corner"), ("host_leaf_boxes", "tris_129")])
def test_each_misreading_of_the_rule_fails(misreading, label):
    """The restatement with one misreading switched on differs from hks_refit_nodes in some word (and without it, not)."""
    prims, nodes = _inputs(label)
    rc, got = _host(prims, nodes)
    assert rc == 0
    corners = rn.corners_of(prims)
    assert (rn.words(got) == rn.words(rn.refit(nodes, corners))).all()
    wrong = rn.refit(nodes, corners, **{misreading: True})
    assert (rn.words(got) != rn.words(wrong)).any(), misreading


@pytest.mark.parametrize("label", ["tris_2", "tris_129", "neg_zero", "coincident_100", "strip"])
@pytest.mark.parametrize("which", [0, 1])
def test_a_refit_over_unchanged_vertices_gives_the_built_boxes(label, which):
    """Entry and exit words identical, every box equal as floats; only the sign of a zero bound may differ."""
    prims, nodes = _slices(label, which)
    rc, got = _host(prims, nodes)
    assert rc == 0
    assert np.array_equal(got["entry"], nodes["entry"]) and np.array_equal(got["exit"], nodes["exit"])
    assert np.array_equal(got["min"], nodes["min"]) and np.array_equal(got["max"], nodes["max"])
    differ = rn.words(got) != rn.words(nodes)
    assert ((rn.words(got)[differ] | 0x80000000) == 0x80000000).all()  # a word that differs is a zero of either sign


def _malformed(nodes):
    """[(label, nodes)]: each kind of slice that is not a well-formed flatten."""
    n = len(nodes)
    leaf = np.flatnonzero(nodes["entry"] >= rn.LEAF)
    inner = np.flatnonzero(nodes["entry"] < rn.LEAF)
    deep = next(int(i) for i in inner if nodes["entry"][i + 1] < rn.LEAF)  # an entry node over two entry nodes
    out = []

    def add(label, i, field, value):
        m = nodes.copy()
        m[field][i] = value
        out.append((label, m))

    add("a leaf whose exit is not i + 1", leaf[3], "exit", leaf[3] + 2)
    add("a leaf payload not below primitive_count", leaf[3], "entry", rn.LEAF + (n + 2) // 3)
    add("a primitive in two leaves", leaf[3], "entry", nodes["entry"][leaf[4]])
    add("an entry node whose entry is not i + 1", inner[2], "entry", inner[2] + 2)
    add("an entry node whose exit is not past i + 1", inner[2], "exit", inner[2] + 1)
    add("an entry node whose exit is i", inner[2], "exit", inner[2])
    add("an entry node whose exit is past the slice", inner[0], "exit", n + 1)
    add("a root whose children do not tile the slice", 0, "exit", n)
    add("a range one node short of its second child's end", deep, "exit", nodes["exit"][deep] - 1)
    add("a range that ends inside its first child", deep, "exit", nodes["exit"][deep + 1])
    add("a first child that runs into the second", deep + 1, "exit", nodes["exit"][deep + 1] + 1)
    add("a leaf where the second entry node belongs", int(nodes["exit"][deep + 1]), "entry", nodes["entry"][leaf[0]])
    return out


def test_refusals_leave_the_nodes_untouched():
    from hikari_amd import _abi
    L = _abi.lib()
    prims, _ = _slices("tris_129", 1)
    _, nodes = _slices("tris_129", 0)
    k, n = len(prims), len(nodes)
    assert L.hks_refit_nodes(None, k, nodes.ctypes.data, n) == _abi.HK_ERR_INVALID
    assert L.hks_refit_nodes(prims.ctypes.data, k, None, n) == _abi.HK_ERR_INVALID
    for pc, ncount in ((k, n - 1), (k - 1, n), (k, n + 1), (0, 0), (0, n), (k, 0)):
        rc, after = _host(prims, nodes, pc, ncount)
        assert rc == _abi.HK_ERR_INVALID and after.tobytes() == nodes.tobytes(), (pc, ncount)
    kinds = _malformed(nodes)
    assert len(kinds) >= 10
    for label, bad in kinds:
        rc, after = _host(prims, bad)
        assert rc == _abi.HK_ERR_INVALID, label
        assert after.tobytes() == bad.tobytes(), label
    rc, after = _host(prims, nodes)  # and the slice they were made from is taken
    assert rc == 0 and after.tobytes() != nodes.tobytes()
    with pytest.raises(_abi.HikariError):
        import hikari_amd
        hikari_amd.refit_nodes(prims, kinds[0][1])


def test_python_refit_nodes_returns_a_copy():
    import hikari_amd
    prims, nodes = _inputs("tris_257")
    before = nodes.tobytes()
    out = hikari_amd.refit_nodes(prims, nodes)
    assert nodes.tobytes() == before
    assert out.tobytes() == _host(prims, nodes)[1].tobytes()


@pytest.mark.parametrize("label", ["tris_129", "tris_257", "degenerate", "nan_corner", "scaled_1e30", "one_point"])
def test_boxes_contain_their_subtrees_and_every_bound_is_attained(label):
    """Independent of both implementations: every entry box contains every non-NaN corner of the primitives stored in
    its range, and every finite bound equals some corner's component."""
    prims, nodes = _inputs(label)
    rc, got = _host(prims, nodes)
    assert rc == 0
    corners = rn.corners_of(prims)
    checked = 0
    for i in np.flatnonzero(nodes["entry"] < rn.LEAF):
        inside = np.arange(i + 1, int(nodes["exit"][i]))
        t = nodes["entry"][inside]
        pts = corners[(t[t >= rn.LEAF] - rn.LEAF).astype(np.int64)].reshape(-1, 3)
        for c in range(3):
            v = pts[:, c][~np.isnan(pts[:, c])]
            lo, hi = got["min"][i][c], got["max"][i][c]
            assert (v >= lo).all() and (v <= hi).all()
            if np.isfinite(lo):
                assert (v == lo).any()
            if np.isfinite(hi):
                assert (v == hi).any()
            if len(v):
                assert np.isfinite(lo) == np.isfinite(v.min()) and np.isfinite(hi) == np.isfinite(v.max())
            checked += 1
    assert checked == 3 * (len(nodes) - len(prims))


def test_refitted_desc_takes_nodes_from_desc0_and_the_rest_from_scene1():
    """Scene.refitted: arrays 0, 1, 3..8 are scene1's as built; array 2 is desc0's with the listed slices refit and the
    others byte for byte desc0's."""
    from hikari_amd import Scene
    from parity import SCENE_ARRAYS
    name = "one_of_three"
    scene0, scene1 = mc.case(name)
    d1 = scene1.desc if scene1.desc is not None else scene1.build()
    d = Scene.refitted(scene0.desc, scene1, mc.listed(name))
    sizes = (32, 48, 32, 8, 176, 32, 80, 32, 64)
    for k, size in enumerate(sizes):
        a, b = getattr(d, SCENE_ARRAYS[k]), getattr(d1, SCENE_ARRAYS[k])
        assert a.count == b.count
        if k != 2:
            assert ctypes.string_at(a.data, a.count * size) == ctypes.string_at(b.data, b.count * size)
    got, old = host_scene_array(d, 2, rn.NODE_DT), host_scene_array(scene0.desc, 2, rn.NODE_DT)
    prims = host_scene_array(d1, 1, PRIM_DT)
    for i in range(len(scene0.meshes)):
        _, p0, n0, nc = scene1.mesh_index(i)
        if i in mc.listed(name):
            want = _host(prims[p0: p0 + (nc + 2) // 3], old[n0: n0 + nc])[1]
            assert got[n0: n0 + nc].tobytes() == want.tobytes() != old[n0: n0 + nc].tobytes()
        else:
            assert got[n0: n0 + nc].tobytes() == old[n0: n0 + nc].tobytes()
