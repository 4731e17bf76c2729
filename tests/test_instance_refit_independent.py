"""hks_refit_boxes (csrc/hk_scene.cpp over include/hk_refit.h) and Scene.refitted_instances against
tests/refit_boxes_numpy.py, a restatement of the rule written from its text that gathers every entry node's leaves instead
of walking the tree bottom-up: every stored word equal, NaN for NaN, on the case trees and on boxes with signed zeros,
infinities, a NaN component and an all-NaN shape; four misreadings each shown to give other words; the refusals; and what
the boxes mean geometrically, checked without either implementation."""
import numpy as np
import pytest

import instance_refit_cases as ic
import refit_boxes_numpy as rb
from parity import host_scene_array

INST_DT, EM_DT = np.dtype((np.void, 176)), np.dtype((np.void, 64))
TREE_CASES = ["n1_m1", "n2", "tlas_at_32", "tlas_at_35", "lights_at_35", "no_large", "many_large", "over_256", "deep",
              "swapped", "coincident", "neg_zero", "unchanged"]
SPECIAL = ["signed_zeros", "infinities", "nan_component", "all_nan_shape"]


def _arrays(desc) -> dict:
    return {"instances": host_scene_array(desc, 4, INST_DT), "instance_nodes": host_scene_array(desc, 5, rb.NODE_DT),
            "emissives": host_scene_array(desc, 8, EM_DT), "emissive_nodes": host_scene_array(desc, 7, rb.NODE_DT)}


def _host(boxes, nodes, count=None, node_count=None):
    """(return code, nodes after) of hks_refit_boxes on copies."""
    from hikari_amd import _abi
    b = np.ascontiguousarray(boxes, np.float32).copy()
    n = np.ascontiguousarray(nodes).copy()
    rc = _abi.lib().hks_refit_boxes(b.ctypes.data, len(b) if count is None else count, n.ctypes.data,
                                    len(n) if node_count is None else node_count)
    return rc, n


def _lone_leaf_shape(nodes) -> int:
    """The shape of a leaf that is the only node in some entry node's range."""
    for i in range(len(nodes) - 1):
        if nodes["entry"][i] < rb.LEAF and nodes["exit"][i] == i + 2:
            return int(nodes["entry"][i + 1] - rb.LEAF)
    raise AssertionError("no entry node over a lone leaf")


def _f32(word):
    return np.frombuffer(np.uint32(word).tobytes(), np.float32)[0]


def _inputs(label):
    """(boxes, nodes): a case's TLAS of scene0 with scene1's instance boxes, or over_256's with special boxes."""
    if label not in SPECIAL:
        return rb.tlas_shapes(host_scene_array(ic.built1(label), 4, INST_DT)), _arrays(ic.case(label)[0].desc)["instance_nodes"]
    nodes = _arrays(ic.case("over_256")[0].desc)["instance_nodes"]
    boxes = rb.tlas_shapes(host_scene_array(ic.built1("over_256"), 4, INST_DT)).copy()
    rng = np.random.default_rng([ic.SEED, SPECIAL.index(label)])
    if label == "signed_zeros":
        boxes[:, [1, 4]] = np.where(rng.random((len(boxes), 2)) < 0.5, np.float32(-0.0), np.float32(0.0))
    elif label == "infinities":
        boxes[5, 0], boxes[5, 3] = -np.inf, np.inf
        boxes[9, 2] = np.inf       # a min of +inf
        boxes[11, 4] = -np.inf     # a max of -inf
    elif label == "nan_component":
        boxes[7, 1] = np.nan
        boxes[40, 5] = _f32(0xFFC00001)  # a negative quiet NaN with a payload
        boxes[41, 0] = _f32(0x7F800001)  # a signalling one
    elif label == "all_nan_shape":
        boxes[_lone_leaf_shape(nodes)] = np.nan
        boxes[3] = np.nan
    return boxes, nodes


@pytest.mark.parametrize("label", TREE_CASES + SPECIAL)
def test_every_stored_word_equals_the_restatement(label):
    boxes, nodes = _inputs(label)
    rc, got = _host(boxes, nodes)
    assert rc == 0
    want = rb.refit(nodes, boxes)
    bad = np.argwhere(rb.words(got) != rb.words(want))
    assert not len(bad), (label, bad[:5].tolist())
    leaf = nodes["entry"] >= rb.LEAF
    assert got[leaf].tobytes() == nodes[leaf].tobytes()  # every byte of a leaf stays
    assert np.array_equal(got["entry"], nodes["entry"]) and np.array_equal(got["exit"], nodes["exit"])
    if len(nodes) > 1 and label != "unchanged":
        assert got.tobytes() != nodes.tobytes()  # and the refit did something


def test_a_lone_leaf_is_returned_as_it_is():
    boxes, nodes = _inputs("n1_m1")
    assert len(nodes) == 1
    rc, got = _host(np.full((1, 6), 5.0, np.float32), nodes)
    assert rc == 0 and got.tobytes() == nodes.tobytes()


def test_an_all_nan_shape_alone_in_a_range_leaves_the_empty_box():
    boxes, nodes = _inputs("all_nan_shape")
    rc, got = _host(boxes, nodes)
    i = int(np.flatnonzero(nodes["entry"] == rb.LEAF + _lone_leaf_shape(nodes))[0]) - 1
    assert rc == 0 and nodes["exit"][i] == i + 2
    assert (got["min"][i] == np.inf).all() and (got["max"][i] == -np.inf).all()
    assert not np.isnan(got["min"]).any() and not np.isnan(got["max"]).any()


@pytest.mark.parametrize("name", ["n1_m0", "n1_m1", "n2", "lights_at_32", "lights_at_35", "many_large", "neg_zero", "swapped"])
def test_the_refitted_scene_equals_the_restatement(name):
    """Scene.refitted_instances (hks_refit_boxes over the records' boxes) against refit_boxes_numpy.refitted_scene: the
    instance and emissive records, the TLAS and the light BVH, word for word; everything else is scene1's as built."""
    import ctypes
    from parity import SCENE_ARRAYS
    d0, d1 = ic.case(name)[0].desc, ic.built1(name)
    got, want = _arrays(ic.refitted(name)), rb.refitted_scene(_arrays(d0), _arrays(d1))
    for key, w in want.items():
        g = np.frombuffer(got[key].tobytes(), np.uint32)
        assert np.array_equal(g, np.frombuffer(np.ascontiguousarray(w).tobytes(), np.uint32)), key
    for k, size in enumerate((32, 48, 32, 8, 176, 32, 80, 32, 64)):
        a, b = getattr(ic.refitted(name), SCENE_ARRAYS[k]), getattr(d1, SCENE_ARRAYS[k])
        assert a.count == b.count
        if k in (0, 1, 2, 3, 6):
            assert ctypes.string_at(a.data, a.count * size) == ctypes.string_at(b.data, b.count * size)
    # node_index names the kept tree's leaves
    inst = rb.instance_words(got["instances"])
    tlas = got["instance_nodes"]
    assert np.array_equal(tlas["entry"][inst[:, 7]], rb.LEAF + np.arange(len(inst), dtype=np.uint32))
    em = rb.emitter_words(got["emissives"])
    if len(em):
        assert np.array_equal(got["emissive_nodes"]["entry"][em[:, 13]], rb.LEAF + np.arange(len(em), dtype=np.uint32))


@pytest.mark.parametrize("misreading, label", [("closed_range", "coincident"), ("nan_propagates", "nan_component")])
def test_each_misreading_of_the_fold_fails(misreading, label):
    boxes, nodes = _inputs(label)
    rc, got = _host(boxes, nodes)
    assert rc == 0
    assert (rb.words(got) == rb.words(rb.refit(nodes, boxes))).all()
    wrong = rb.refit(nodes, boxes, **{misreading: True})
    assert (rb.words(got) != rb.words(wrong)).any(), misreading


@pytest.mark.parametrize("misreading, key", [("from_instance_box", "emissive_nodes"),
                                             ("node_index_of_scene1", "instances"),
                                             ("node_index_of_scene1", "emissives")])
def test_each_misreading_of_the_scene_fails(misreading, key):
    """The emitter box taken from the instance's box instead of the sphere's; node_index taken from the rebuilt scene."""
    name = "lights_at_35"
    d0, d1 = ic.case(name)[0].desc, ic.built1(name)
    got = _arrays(ic.refitted(name))
    right = rb.refitted_scene(_arrays(d0), _arrays(d1))
    wrong = rb.refitted_scene(_arrays(d0), _arrays(d1), **{misreading: True})
    as_words = lambda a: np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint32)
    assert np.array_equal(as_words(got[key]), as_words(right[key]))
    assert not np.array_equal(as_words(got[key]), as_words(wrong[key]))


def test_the_emitter_box_is_the_builds():
    """S[e] from the emissive record is the box the host build hands its light BVH: with one emitter pair the root's two
    entry nodes carry exactly their leaf's box, in the built tree as in the refit one."""
    name = "n2"  # one emitter only: use a two-emitter tree
    d = ic.built1("no_large")
    lbvh, em = host_scene_array(d, 7, rb.NODE_DT), host_scene_array(d, 8, EM_DT)
    shapes = rb.light_shapes(em)
    for i in np.flatnonzero((lbvh["entry"] < rb.LEAF) & (lbvh["exit"] == np.arange(len(lbvh)) + 2)):
        e = int(lbvh["entry"][i + 1] - rb.LEAF)
        assert np.array_equal(lbvh["min"][i], shapes[e, 0:3]) and np.array_equal(lbvh["max"][i], shapes[e, 3:6])


def _malformed(nodes):
    """[(label, nodes)]: each kind of tree that is not a well-formed flatten."""
    n = len(nodes)
    leaf = np.flatnonzero(nodes["entry"] >= rb.LEAF)
    inner = np.flatnonzero(nodes["entry"] < rb.LEAF)
    deep = next(int(i) for i in inner if nodes["entry"][i + 1] < rb.LEAF)  # an entry node over two entry nodes
    out = []

    def add(label, i, field, value):
        m = nodes.copy()
        m[field][i] = value
        out.append((label, m))

    add("a leaf whose exit is not i + 1", leaf[3], "exit", leaf[3] + 2)
    add("a leaf payload not below count", leaf[3], "entry", rb.LEAF + (n + 2) // 3)
    add("a shape in two leaves", leaf[3], "entry", nodes["entry"][leaf[4]])
    add("an entry node whose entry is not i + 1", inner[2], "entry", inner[2] + 2)
    add("an entry node whose exit is not past i + 1", inner[2], "exit", inner[2] + 1)
    add("an entry node whose exit is i", inner[2], "exit", inner[2])
    add("an entry node whose exit is past the tree", inner[0], "exit", n + 1)
    add("a root whose children do not tile the tree", 0, "exit", n)
    add("a range one node short of its second child's end", deep, "exit", nodes["exit"][deep] - 1)
    add("a range that ends inside its first child", deep, "exit", nodes["exit"][deep + 1])
    add("a first child that runs into the second", deep + 1, "exit", nodes["exit"][deep + 1] + 1)
    add("a leaf where the second entry node belongs", int(nodes["exit"][deep + 1]), "entry", nodes["entry"][leaf[0]])
    return out


def test_refusals_leave_the_nodes_untouched():
    import hikari_amd
    from hikari_amd import _abi
    L = _abi.lib()
    boxes, nodes = _inputs("over_256")
    boxes = np.ascontiguousarray(boxes)
    k, n = len(boxes), len(nodes)
    assert L.hks_refit_boxes(None, k, nodes.ctypes.data, n) == _abi.HK_ERR_INVALID
    assert L.hks_refit_boxes(boxes.ctypes.data, k, None, n) == _abi.HK_ERR_INVALID
    for count, ncount in ((k, n - 1), (k - 1, n), (k, n + 1), (0, 0), (0, n), (k, 0)):
        rc, after = _host(boxes, nodes, count, ncount)
        assert rc == _abi.HK_ERR_INVALID and after.tobytes() == nodes.tobytes(), (count, ncount)
    kinds = _malformed(nodes)
    assert len(kinds) >= 10
    for label, bad in kinds:
        rc, after = _host(boxes, bad)
        assert rc == _abi.HK_ERR_INVALID, label
        assert after.tobytes() == bad.tobytes(), label
    rc, after = _host(boxes, nodes)  # and the tree they were made from is taken
    assert rc == 0 and after.tobytes() != nodes.tobytes()
    with pytest.raises(_abi.HikariError):
        hikari_amd.refit_boxes(boxes, kinds[0][1])


def test_python_refit_boxes_returns_a_copy():
    import hikari_amd
    boxes, nodes = _inputs("tlas_at_35")
    before = nodes.tobytes()
    out = hikari_amd.refit_boxes(boxes, nodes)
    assert nodes.tobytes() == before
    assert out.tobytes() == _host(boxes, nodes)[1].tobytes()


@pytest.mark.parametrize("label", ["over_256", "deep", "infinities", "nan_component", "signed_zeros"])
def test_boxes_contain_their_subtrees_and_every_bound_is_attained(label):
    """Independent of both implementations: every entry box contains every non-NaN bound of the shapes stored in its
    range, and every finite bound equals some shape's."""
    boxes, nodes = _inputs(label)
    rc, got = _host(boxes, nodes)
    assert rc == 0
    checked = 0
    for i in np.flatnonzero(nodes["entry"] < rb.LEAF):
        inside = np.arange(i + 1, int(nodes["exit"][i]))
        t = nodes["entry"][inside]
        s = boxes[(t[t >= rb.LEAF] - rb.LEAF).astype(np.int64)]
        for c in range(3):
            lo_v, hi_v = s[:, c][~np.isnan(s[:, c])], s[:, 3 + c][~np.isnan(s[:, 3 + c])]
            lo, hi = got["min"][i][c], got["max"][i][c]
            assert (lo_v >= lo).all() and (hi_v <= hi).all()
            if np.isfinite(lo):
                assert (lo_v == lo).any()
            if np.isfinite(hi):
                assert (hi_v == hi).any()
            checked += 1
    assert checked == 3 * (len(nodes) - len(boxes))
