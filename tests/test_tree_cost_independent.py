"""hks_tree_cost (csrc/hk_scene.cpp over include/hk_cost.h) against tests/tree_cost_numpy.py, a restatement of the rule
written from its text that weighs all entry nodes at once: every field equal, R bit for bit, on every tree of the
instance refit cases and every mesh slice of the BLAS refit cases in three states (uploaded, rebuilt, refitted), and on
hand-made trees at the rule's numeric edges; five misreadings each shown to give another result; the refusals."""
import numpy as np
import pytest

import instance_refit_cases as ic
import refit_cases as rc
import tree_cost_numpy as tc
from parity import host_scene_array

INST_DT = np.dtype((np.void, 176))
F = np.float32


def _host(nodes, count=None):
    """(return code, TreeCost or None) of hks_tree_cost."""
    from hikari_amd import TreeCost, _abi
    n = np.ascontiguousarray(nodes).copy()
    out = _abi.hk_tree_cost(1, 2, 3.0, 4)
    code = _abi.lib().hks_tree_cost(n.ctypes.data if len(n) else None, len(n) if count is None else count, out)
    return code, TreeCost.from_c(out)


def _assert_same(nodes, label):
    code, got = _host(nodes)
    want = tc.tree_cost(nodes)
    assert code == 0 and tc.same(got, want), (label, got, want)
    return got


def _states(module, name):
    return {"uploaded": module.case(name)[0].desc, "rebuilt": module.built1(name), "refitted": module.refitted(name)}


def mesh_slices(desc):
    return tc.known_slices(host_scene_array(desc, 4, INST_DT))


# ------------------------------------------------------------------ the case trees
@pytest.mark.parametrize("name", ic.ARRAY_CASES)
def test_instance_trees_equal_the_restatement(name):
    for state, desc in _states(ic, name).items():
        for array in (5, 7):
            got = _assert_same(host_scene_array(desc, array, tc.NODE_DT), (name, state, array))
            count = ic.COUNTS[name][0 if array == 5 else 1]
            assert got.entries == max(2 * count - 2, 0)
            if count >= 2:
                assert got.root_half_area > 0 and got.leaf > 0


@pytest.mark.parametrize("name", rc.ARRAY_CASES)
def test_mesh_slices_equal_the_restatement(name):
    total = 0
    for state, desc in _states(rc, name).items():
        nodes = host_scene_array(desc, 2, tc.NODE_DT)
        for offset, length in mesh_slices(desc):
            got = _assert_same(nodes[offset:offset + length], (name, state, offset))
            assert got.entries == 2 * ((length + 2) // 3) - 2
            total += got.entries
    assert total > 0 or name == "tris_1"


# ------------------------------------------------------------------ numeric edges
def _boxes(k, seed, scale=1.0):
    rng = np.random.default_rng([0x54434F53, seed])  # "TCOS"
    lo = rng.uniform(-4.0, 4.0, (k, 3))
    return (np.concatenate([lo, lo + rng.uniform(0.05, 1.5, (k, 3))], axis=1) * scale).astype(F)


def _edge(label):
    if label == "lone_leaf":
        return tc.flat_tree(_boxes(1, 0))
    if label == "coplanar_pair":  # the two triangles of one flat quad: both entries ARE the root, r == 1
        return tc.flat_tree(np.array([[0, 0, 0, 1, 1, 0]] * 2, F))
    if label == "one_point":      # R == 0: every r is 0 / 0
        return tc.flat_tree(np.tile(np.array([[0.25, -1.5, 3.0] * 2], F), (9, 1)))
    if label == "huge":           # H overflows: inf / inf
        return tc.flat_tree(_boxes(12, 1, 1e30))
    if label == "huge_root_only":  # R is inf under finite H: every r is 0
        b = _boxes(12, 2)
        b[11, 3:] = 3e30
        return tc.flat_tree(b)
    if label == "denormal":       # H and R denormal, r normal
        return tc.flat_tree(_boxes(12, 3, 2e-21))
    nodes = tc.flat_tree(_boxes(12, 4))
    entry = np.flatnonzero(nodes["entry"] < tc.LEAF)
    if label == "nan_bound":      # one bound of a deep node, and one of a top entry: the root skips it
        nodes["max"][entry[3]][1] = np.nan
        nodes["min"][0][2] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), F)[0]
    elif label == "all_nan_box":  # a whole box NaN, and the other top entry too: that root component is +inf / -inf
        nodes["min"][entry[5]] = np.nan
        nodes["max"][entry[5]] = np.nan
        nodes["min"][int(nodes["exit"][0])][0] = np.nan
        nodes["min"][0][0] = np.nan
    elif label == "signed_zeros":
        flat = _boxes(12, 5)
        flat[:, 1], flat[:, 4] = F(-0.0), F(0.0)
        flat[::2, 4] = F(-0.0)
        flat[::3, 1] = F(0.0)
        nodes = tc.flat_tree(flat)
    return nodes


EDGES = ["lone_leaf", "coplanar_pair", "one_point", "huge", "huge_root_only", "denormal", "nan_bound", "all_nan_box",
         "signed_zeros"]


@pytest.mark.parametrize("label", EDGES)
def test_numeric_edges_equal_the_restatement(label):
    _assert_same(_edge(label), label)


def test_the_edges_are_the_edges_their_names_say():
    from hikari_amd import TreeCost
    assert _host(_edge("lone_leaf"))[1] == TreeCost(0, 0, 0.0, 0)
    assert _host(np.zeros(0, tc.NODE_DT))[1] == TreeCost(0, 0, 0.0, 0)
    assert _host(_edge("coplanar_pair"))[1] == TreeCost(0, 2 << 32, 1.0, 2)  # the 2^32 branch, twice
    point = _host(_edge("one_point"))[1]
    assert (point.inner, point.leaf, point.root_half_area, point.entries) == (0, 0, 0.0, 16)
    huge = _host(_edge("huge"))[1]
    assert np.isinf(huge.root_half_area) and huge.inner == 0 and huge.entries == 22
    assert _host(_edge("huge_root_only"))[1].leaf == 0
    small = _host(_edge("denormal"))[1]
    assert 0 < small.root_half_area < np.finfo(F).tiny and small.inner > 0 and small.leaf > 0
    plain, with_nan = _host(tc.flat_tree(_boxes(12, 4)))[1], _host(_edge("nan_bound"))[1]
    assert with_nan.entries == plain.entries and with_nan.inner + with_nan.leaf < plain.inner + plain.leaf
    assert np.isinf(_host(_edge("all_nan_box"))[1].root_half_area)
    zeros = _host(_edge("signed_zeros"))[1]
    assert zeros.root_half_area > 0 and zeros.leaf > 0


def test_a_zero_bounds_sign_does_not_reach_the_arithmetic():
    nodes = _edge("signed_zeros")
    other = nodes.copy()
    for field in ("min", "max"):
        w = other[field].view(np.uint32)
        w[(w & 0x7FFFFFFF) == 0] ^= 0x80000000
    assert other.tobytes() != nodes.tobytes()
    assert _host(other)[1] == _host(nodes)[1]


def test_leaf_boxes_are_not_read():
    nodes = host_scene_array(ic.case("over_256")[0].desc, 5, tc.NODE_DT).copy()
    want = _host(nodes)[1]
    leaf = nodes["entry"] >= tc.LEAF
    nodes["min"][leaf], nodes["max"][leaf] = np.nan, 7.0
    assert _host(nodes)[1] == want


# ------------------------------------------------------------------ misreadings
MISREADINGS = {"node0_only": "many_large", "volume": "over_256", "round_nearest": "many_large",
               "right_to_left": "many_large", "leaf_entries_into_inner": "n2"}


@pytest.mark.parametrize("misreading", MISREADINGS)
def test_each_misreading_gives_another_result(misreading):
    nodes = host_scene_array(ic.refitted(MISREADINGS[misreading]), 5, tc.NODE_DT)
    code, got = _host(nodes)
    assert code == 0 and tc.same(got, tc.tree_cost(nodes))
    assert not tc.same(got, tc.tree_cost(nodes, **{misreading: True})), misreading


# ------------------------------------------------------------------ refusals
def _refused(nodes, count=None):
    code, out = _host(nodes, count)
    from hikari_amd import TreeCost, _abi
    return code == _abi.HK_ERR_INVALID and out == TreeCost(1, 2, 3.0, 4)  # and `out` was left alone


def test_malformed_slices_are_refused_as_by_the_refit():
    """Every malformed flatten hks_refit_boxes refuses (tests/test_instance_refit_independent.py), with `out` untouched."""
    from hikari_amd import _abi
    good = host_scene_array(ic.case("no_large")[0].desc, 5, tc.NODE_DT)
    assert _host(good)[0] == 0
    assert _abi.lib().hks_tree_cost(good.ctypes.data, len(good), None) == _abi.HK_ERR_INVALID
    assert _abi.lib().hks_tree_cost(None, len(good), _abi.hk_tree_cost()) == _abi.HK_ERR_INVALID
    for count in (len(good) - 1, len(good) - 2, len(good) - 3, 2, 3):
        assert _refused(good, count), count  # not 3k - 2, or a prefix that is no tree
    inner = np.flatnonzero(good["entry"] < tc.LEAF)
    leaf = np.flatnonzero(good["entry"] >= tc.LEAF)

    def broken(field, at, value):
        n = good.copy()
        n[field][at] = value
        return n

    cases = {
        "a leaf's exit": broken("exit", leaf[2], leaf[2] + 2),
        "a payload past the shapes": broken("entry", leaf[2], tc.LEAF + len(leaf)),
        "a shape in two leaves": broken("entry", leaf[2], good["entry"][leaf[3]]),
        "an entry that is not i + 1": broken("entry", inner[1], inner[1] + 2),
        "an exit at i + 1": broken("exit", inner[1], inner[1] + 1),
        "an exit past the slice": broken("exit", inner[1], len(good) + 1),
        "an exit of 2^32 - 1": broken("exit", 0, 0xFFFFFFFF),
        "a range its children do not tile": broken("exit", 0, good["exit"][0] + 3),
        "a leaf first": broken("entry", 0, tc.LEAF),
    }
    for label, nodes in cases.items():
        assert _refused(nodes), label
        boxes = np.zeros((len(leaf), 6), F)
        n = nodes.copy()
        assert _abi.lib().hks_refit_boxes(boxes.ctypes.data, len(boxes), n.ctypes.data, len(n)) == _abi.HK_ERR_INVALID, label


def test_python_tree_cost_raises_on_a_malformed_tree():
    from hikari_amd import HikariError, TreeCost, tree_cost
    good = host_scene_array(ic.case("no_large")[0].desc, 5, tc.NODE_DT)
    assert tree_cost(good).total(2.0, 0.5) == (2.0 * tree_cost(good).inner + 0.5 * tree_cost(good).leaf) / 2.0 ** 32
    assert tree_cost(np.zeros(0, tc.NODE_DT)) == TreeCost()
    with pytest.raises(HikariError, match="hks_tree_cost refused"):
        tree_cost(good[:-3])
    with pytest.raises(ValueError):
        tree_cost(np.zeros(33, np.uint8))
