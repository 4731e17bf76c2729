"""The instance-refit cases (tests/instance_refit_cases.py) on the CPU: the host builder and hks_refit_boxes alone confirm
that every case sits where its name says (the counts, the ranges either side of REFIT_SMALL in both trees, nested large
ranges, the build kinds, the chain's depth, stale trees, zeros of both signs), that the constant the cases restate is the
source's, that the ABI declares and documents the calls, and what a refit over unchanged models gives.
tests/test_gpu_instance_refit.py runs the same cases through hk_refit_instances."""
import re
from pathlib import Path

import numpy as np
import pytest

import dynamic_cases as dc
import instance_refit_cases as ic
from parity import NODE_DT, host_scene_array

ROOT = Path(__file__).resolve().parent.parent
INST_DT, EM_DT = np.dtype((np.void, 176)), np.dtype((np.void, 64))


def _trees(desc):
    return host_scene_array(desc, 5, NODE_DT), host_scene_array(desc, 7, NODE_DT)


def _words(nodes):
    return np.frombuffer(np.ascontiguousarray(nodes).tobytes(), np.uint32).reshape(-1, 8)


def test_the_constants_are_the_sources():
    src = (ROOT / "bevy-hikari_amd" / "csrc" / "hk_dynamic.hip").read_text()
    assert re.findall(r"constexpr uint32_t REFIT_SMALL = (\d+);", src) == [str(ic.REFIT_SMALL)]
    assert src.count("e - i > REFIT_SMALL") == 2  # the mesh kernels' comparison and the instance trees', one constant
    assert re.findall(r"constexpr uint32_t BVH_LDS_SHAPES = (\d+);", src) == [str(dc.BVH_LDS_SHAPES)]
    assert ic.REFIT_SMALL % 3 == 2  # a range is 3p - 1: the limit itself is a range that exists (p = 11)


def test_every_case_of_the_issue_is_listed():
    assert set(ic.COUNTS) == set(ic.CASES)
    for group in (ic.REPEAT_CASES, ic.BUILD_CASES, ic.FRAME_CASES, [ic.VARIANT_CASE]):
        assert set(group) <= set(ic.CASES)
    assert ic.FRAME_SIZE == (64, 48)
    assert max(n for n, _ in ic.COUNTS.values()) <= 3000  # a few thousand instances at the most


@pytest.mark.parametrize("name", ic.CASES)
def test_counts_and_pairs(name):
    """The counts the name promises, 3k - 2 nodes per tree, the same emitters in both scenes, other models in scene1
    (unless the case is `unchanged`)."""
    scene0, scene1 = ic.case(name)
    d0, d1 = scene0.desc, ic.built1(name)
    n, m = ic.COUNTS[name]
    for d in (d0, d1):
        assert (d.instances.count, d.emissives.count) == (n, m)
        assert d.instance_nodes.count == 3 * n - 2 and d.emissive_nodes.count == (3 * m - 2 if m else 0)
    e0 = np.frombuffer(host_scene_array(d0, 8, EM_DT).tobytes(), np.uint32).reshape(-1, 16)
    e1 = np.frombuffer(host_scene_array(d1, 8, EM_DT).tobytes(), np.uint32).reshape(-1, 16)
    assert np.array_equal(e0[:, [8, 10, 11]], e1[:, [8, 10, 11]])  # instance and alias range
    same = np.array_equal(scene0.instance_models(), scene1.instance_models())
    assert same == (name == "unchanged")


def test_edge_sizes():
    for name, (n, m) in (("n1_m0", (1, 0)), ("n1_m1", (1, 1)), ("n2", (2, 1))):
        tlas, lbvh = _trees(ic.case(name)[0].desc)
        assert len(tlas) == 3 * n - 2 and len(lbvh) == (1 if m else 0)
        assert ic.large_nodes(tlas) == 0
        if n == 1:
            assert tlas["entry"][0] == 0x80000000 and len(ic.ranges(tlas)) == 0  # a lone leaf: nothing to fold
        else:
            assert sorted(ic.ranges(tlas).tolist()) == [2, 2]
        if m:
            assert lbvh["entry"][0] == 0x80000000


def test_the_threshold_ranges_exist_in_both_trees():
    """The widest range below the root is exactly REFIT_SMALL (no node is large) / REFIT_SMALL + 3 (exactly one is), in
    the TLAS of the tlas_ cases and in the light BVH of the lights_ cases."""
    for name, tree, widest, large in (("tlas_at_32", 0, 32, 0), ("tlas_at_35", 0, 35, 1), ("lights_at_32", 1, 32, 0),
                                      ("lights_at_35", 1, 35, 1)):
        nodes = _trees(ic.case(name)[0].desc)[tree]
        assert ic.widest_range(nodes) == widest and ic.large_nodes(nodes) == large, name
        assert set(ic.ranges(nodes).tolist()) <= {3 * p - 1 for p in range(1, 13)}
    # the lights_ cases' TLAS has large nodes of its own: one list holds both trees' nodes
    assert ic.large_nodes(_trees(ic.case("lights_at_35")[0].desc)[0]) > 0


def test_no_large_and_many_large():
    tlas, lbvh = _trees(ic.case("no_large")[0].desc)
    assert ic.large_nodes(tlas) == 0 and ic.large_nodes(lbvh) == 0 and len(ic.ranges(tlas)) == 20
    tlas, lbvh = _trees(ic.case("many_large")[0].desc)
    assert ic.large_nodes(tlas) > 100 and ic.large_nodes(lbvh) > 5
    assert ic.widest_range(tlas) > 2 * 256  # a range the 256 threads stride over more than once


def test_build_kinds():
    (n0, _), (n1, _) = ic.COUNTS["over_256"], ic.COUNTS["over_lds"]
    assert dc.BALLOT_CHUNK < n0 <= dc.BVH_LDS_SHAPES < n1


def test_the_deep_case_keeps_a_chain_at_the_stack_limit():
    scene0, scene1 = ic.case("deep")
    assert dc.stack_need(scene0) == dc.GB_STACK  # the deepest scene the G-buffer walk takes
    tlas0, tlas1 = _trees(scene0.desc)[0], _trees(ic.built1("deep"))[0]
    assert dc.inner_depth(tlas0) == dc.GB_STACK - 1 and dc.inner_depth(tlas1) < 16
    assert ic.large_nodes(tlas0) > 50  # every upper level is a large node over the levels below


def test_stale_trees_swapped_and_coincident():
    """swapped: instance k takes the place of instance n - 1 - k, so the kept tree's leaves are as far from where it put
    them as the scene allows and sibling boxes overlap; coincident: every instance has one model."""
    from hikari_amd import Scene
    scene0, scene1 = ic.case("swapped")
    assert np.array_equal(scene0.instance_models(), scene1.instance_models()[::-1])
    t0 = _trees(scene0.desc)[0]
    t1 = host_scene_array(ic.refitted("swapped"), 5, NODE_DT)

    def volume(t):
        inner = t["entry"] < 0x80000000
        return float(np.prod((t["max"][inner] - t["min"][inner]).astype(np.float64), axis=1).sum())
    assert volume(t1) > 2.0 * volume(t0)
    m = ic.case("coincident")[1].instance_models()
    assert (m == m[0]).all()
    # the quads' boxes are one box (the four emitters' strips have other local boxes), and every entry node's range holds
    # a quad, so every entry box contains it
    d = ic.refitted("coincident")
    f = np.frombuffer(host_scene_array(d, 4, INST_DT).tobytes(), np.float32).reshape(-1, 44)
    emitters = np.frombuffer(host_scene_array(d, 8, EM_DT).tobytes(), np.uint32).reshape(-1, 16)[:, 8]
    quads = np.delete(f, emitters, axis=0)
    assert (quads[:, 0:3] == quads[0, 0:3]).all() and (quads[:, 4:7] == quads[0, 4:7]).all()
    t = host_scene_array(d, 5, NODE_DT)
    wide = t[(t["entry"] < 0x80000000) & (t["exit"] - np.arange(len(t)) > 3 * len(emitters) + 2)]
    assert len(wide) > 20 and (wide["min"] <= quads[0, 0:3]).all() and (wide["max"] >= quads[0, 4:7]).all()


def test_neg_zero_has_bounds_of_both_signs():
    t = host_scene_array(ic.refitted("neg_zero"), 5, NODE_DT)
    inner = t["entry"] < 0x80000000
    w = _words(t[inner])[:, [0, 1, 2, 4, 5, 6]]
    assert (w == 0x80000000).any() and (w == 0).any()


@pytest.mark.parametrize("name", ["unchanged", "n2", "neg_zero"])
def test_a_refit_over_unchanged_models_gives_the_built_boxes(name):
    """A tree refit over the boxes it was built from: entry and exit words identical, every box equal as floats.  Only
    the sign of a zero bound may differ: the build joins child boxes with std::fmin / std::fmax, which of the two
    zeros keep the second operand (the sign depends on the order of the shapes), while the refit's fold orders
    -0 < +0 whatever the order.  Every word that differs is therefore a zero in both trees."""
    from hikari_amd import Scene
    scene = ic.case(name)[1]
    d = ic.built1(name)
    got = Scene.refitted_instances(d, scene)
    for idx in (5, 7):
        a, b = host_scene_array(got, idx, NODE_DT), host_scene_array(d, idx, NODE_DT)
        assert np.array_equal(a["entry"], b["entry"]) and np.array_equal(a["exit"], b["exit"])
        assert np.array_equal(a["min"], b["min"]) and np.array_equal(a["max"], b["max"])
        differ = _words(a) != _words(b)
        assert ((_words(a)[differ] | 0x80000000) == 0x80000000).all()
        assert ((_words(b)[differ] | 0x80000000) == 0x80000000).all()
    for idx, dt in ((4, INST_DT), (8, EM_DT)):
        assert host_scene_array(got, idx, dt).tobytes() == host_scene_array(d, idx, dt).tobytes()


def test_the_abi_declares_and_documents_the_calls():
    from hikari_amd import _abi
    header = (ROOT / "include" / "hikari_amd.h").read_text()
    scene_h = (ROOT / "include" / "hikari_scene.h").read_text()
    for fn in ("hk_refit_instances", "hk_refit_meshes_all", "hk_skin_meshes_refit_all"):
        assert re.search(rf"^int {fn}\(hk_ctx\* ctx,", header, flags=re.M), fn
        assert fn in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), fn)
    assert re.search(r"^int hks_refit_boxes\(const float\* boxes, uint32_t count, hk_node\* nodes, uint32_t node_count\);",
                     scene_h, flags=re.M)
    assert "hks_refit_boxes" in _abi.EXPORTED_SYMBOLS
    for text in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "hk_refit_instances" in (ROOT / text).read_text(), text
