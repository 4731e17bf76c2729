"""The refit cases (tests/refit_cases.py) on the CPU: the host builder and hks_refit_nodes alone confirm that every case
sits where its name says (entry node counts, the ranges either side of REFIT_SMALL, nested small and large ranges, the
slice counts, overlapping sibling boxes), that the constant the cases restate is the source's, that the ABI declares and
documents the calls, and that the oracle renders the frame cases' refitted scenes and sees the meshes.
tests/test_gpu_refit.py runs the same cases through hk_refit_meshes."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import dynamic_cases as dc
import mesh_cases as mc
import refit_cases as rc
from parity import NODE_DT, canon_plane, host_scene_array

ROOT = Path(__file__).resolve().parent.parent


def _nodes(name, desc=None, mesh=None):
    scene0, _ = rc.case(name)
    mesh = rc.listed(name)[0] if mesh is None else mesh
    return mc.mesh_nodes(scene0.desc if desc is None else desc, scene0.mesh_index(mesh))


def test_the_constant_is_the_sources():
    src = (ROOT / "bevy-hikari_amd" / "csrc" / "hk_dynamic.hip").read_text()
    found = re.findall(r"constexpr uint32_t REFIT_SMALL = (\d+);", src)
    assert found == [str(rc.REFIT_SMALL)]
    assert "e - i > REFIT_SMALL" in src  # the comparison the cases straddle
    assert rc.REFIT_SMALL % 3 == 2  # a range is 3p - 1: the limit itself is a range that exists (p = 11)


def test_every_case_of_the_issue_is_listed():
    for name in ("tris_1", "tris_2", "small_32", "small_35", "tris_1281", "tris_2600", "deep_17", "deep_65",
                 "many_meshes", "one_of_three", "shared_mesh", "emissive_mesh", "strip", "keep_normals", "neg_zero",
                 "coincident_300", "folded"):
        assert name in rc.CASES
    assert set(rc.FRAME_CASES) | set(rc.REPEAT_CASES) | set(rc.VARIANT_CASES) <= set(rc.CASES)
    assert rc.FRAME_SIZE == (32, 24)


@pytest.mark.parametrize("name", rc.CASES)
def test_pairs_share_topology_and_differ_in_the_listed_meshes(name):
    scene0, scene1 = rc.case(name)
    d0, d1 = scene0.desc, rc.built1(name)
    assert mc.mesh_slices(d0) == mc.mesh_slices(d1)
    p0 = np.frombuffer(host_scene_array(d0, 1, np.dtype((np.void, 48))).tobytes(), np.uint32).reshape(-1, 3, 4)
    p1 = np.frombuffer(host_scene_array(d1, 1, np.dtype((np.void, 48))).tobytes(), np.uint32).reshape(-1, 3, 4)
    assert np.array_equal(p0[:, :, 3], p1[:, :, 3])  # the stored vertex indices
    for i in range(len(scene0.meshes)):
        _, p, n0, nc = scene1.mesh_index(i)
        k = (nc + 2) // 3
        assert (p0[p: p + k].tobytes() != p1[p: p + k].tobytes()) == (i in rc.listed(name)), i


def test_tris_1_has_no_entry_node_and_tris_2_has_two():
    a, b = _nodes("tris_1"), _nodes("tris_2")
    assert len(a) == 1 and a["entry"][0] >= 0x80000000 and len(rc.spans(a)) == 0
    assert len(b) == 4 and rc.spans(b).tolist() == [2, 2]


def test_small_cases_sit_either_side_of_the_limit():
    """small_32: the largest range is exactly REFIT_SMALL, so no node is large; small_35: the root's two children are
    the next range that exists (REFIT_SMALL + 3) and the one below, and they alone are large."""
    a, b = rc.spans(_nodes("small_32")), rc.spans(_nodes("small_35"))
    assert a.max() == rc.REFIT_SMALL and (a > rc.REFIT_SMALL).sum() == 0
    assert b.max() == rc.REFIT_SMALL + 3 and (b > rc.REFIT_SMALL).sum() == 1
    assert sorted(b)[-2] == rc.REFIT_SMALL
    assert ((a + 1) % 3 == 0).all() and ((b + 1) % 3 == 0).all()  # 3p - 1, every one


@pytest.mark.parametrize("name, least", [("tris_1281", 100), ("tris_2600", 200)])
def test_big_grids_have_large_nodes_on_several_levels(name, least):
    nodes = _nodes(name)
    large = {depth for a, k, depth in dc.subtrees(nodes) if a and 3 * k - 1 > rc.REFIT_SMALL}
    assert (rc.spans(nodes) > rc.REFIT_SMALL).sum() >= least and len(large) >= 4
    assert rc.spans(nodes).max() > 256 * 3  # a range the 256 threads stride over more than once


@pytest.mark.parametrize("name, levels", [("deep_17", 17), ("deep_65", 65)])
def test_deep_cases_nest_small_ranges_inside_large_ones(name, levels):
    nodes = _nodes(name)
    assert dc.inner_depth(nodes) == levels
    spans = rc.spans(nodes)
    inner = np.flatnonzero(nodes["entry"] < 0x80000000)
    large = [(int(i), int(i + s)) for i, s in zip(inner, spans) if s > rc.REFIT_SMALL]
    small = [int(i) for i, s in zip(inner, spans) if s <= rc.REFIT_SMALL]
    assert len(large) >= 5 and len(small) >= 5
    # a chain: every large range but the outermost two lies inside another large one, and small ones inside them
    nested = sum(any(a < i and e <= b for a, b in large if (a, b) != (i, e)) for i, e in large)
    assert nested >= len(large) - 2
    assert sum(any(a < i < b for a, b in large) for i in small) >= 0.9 * len(small)


def test_many_meshes_and_one_of_three_list_what_they_say():
    scene0, scene1 = rc.case("many_meshes")
    assert len(rc.listed("many_meshes")) == 40 == len(scene0.meshes) - 1
    with_large = sum((rc.spans(_nodes("many_meshes", mesh=i)) > rc.REFIT_SMALL).any() for i in rc.listed("many_meshes"))
    assert 10 <= with_large <= 30  # slices with and without large nodes in one call
    assert rc.listed("one_of_three") == [1] and len(rc.case("one_of_three")[0].meshes) == 4


def test_folded_grid_has_overlapping_sibling_boxes():
    """After the refit the root's two child boxes share most of their area in the xy plane (the left half lies on the
    right one); scene0's and the rebuilt tree's share little."""
    def overlap(nodes):
        a, b = nodes[0], nodes[int(nodes["exit"][0])]
        lo, hi = np.maximum(a["min"], b["min"])[:2], np.minimum(a["max"], b["max"])[:2]
        area = min(np.prod((a["max"] - a["min"])[:2]), np.prod((b["max"] - b["min"])[:2]))
        return float(np.prod(np.clip(hi - lo, 0.0, None)) / area)
    assert overlap(_nodes("folded", rc.refitted("folded"))) > 0.8
    assert overlap(_nodes("folded")) < 0.2 and overlap(_nodes("folded", rc.built1("folded"))) < 0.2


@pytest.mark.parametrize("name", rc.CASES)
def test_refitted_scene_keeps_the_topology_and_differs_from_the_rebuilt_one(name):
    scene0, scene1 = rc.case(name)
    d = rc.refitted(name)
    for i in rc.listed(name):
        index = scene0.mesh_index(i)
        a, b = mc.mesh_nodes(scene0.desc, index), mc.mesh_nodes(d, index)
        assert np.array_equal(a["entry"], b["entry"]) and np.array_equal(a["exit"], b["exit"])
        if len(a) > 1:
            assert a.tobytes() != b.tobytes()
    if name in ("tris_1281", "tris_2600", "folded", "shared_mesh", "keep_normals"):
        built = host_scene_array(rc.built1(name), 2, NODE_DT)
        got = host_scene_array(d, 2, NODE_DT)
        assert not np.array_equal(built["exit"], got["exit"])  # the rebuild is another tree: the refit is not it


@pytest.mark.parametrize("name", rc.FRAME_CASES)
def test_the_oracle_renders_the_refitted_scene_and_sees_the_mesh(name):
    """One 32 x 24 frame of the oracle on the refitted desc, without error; depth > 0 on at least 0.2 of the pixels."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs, load_noise
    from oracle import Oracle
    from parity import passes
    scene0, _ = rc.case(name)
    cam, lights = rc.camera_for(name)
    w, h = rc.FRAME_SIZE
    o = Oracle(scene0.desc, load_noise(), w, h, 1.0)
    o.set_scene(rc.refitted(name))
    passes(o, HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False).to_c(),
           frame_inputs(0, cam, lights, w, h))
    depth = canon_plane(11, o.output(11)).view(np.float32).reshape(h, w, 4)[..., 3]
    lit = canon_plane(10, o.output(10)).view(np.float16).astype(np.float32)
    o.close()
    assert (depth > 0).mean() >= 0.2 and np.isfinite(lit).all()


def test_header_documents_and_abi_declares_the_refit_calls():
    import ctypes as C

    import hikari_amd
    header = (ROOT / "include" / "hikari_amd.h").read_text()
    doc = header[header.index("BLAS refit (DESIGN"):header.index("int hk_skin_meshes_refit(")]
    for text in ("hk_refit.h", "QUALITY DEGRADES", "walks more nodes", "hk_update_meshes / hk_skin_meshes",
                 "mesh.rs:77-166", "hks_refit_nodes", "int hk_refit_meshes("):
        assert text in doc, text
    assert re.search(r"#define HK_ABI_VERSION\s+3\b", header)
    A = hikari_amd._abi
    for name in ("hk_refit_meshes", "hk_skin_meshes_refit", "hks_refit_nodes"):
        assert name in A.EXPORTED_SYMBOLS
    assert A.lib().hk_refit_meshes.argtypes == A.lib().hk_update_meshes.argtypes
    assert A.lib().hk_skin_meshes_refit.argtypes == A.lib().hk_skin_meshes.argtypes
    assert A.lib().hk_refit_meshes.argtypes[1] == C.POINTER(A.hk_mesh_update)
    for cls in (hikari_amd.HikariRenderer, hikari_amd.HikariPlugin):
        for fn in (cls.update_meshes, cls.skin_meshes):
            assert inspect.signature(fn).parameters["refit"].default is False
    for src in ("hk_scene.cpp", "hk_dynamic.hip"):
        assert "hk_refit.h" in (ROOT / "bevy-hikari_amd" / "csrc" / src).read_text()
