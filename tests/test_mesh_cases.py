"""The mesh-rebuild cases (tests/mesh_cases.py) on the CPU: the host builder alone confirms that every case sits where
its name says (triangle counts, the split path a BLAS enters, `halves`, zeros of both signs, the stack bounds, the
alias count), that scene1's BLAS is another tree than scene0's (so a refit that kept the tree would fail the GPU
test), that the frame cases' camera sees the meshes, and that Scene.mesh_index restates the builder's concatenation.
tests/test_gpu_mesh_update.py runs the same cases through hk_update_meshes."""
import re
from pathlib import Path

import numpy as np
import pytest

import dynamic_cases as dc
import mesh_cases as mc
from parity import NODE_DT, canon_plane, host_scene_array

ROOT = Path(__file__).resolve().parent.parent
PRIM_DT = np.dtype([("v", [("position", "<f4", 3), ("index", "<u4")], 3)])
VERTEX_DT = np.dtype([("position", "<f4", 3), ("u", "<f4"), ("normal", "<f4", 3), ("v", "<f4")])


def _prims(desc, index):
    k = (index[3] + 2) // 3
    return host_scene_array(desc, 1, PRIM_DT)[index[1]: index[1] + k]


def _both(name):
    scene0, scene1 = mc.case(name)
    return scene0, scene1, scene0.desc, mc.built1(name)


def test_every_case_is_listed():
    assert set(mc.FRAME_CASES) | set(mc.SECOND_UPDATE_CASES) | set(mc.LISTED) | set(mc.COINCIDENT) <= set(mc.CASES)
    for name in ("tris_1", "tris_2", "tris_128", "tris_129", "tris_256", "tris_257", "tris_1280", "tris_1281",
                 "tris_2600", "many_meshes", "one_of_three", "shared_mesh", "emissive_mesh", "coincident_100",
                 "coincident_300", "degenerate", "neg_zero", "strip", "keep_normals", "deepen_16", "deepen_17",
                 "shallower"):
        assert name in mc.CASES
    src = (ROOT / "bevy-hikari_amd" / "csrc" / "hk_dynamic.hip").read_text()
    for text in ("COOP_MIN = 128;", "BVH_LDS_SHAPES = 1280;", "base += 256u"):  # the constants the sizes straddle
        assert text in src, text


@pytest.mark.parametrize("name", list(mc.CASES))
def test_pairs_share_topology_and_differ_in_geometry(name):
    """Both scenes: the same mesh slices, primitive vertex indices, uvs, instances' models and materials; the listed
    meshes' positions differ, every other mesh's vertex and primitive bytes are equal."""
    scene0, scene1, d0, d1 = _both(name)
    assert mc.mesh_slices(d0) == mc.mesh_slices(d1)
    for k in range(9):
        assert getattr(d0, dc_array(k)).count == getattr(d1, dc_array(k)).count
    p0, p1 = host_scene_array(d0, 1, PRIM_DT), host_scene_array(d1, 1, PRIM_DT)
    v0, v1 = host_scene_array(d0, 0, VERTEX_DT), host_scene_array(d1, 0, VERTEX_DT)
    assert np.array_equal(p0["v"]["index"], p1["v"]["index"])
    assert v0["u"].tobytes() == v1["u"].tobytes() and v0["v"].tobytes() == v1["v"].tobytes()
    assert scene0.instance_models().tobytes() == scene1.instance_models().tobytes()
    assert host_scene_array(d0, 6, np.dtype((np.void, 80))).tobytes() == host_scene_array(d1, 6, np.dtype((np.void, 80))).tobytes()
    for i in range(len(scene0.meshes)):
        v, p, n0, nc = scene1.mesh_index(i)
        nv, k = len(scene0.meshes[i].positions), (nc + 2) // 3
        same = v0[v: v + nv].tobytes() == v1[v: v + nv].tobytes() and p0[p: p + k].tobytes() == p1[p: p + k].tobytes()
        assert same == (i not in mc.listed(name)), i
        if i in mc.listed(name):
            assert v0["position"][v: v + nv].tobytes() != v1["position"][v: v + nv].tobytes()


def dc_array(k):
    from parity import SCENE_ARRAYS
    return SCENE_ARRAYS[k]


def test_normals_differ_in_most_cases_and_stay_in_keep_normals():
    differ = 0
    for name in mc.CASES:
        _, scene1, d0, d1 = _both(name)
        v0, v1 = host_scene_array(d0, 0, VERTEX_DT), host_scene_array(d1, 0, VERTEX_DT)
        differ += v0["normal"].tobytes() != v1["normal"].tobytes()
        if name == "keep_normals":
            assert v0["normal"].tobytes() == v1["normal"].tobytes()
            assert all(m.normals is None for m in mc.update_source(name).meshes)
            assert (v0["normal"] != np.array([0, 0, 1], np.float32)).any()  # and they are not the default ones
    assert differ >= 2


@pytest.mark.parametrize("name", list(mc.SIZES))
def test_triangle_counts_and_split_paths(name):
    """The deformed mesh has exactly the triangles its name says, in 3k - 2 nodes; its root is split per thread up to
    COOP_MIN shapes and by the whole block above; tris_257 needs a second 256-chunk of the ballot ranking; tris_1280 is
    the last LDS-staged build and tris_1281 the first global one; tris_2600 has big segments on several levels."""
    n = mc.SIZES[name]
    scene0, scene1, d0, d1 = _both(name)
    index = scene1.mesh_index(0)
    assert index == (0, 0, 0, 3 * n - 2) and len(_prims(d1, index)) == n
    for d in (d0, d1):
        trees = dc.subtrees(mc.mesh_nodes(d, index))
        assert len(trees) == 2 * n - 1 and trees[0][1] == n
        big_levels = {depth for _, k, depth in trees if k > dc.COOP_MIN}
        assert bool(big_levels) == (n > dc.COOP_MIN)
        if name == "tris_2600":
            assert len(big_levels) >= 3
    assert (n > dc.COOP_MIN) == (name not in ("tris_1", "tris_2", "tris_128"))
    assert (n > dc.BALLOT_CHUNK) == (name in ("tris_257", "tris_1280", "tris_1281", "tris_2600"))
    assert (n > dc.BVH_LDS_SHAPES) == (name in ("tris_1281", "tris_2600"))


def test_many_meshes_fill_both_build_launches():
    """40 meshes, all listed: several at most BVH_LDS_SHAPES triangles and several above, so both instantiations of the
    build run workgroups with blockIdx.x > 0, on scratch slices that start past 0; sizes on both sides of COOP_MIN."""
    scene0, scene1, d0, d1 = _both("many_meshes")
    sizes = [(scene1.mesh_index(i)[3] + 2) // 3 for i in mc.listed("many_meshes")]
    assert sizes == mc.MANY_SIZES and len(sizes) == 40
    small = [s for s in sizes if s <= dc.BVH_LDS_SHAPES]
    assert len(small) >= 2 and len(sizes) - len(small) >= 2
    assert sizes[0] <= dc.BVH_LDS_SHAPES < sizes[3]  # neither launch's table is in list order from the start
    assert min(sizes) == 1 and any(s <= dc.COOP_MIN for s in sizes) and any(dc.COOP_MIN < s <= dc.BVH_LDS_SHAPES for s in sizes)
    assert dc.BVH_LDS_SHAPES in sizes and dc.BVH_LDS_SHAPES + 1 in sizes


@pytest.mark.parametrize("name", [n for n in mc.CASES if n not in mc.COINCIDENT and n not in ("tris_1", "tris_2")])
def test_the_rebuilt_tree_is_another_tree(name):
    """The listed meshes' entry / exit words differ between scene0's and scene1's host builds: the update has to build,
    a refit of the old tree cannot pass.  (many_meshes: every listed mesh of 8 triangles or more.)"""
    scene0, scene1, d0, d1 = _both(name)
    for i in mc.listed(name):
        index = scene1.mesh_index(i)
        if (index[3] + 2) // 3 < (8 if name == "many_meshes" else 3):
            continue
        a, b = mc.mesh_nodes(d0, index), mc.mesh_nodes(d1, index)
        assert not (np.array_equal(a["entry"], b["entry"]) and np.array_equal(a["exit"], b["exit"])), i


@pytest.mark.parametrize("name", list(mc.COINCIDENT))
def test_coincident_centroids_split_in_halves(name):
    """scene1: every triangle's box is centred on the origin exactly, so every split of its BLAS is `halves`: at 100
    shapes in split_segment, at 300 in coop_split first."""
    n = mc.COINCIDENT[name]
    _, scene1, _, d1 = _both(name)
    index = scene1.mesh_index(0)
    pos = _prims(d1, index)["v"]["position"]
    centre = (pos.min(axis=1) + pos.max(axis=1)) * np.float32(0.5)
    assert len(pos) == n and not centre.any()
    trees = {a: k for a, k, _ in dc.subtrees(mc.mesh_nodes(d1, index))}
    nodes = mc.mesh_nodes(d1, index)
    for a, k in trees.items():
        if k > 1:
            assert (int(nodes["exit"][a]) - a + 1) // 3 == k // 2
    assert (n > dc.COOP_MIN) == (name == "coincident_300")


def test_degenerate_has_zero_area_and_repeated_vertices():
    _, scene1, _, d1 = _both("degenerate")
    pos = _prims(d1, scene1.mesh_index(0))["v"]["position"].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]), axis=1)
    assert (pos[7, 0] == pos[7, 1]).all() and (pos[7, 0] == pos[7, 2]).all() and area[7] == 0.0
    assert area[12] < 1e-6 * np.median(area)
    p = scene1.meshes[0].positions
    assert len(np.unique(p, axis=0)) <= len(p) - 3


def test_neg_zero_has_zeros_of_both_signs_in_triangles_and_sibling_boxes():
    _, scene1, _, d1 = _both("neg_zero")
    index = scene1.mesh_index(0)
    bits = _prims(d1, index)["v"]["position"].view(np.uint32)  # (tris, 3 corners, 3 axes)
    plus, minus = (bits == 0).any(axis=1), (bits == 0x80000000).any(axis=1)
    assert (plus & minus).any(axis=0).all()  # on every axis some triangle has +0 and -0 among its corners
    nodes = mc.mesh_nodes(d1, index)
    inner = nodes[nodes["entry"] < 0x80000000]
    for field in ("min", "max"):
        b = inner[field].view(np.uint32)
        assert (b == 0).any() and (b == 0x80000000).any()
    # the local AABB the tests hand to the update is the host builder's: the instance boxes of the host build follow
    # from it with the device's own arithmetic only if the zero bounds carry the host's sign
    assert mc.local_aabbs(scene1).shape == (2, 6)


def test_strip_is_a_triangle_strip_with_alternating_winding():
    _, scene1, _, d1 = _both("strip")
    assert scene1.meshes[0].topology == 1
    index = scene1.mesh_index(0)
    ix = _prims(d1, index)["v"]["index"]
    assert len(ix) == mc.STRIP_TRIS and ix[0].tolist() == [0, 1, 2] and ix[1].tolist() == [2, 1, 3]
    assert ix[2].tolist() == [2, 3, 4]


def test_emissive_mesh_is_an_emitter_of_65_triangles():
    scene0, scene1, d0, d1 = _both("emissive_mesh")
    em0 = np.frombuffer(host_scene_array(d0, 8, np.dtype((np.void, 64))).tobytes(), np.uint32).reshape(-1, 16)
    em1 = np.frombuffer(host_scene_array(d1, 8, np.dtype((np.void, 64))).tobytes(), np.uint32).reshape(-1, 16)
    assert em0[:, 8].tolist() == [1, 2] and em0[:, 11].tolist() == [mc.EMISSIVE_TRIS, 2]  # instance, alias count
    assert d1.alias_table.count == mc.EMISSIVE_TRIS + 2 and mc.EMISSIVE_TRIS == dc.WAVE + 1
    assert em0[0, 12] != em1[0, 12] and em0[1, 12] == em1[1, 12]  # surface_area
    assert host_scene_array(d0, 3, np.dtype((np.void, 8))).tobytes() != host_scene_array(d1, 3, np.dtype((np.void, 8))).tobytes()
    assert host_scene_array(d0, 7, NODE_DT).tobytes() != host_scene_array(d1, 7, NODE_DT).tobytes()  # light BVH box


def test_stack_bounds_of_the_depth_cases():
    """hk_scene_gbuffer_stack: deepen_16 / deepen_17 go from a shallow scene to exactly 16 (every LDS level of the
    shallow walk) and 17 (the deep walk); shallower falls from the first mesh's depth to the second's, which is
    unlisted and as deep in both scenes."""
    from hikari_amd.plugin import scene_gbuffer_stack
    for name, want in (("deepen_16", 16), ("deepen_17", 17)):
        _, scene1, d0, d1 = _both(name)
        assert scene_gbuffer_stack(d0)[0] < 8 and scene_gbuffer_stack(d1) == (want, dc.GB_STACK_LDS)
        assert dc.inner_depth(mc.mesh_nodes(d1, scene1.mesh_index(0))) == mc.DEEPEN[name] - 1
    _, scene1, d0, d1 = _both("shallower")
    a, b = mc.SHALLOWER
    first = [dc.inner_depth(mc.mesh_nodes(d, scene1.mesh_index(0))) for d in (d0, d1)]
    second = [dc.inner_depth(mc.mesh_nodes(d, scene1.mesh_index(1))) for d in (d0, d1)]
    assert first[0] == a - 1 and second == [b - 1, b - 1] and first[1] < b - 1
    tlas = [dc.inner_depth(host_scene_array(d, 5, NODE_DT)) for d in (d0, d1)]
    assert scene_gbuffer_stack(d0)[0] == tlas[0] + a - 1 and scene_gbuffer_stack(d1)[0] == tlas[1] + b - 1
    assert scene_gbuffer_stack(d1)[0] < scene_gbuffer_stack(d0)[0]
    _, _, d0, d1 = _both("too_deep")  # one past the deepest scene the walk takes, from a shallow one
    assert scene_gbuffer_stack(d0)[0] <= dc.GB_STACK_LDS and scene_gbuffer_stack(d1)[0] == dc.GB_STACK + 1


@pytest.mark.parametrize("name", mc.FRAME_CASES)
def test_the_camera_sees_the_mesh(name):
    """The oracle alone, on the host-built scene1: depth > 0 on more than 0.2 of the frame's pixels."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    cam, lights = mc.camera_for(name)
    w, h = mc.FRAME_SIZE
    o = Oracle(mc.built1(name), load_noise(), w, h, 1.0)
    o.render_gbuffer(frame_inputs(0, cam, lights, w, h))
    depth = canon_plane(11, o.output(11)).view(np.float32).reshape(h, w, 4)[..., 3]
    o.close()
    assert (depth > 0).mean() > 0.2


def test_mesh_index_restates_the_builders_concatenation():
    """Scene.mesh_index(mesh) equals the hk_mesh_index in the host-built instance record of every instance of
    cornell, city and many_meshes."""
    from hikari_amd import examples
    scenes = [examples.SCENES["cornell"]()[0], examples.SCENES["city"]()[0], mc.case("many_meshes")[1]]
    for scene in scenes:
        desc = scene.build()
        slices = mc.mesh_slices(desc)
        assert len(slices) == len(scene.instances)
        for (mesh, _, _), got in zip(scene.instances, slices):
            assert scene.mesh_index(mesh) == got


def test_local_aabbs_equal_the_scenes_own_without_zeros():
    scene1 = mc.case("tris_129")[1]
    assert mc.local_aabbs(scene1).tobytes() == scene1.instance_local_aabbs().tobytes()


def test_header_documents_and_abi_declares_hk_update_meshes():
    import ctypes as C

    import hikari_amd
    header = (ROOT / "include" / "hikari_amd.h").read_text()
    doc = header[header.index("Deforming meshes"):header.index("int hk_update_meshes(")]
    for text in ("mesh.rs:77-166", "mod.rs:379-467", "instance.rs:193-206, 287-293", "HK_ERR_INVALID", "HK_ERR_STATE",
                 "listed twice", "NULL", "3k - 2", "Waits for the", "typedef struct hk_mesh_update"):
        assert text in doc, text
    assert re.search(r"#define HK_ABI_VERSION\s+3\b", header)
    A = hikari_amd._abi
    assert "hk_update_meshes" in A.EXPORTED_SYMBOLS
    assert C.sizeof(A.hk_mesh_update) == 40 and A.hk_mesh_update.positions.offset == 24
    assert A.lib().hk_update_meshes.argtypes[1] == C.POINTER(A.hk_mesh_update)
    assert callable(hikari_amd.HikariRenderer.update_meshes) and callable(hikari_amd.HikariPlugin.update_meshes)
