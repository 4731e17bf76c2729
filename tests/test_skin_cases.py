"""The skin cases (tests/skin_cases.py) on the CPU: the host builder and hks_skin_vertices alone confirm that every case
sits where its name says (vertex and triangle counts, joint counts and the indices used, which meshes keep their
bytes, zeros of both signs, the normals that stay), that a posed mesh's BLAS is another tree than the bind pose's (so a
refit that kept the tree would fail the GPU test), that posing moves the emitters' areas, and that Scene.posed holds
hks_skin_vertices' output where tests/skin_numpy.py says it should.  tests/test_gpu_skin.py runs the same cases through
hk_set_mesh_skins and hk_skin_meshes."""
import re
from pathlib import Path

import numpy as np
import pytest

import mesh_cases as mc
import skin_cases as sc
import skin_numpy as sn
from parity import NODE_DT, host_scene_array
from test_mesh_cases import PRIM_DT, VERTEX_DT
from test_skin_independent import same_words

ROOT = Path(__file__).resolve().parent.parent


def _slices(scene, i):
    v, p, n0, nc = scene.mesh_index(i)
    return v, len(scene.meshes[i].positions), p, (nc + 2) // 3, n0, nc


def test_every_case_is_listed_and_the_edges_are_the_kernels():
    for name in ("verts_3", "verts_63", "verts_64", "verts_65", "verts_256", "verts_257", "tris_1281", "many_skins",
                 "one_of_three", "shared_mesh", "emissive_skin", "scaled_joint", "flat_zero", "keep_normals"):
        assert name in sc.CASES
    assert set(sc.SECOND_POSE_CASES) | set(sc.FRAME_CASES) <= set(sc.CASES)
    assert all(len(sc.case(n).poses) == 2 for n in sc.SECOND_POSE_CASES)
    src = (ROOT / "bevy-hikari_amd" / "csrc" / "hk_dynamic.hip").read_text()
    for text in ("BVH_LDS_SHAPES = 1280;", "k_skin_vertices", "k_skin_bounds", "v += 256u"):
        assert text in src, text
    assert re.search(r"__launch_bounds__\(256\) void k_skin_vertices", src)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_posed_scenes_share_topology_and_hold_the_host_skin(name):
    """The posed scene: the bind pose's slices, vertex indices, uvs, instances and materials; a posed mesh's positions
    (and normals, but for keep_normals) are the restatement's words and differ from the bind pose; every other mesh's
    vertex and primitive bytes are the bind pose's."""
    c = sc.case(name)
    d0 = c.scene0.desc
    v0, p0 = host_scene_array(d0, 0, VERTEX_DT), host_scene_array(d0, 1, PRIM_DT)
    for k, pose in enumerate(c.poses):
        s1, d1 = sc.posed(name, k)
        assert mc.mesh_slices(d0) == mc.mesh_slices(d1)
        v1, p1 = host_scene_array(d1, 0, VERTEX_DT), host_scene_array(d1, 1, PRIM_DT)
        assert np.array_equal(p0["v"]["index"], p1["v"]["index"])
        assert v0["u"].tobytes() == v1["u"].tobytes() and v0["v"].tobytes() == v1["v"].tobytes()
        assert set(pose) <= set(c.skinned)
        for i, m in enumerate(c.scene0.meshes):
            v, nv, p, nt, _, _ = _slices(c.scene0, i)
            if i not in pose:
                assert v0[v: v + nv].tobytes() == v1[v: v + nv].tobytes(), i
                assert p0[p: p + nt].tobytes() == p1[p: p + nt].tobytes(), i
                continue
            keep = i in c.keep_normals
            want_p, want_n = sn.skin(m.positions, None if keep else m.normals, m.skin.joint_indices,
                                     m.skin.joint_weights, pose[i])
            assert same_words(v1["position"][v: v + nv], want_p), i
            assert same_words(v1["normal"][v: v + nv], m.normals if keep else want_n), i
            assert v0["position"][v: v + nv].tobytes() != v1["position"][v: v + nv].tobytes()
            assert len(pose[i]) == m.skin.joint_count and int(m.skin.joint_indices.max()) < m.skin.joint_count


@pytest.mark.parametrize("n", sc.VERTEX_SIZES)
def test_vertex_counts_sit_on_the_wave_and_workgroup_edges(n):
    c = sc.case(f"verts_{n}")
    assert _slices(c.scene0, 0)[:4] == (0, n, 0, n - 2)
    assert (n <= 64) == (n in (3, 63, 64)) and (n <= 256) == (n != 257)


def test_the_big_mesh_takes_the_global_memory_build():
    c = sc.case("tris_1281")
    _, nv, _, nt, _, nc = _slices(c.scene0, 0)
    assert nt == sc.BVH_LDS_SHAPES + 1 and nc == 3 * nt - 2 and nv > 256


def test_many_skins_cover_the_table_search_and_palette_offsets():
    """12 meshes posed in one call; joint counts 1, 2, 7 and 256 in turn, so the palettes start at offsets that are no
    multiple of anything; a 256-joint rig uses index 255; vertex counts on both sides of a workgroup."""
    c = sc.case("many_skins")
    assert len(c.skinned) == 12 and all(set(p) == set(range(12)) for p in c.poses)
    counts = [c.scene0.meshes[i].skin.joint_count for i in range(12)]
    assert counts == [1, 2, 7, 256] * 3
    assert any(int(c.scene0.meshes[i].skin.joint_indices.max()) == 255 for i in range(12))
    nv = [len(c.scene0.meshes[i].positions) for i in range(12)]
    assert min(nv) < 64 and max(nv) > 256
    assert [(_slices(c.scene0, i)[3]) for i in range(12)] == sc.MANY_TRIS


@pytest.mark.parametrize("name", [n for n in sc.CASES if n != "verts_3"])
def test_the_posed_tree_is_another_tree(name):
    """The posed meshes' entry / exit words differ between the bind pose's and the posed scene's host builds.  (A
    one-joint rig moves rigidly or affinely and may keep its tree: many_skins' meshes of one joint, and those under 8
    triangles, are left out.)"""
    c = sc.case(name)
    for k, pose in enumerate(c.poses):
        _, d1 = sc.posed(name, k)
        for i in pose:
            m = c.scene0.meshes[i]
            index = c.scene0.mesh_index(i)
            if name == "many_skins" and (m.skin.joint_count == 1 or (index[3] + 2) // 3 < 8):
                continue
            a, b = mc.mesh_nodes(c.scene0.desc, index), mc.mesh_nodes(d1, index)
            assert not (np.array_equal(a["entry"], b["entry"]) and np.array_equal(a["exit"], b["exit"])), (k, i)


def test_one_of_three_leaves_a_skinned_and_an_unskinned_mesh_alone():
    c = sc.case("one_of_three")
    assert c.skinned == [0, 1] and [set(p) for p in c.poses] == [{1}]
    assert c.scene0.meshes[0].skin is not None and c.scene0.meshes[2].skin is None
    _, d1 = sc.posed("one_of_three")
    n0, n1 = host_scene_array(c.scene0.desc, 2, NODE_DT), host_scene_array(d1, 2, NODE_DT)
    for i in (0, 2):
        a, b = _slices(c.scene0, i)[4:]
        assert n0[a: a + b].tobytes() == n1[a: a + b].tobytes()


def test_shared_mesh_has_five_instances_whose_boxes_all_move():
    c = sc.case("shared_mesh")
    _, d1 = sc.posed("shared_mesh")
    assert mc.mesh_slices(d1)[:5] == [c.scene0.mesh_index(0)] * 5
    inst = np.dtype((np.void, 176))
    a = np.frombuffer(host_scene_array(c.scene0.desc, 4, inst).tobytes(), np.float32).reshape(-1, 44)
    b = np.frombuffer(host_scene_array(d1, 4, inst).tobytes(), np.float32).reshape(-1, 44)
    for k in range(5):
        assert a[k, :7].tobytes() != b[k, :7].tobytes(), k
    assert a[5].tobytes() == b[5].tobytes()  # the light's instance stays


def test_emissive_skin_moves_areas_alias_table_and_light_bvh():
    c = sc.case("emissive_skin")
    _, d1 = sc.posed("emissive_skin")
    d0 = c.scene0.desc
    assert d0.emissives.count == d1.emissives.count == 2 and d0.alias_table.count == sc.EMISSIVE_TRIS + 2
    for idx, size in ((3, 8), (7, 32), (8, 64)):
        dt = np.dtype((np.void, size))
        assert host_scene_array(d0, idx, dt).tobytes() != host_scene_array(d1, idx, dt).tobytes(), idx


def test_scaled_joint_tells_the_inverse_transpose_from_the_matrix():
    """The joints' scales differ per axis by a factor of 1.5 or more somewhere, and the normals through mat3(M) point
    elsewhere than the rule's: by more than 5 degrees for most vertices."""
    c = sc.case("scaled_joint")
    m, pal = c.scene0.meshes[0], c.poses[0][0]
    lin = pal.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    sv = np.linalg.svd(lin, compute_uv=False)
    assert (sv[:, 0] / sv[:, 2]).max() > 1.5
    _, good = sn.skin(m.positions, m.normals, m.skin.joint_indices, m.skin.joint_weights, pal)
    _, bad = sn.skin(m.positions, m.normals, m.skin.joint_indices, m.skin.joint_weights, pal, wrong="mat3")
    unit = lambda a: a / np.linalg.norm(a, axis=1)[:, None]  # noqa: E731
    cos = (unit(good.astype(np.float64)) * unit(bad.astype(np.float64))).sum(axis=1)
    assert (cos < np.cos(np.radians(5.0))).mean() > 0.5


def test_flat_zero_holds_zeros_of_both_signs_up_to_the_mesh_bounds():
    """Every posed z is a zero, of both signs; triangles hold both; and the posed Aabb's z follows the LAST vertex's
    sign (-0: min = max = -0, centre -0, half extent +0) where a sign-blind minimum and maximum would centre on +0."""
    from hikari_amd import skin_vertices
    c = sc.case("flat_zero")
    posed_mesh, box = skin_vertices(c.scene0.meshes[0], c.poses[0][0], aabb=True)
    z = posed_mesh.positions[:, 2]
    neg = np.signbit(z)
    assert (z == 0.0).all() and neg.any() and not neg.all() and neg[-1]
    assert same_words(box, sn.bounds(posed_mesh.positions))
    assert box.view(np.uint32)[[2, 5]].tolist() == [0x80000000, 0]
    tri = neg[posed_mesh.indices.reshape(-1, 3)]
    assert (tri.any(axis=1) & ~tri.all(axis=1)).sum() >= 4
    _, d1 = sc.posed("flat_zero")
    nodes = mc.mesh_nodes(d1, c.scene0.mesh_index(0))
    inner = nodes[nodes["entry"] < 0x80000000]
    zb = np.concatenate([inner["min"][:, 2], inner["max"][:, 2]])
    assert (zb == 0.0).all() and np.signbit(zb).any() and not np.signbit(zb).all()
    # the sign reaches the instance record: its world centre's z from the rule's cz and from a sign-blind +0
    f = np.float32
    m = c.scene0.instance_models()[0]
    assert box[0] > 0 and box[1] > 0 and m.view(np.uint32)[[2, 6, 14]].tolist() == [0x80000000] * 3 and m[10] == -1.0

    def world_z(cz):
        return f(f(f(m[2] * box[0]) + f(m[6] * box[1])) + f(m[10] * cz)) + m[14]
    assert f(world_z(box[2])).view(np.uint32) == 0 and f(world_z(f(0.0))).view(np.uint32) == 0x80000000
    rec = np.frombuffer(host_scene_array(d1, 4, np.dtype((np.void, 176))).tobytes(), np.uint32).reshape(-1, 44)[0]
    assert rec[2] == 0 and rec[6] == 0  # min.z, max.z: -0 + (+0); with the sign-blind centre they would be -0


def test_keep_normals_keeps_them():
    c = sc.case("keep_normals")
    assert c.keep_normals == (0,)
    s1, d1 = sc.posed("keep_normals")
    assert s1.meshes[0].normals.tobytes() == c.scene0.meshes[0].normals.tobytes()
    assert (s1.meshes[0].normals != np.array([0, 0, 1], np.float32)).any()
    assert s1.meshes[0].positions.tobytes() != c.scene0.meshes[0].positions.tobytes()


def test_frame_cases_are_in_view():
    """The camera of the frame cases sees the posed meshes: their instances' boxes project inside the 32 x 24 frame."""
    for name in sc.FRAME_CASES:
        _, d1 = sc.posed(name)
        cam, _ = sc.camera_for(name)
        w, h = sc.FRAME_SIZE
        vp = np.array(cam.view(w, h).view_proj, np.float64).reshape(4, 4).T
        inst = np.frombuffer(host_scene_array(d1, 4, np.dtype((np.void, 176))).tobytes(), np.float32).reshape(-1, 44)
        centre = 0.5 * (inst[0, 0:3] + inst[0, 4:7]).astype(np.float64)
        clip = vp @ np.append(centre, 1.0)
        assert clip[3] > 0 and abs(clip[0] / clip[3]) < 1 and abs(clip[1] / clip[3]) < 1, name
