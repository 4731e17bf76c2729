"""The morph cases (tests/morph_cases.py) on the CPU: the host builder and hks_morph_vertices alone confirm that every case
sits where its name says (vertex, triangle, target and active counts, which meshes keep their bytes, zeros of both
signs, the normals that stay, the skin under the morph), that every posed vertex is finite, that a posed mesh's BLAS is
another tree than the base's (so a refit that kept the tree would fail the GPU test), that morphing moves the emitters'
areas, and that Scene.morphed holds the words tests/morph_numpy.py (and tests/skin_numpy.py after it) says it should.
tests/test_gpu_morph.py runs the same cases through hk_set_mesh_morphs and hk_morph_meshes."""
import re
from pathlib import Path

import numpy as np
import pytest

import mesh_cases as mc
import morph_cases as mo
import morph_numpy as mn
import skin_numpy as sn
from parity import NODE_DT, host_scene_array
from test_mesh_cases import PRIM_DT, VERTEX_DT
from test_skin_independent import same_words

ROOT = Path(__file__).resolve().parent.parent


def _slices(scene, i):
    v, p, n0, nc = scene.mesh_index(i)
    return v, len(scene.meshes[i].positions), p, (nc + 2) // 3, n0, nc


def test_every_case_is_listed_and_the_edges_are_the_kernels():
    names = [f"verts_{n}" for n in (3, 63, 64, 65, 256, 257)] + [f"active_{k}" for k in (0, 1, mo.B - 1, mo.B, mo.B + 1)]
    names += ["targets_256", "tris_1281", "many_morphs", "one_of_three", "shared_mesh", "emissive_morph", "flat_zero",
              "keep_normals", "no_normal_deltas", "skin_65", "skin_scaled"]
    assert sorted(names) == sorted(mo.CASES)
    assert set(mo.SECOND_POSE_CASES) | set(mo.FRAME_CASES) | set(mo.REFIT_CASES) <= set(mo.CASES)
    assert all(len(mo.case(n).poses) == 2 for n in mo.SECOND_POSE_CASES)
    launch = (ROOT / "bevy-hikari_amd" / "csrc" / "hk_launch.h").read_text()
    assert int(re.search(r"constexpr int MORPH_BATCH = (\d+);", launch).group(1)) == mo.B
    src = (ROOT / "bevy-hikari_amd" / "csrc" / "hk_dynamic.hip").read_text()
    for text in ("BVH_LDS_SHAPES = 1280;", "k_morph_vertices", "k_skin_bounds", "b += (uint32_t)MORPH_BATCH", "morph_batch<MORPH_BATCH, true>"):
        assert text in src, text
    assert re.search(r"__launch_bounds__\(256\) void k_morph_vertices", src)
    header = (ROOT / "include" / "hk_morph.h").read_text()
    assert "#define HK_MORPH_MAX_TARGETS 256u" in header


@pytest.mark.parametrize("name", list(mo.CASES))
def test_posed_scenes_share_topology_and_hold_the_host_morph(name):
    """The posed scene: the base's slices, vertex indices, uvs, instances and materials; a posed mesh's positions and
    normals are the restatements' words, finite, and (but for active_0) differ from the base; every other mesh's vertex
    and primitive bytes are the base's."""
    c = mo.case(name)
    d0 = c.scene0.desc
    v0, p0 = host_scene_array(d0, 0, VERTEX_DT), host_scene_array(d0, 1, PRIM_DT)
    for k, pose in enumerate(c.poses):
        s1, d1 = mo.posed(name, k)
        assert mc.mesh_slices(d0) == mc.mesh_slices(d1)
        v1, p1 = host_scene_array(d1, 0, VERTEX_DT), host_scene_array(d1, 1, PRIM_DT)
        assert np.array_equal(p0["v"]["index"], p1["v"]["index"])
        assert v0["u"].tobytes() == v1["u"].tobytes() and v0["v"].tobytes() == v1["v"].tobytes()
        assert set(pose) <= set(c.morphed)
        for i, m in enumerate(c.scene0.meshes):
            v, nv, p, nt, _, _ = _slices(c.scene0, i)
            if i not in pose:
                assert v0[v: v + nv].tobytes() == v1[v: v + nv].tobytes(), i
                assert p0[p: p + nt].tobytes() == p1[p: p + nt].tobytes(), i
                continue
            w, joints = mo.parts(pose[i])
            keep = i in c.keep_normals
            assert len(w) == m.morph.target_count == len(m.morph.position_deltas)
            want_p, want_n = mn.morph(m.positions, None if keep else m.normals, m.morph.position_deltas,
                                      None if keep else m.morph.normal_deltas, w)
            assert (joints is not None) == (i in c.skinned)
            if joints is not None:
                assert len(joints) == m.skin.joint_count
                alone = want_p
                want_p, want_n = sn.skin(want_p, want_n, m.skin.joint_indices, m.skin.joint_weights, joints)
                assert not same_words(alone, want_p)
                assert not same_words(want_p, sn.skin(m.positions, None, m.skin.joint_indices, m.skin.joint_weights,
                                                      joints)[0])
            got_p, got_n = v1["position"][v: v + nv], v1["normal"][v: v + nv]
            assert same_words(got_p, want_p), i
            assert same_words(got_n, m.normals if keep else want_n), i
            assert np.isfinite(got_p).all() and np.isfinite(got_n).all()
            moved = v0["position"][v: v + nv].tobytes() != got_p.tobytes()
            assert moved == bool(mo.active_of(w) or joints is not None), i


@pytest.mark.parametrize("n", mo.VERTEX_SIZES)
def test_vertex_counts_sit_on_the_wave_and_workgroup_edges(n):
    c = mo.case(f"verts_{n}")
    assert _slices(c.scene0, 0)[:4] == (0, n, 0, n - 2)
    assert all(len(mo.active_of(p[0])) == 3 for p in c.poses)


@pytest.mark.parametrize("k", mo.ACTIVE_COUNTS)
def test_active_counts_sit_on_the_batch_edges(k):
    """The active list's length against the kernel's batch B: none, one, a batch less one, a whole batch, one into the
    next; the skipped weights are zeros of both signs."""
    c = mo.case(f"active_{k}")
    w = c.poses[0][0]
    on = mo.active_of(w)
    assert len(w) == mo.ACTIVE_TARGETS and len(on) == k and on == sorted(on)
    off = np.delete(w, on).view(np.uint32)
    assert (off == 0).any() and (off == 0x80000000).any()
    assert sorted(mo.ACTIVE_COUNTS) == [0, 1, mo.B - 1, mo.B, mo.B + 1]
    if k == 0:
        assert host_scene_array(mo.posed("active_0")[1], 0, VERTEX_DT).tobytes() == \
            host_scene_array(c.scene0.desc, 0, VERTEX_DT).tobytes()


def test_256_targets_with_three_active_one_of_them_the_last():
    c = mo.case("targets_256")
    w = c.poses[0][0]
    assert len(w) == 256 and c.scene0.meshes[0].morph.target_count == 256
    assert mo.active_of(w) == [9, 130, 255]


def test_the_big_mesh_takes_the_global_memory_build():
    c = mo.case("tris_1281")
    _, nv, _, nt, _, nc = _slices(c.scene0, 0)
    assert nt == mo.BVH_LDS_SHAPES + 1 and nc == 3 * nt - 2 and nv > 256


def test_many_morphs_cover_the_table_search_and_delta_offsets():
    """12 meshes posed in one call; target counts 1, 2, 7 and 16 in turn and vertex counts on both sides of a workgroup,
    so the delta blocks and the active ranges start at offsets that are no multiple of anything; every third mesh has
    no normal deltas, so the two delta streams' offsets differ."""
    c = mo.case("many_morphs")
    assert len(c.morphed) == 12 and all(set(p) == set(range(12)) for p in c.poses)
    assert [c.scene0.meshes[i].morph.target_count for i in range(12)] == [1, 2, 7, 16] * 3
    nv = [len(c.scene0.meshes[i].positions) for i in range(12)]
    assert min(nv) < 64 and max(nv) > 256 and len(set(nv)) > 8
    assert [(_slices(c.scene0, i)[3]) for i in range(12)] == mo.MANY_TRIS
    assert [c.scene0.meshes[i].morph.normal_deltas is None for i in range(12)] == [k % 3 == 1 for k in range(12)]
    counts = {len(mo.active_of(p[i])) for p in c.poses for i in range(12)}
    assert len(counts) >= 4 and max(counts) > mo.B


SAME_TREE = ("verts_3", "active_0")  # one triangle has one tree; no active target leaves the base where it is


@pytest.mark.parametrize("name", [n for n in mo.CASES if n not in SAME_TREE])
def test_the_posed_tree_is_another_tree(name):
    """The posed meshes' entry / exit words differ between the base's and the posed scene's host builds.  (many_morphs'
    meshes under 8 triangles are left out.)"""
    c = mo.case(name)
    for k, pose in enumerate(c.poses):
        _, d1 = mo.posed(name, k)
        for i in pose:
            index = c.scene0.mesh_index(i)
            if name == "many_morphs" and (index[3] + 2) // 3 < 8:
                continue
            a, b = mc.mesh_nodes(c.scene0.desc, index), mc.mesh_nodes(d1, index)
            assert not (np.array_equal(a["entry"], b["entry"]) and np.array_equal(a["exit"], b["exit"])), (k, i)


def test_one_of_three_leaves_a_morphed_and_an_unmorphed_mesh_alone():
    c = mo.case("one_of_three")
    assert c.morphed == [0, 1] and [set(p) for p in c.poses] == [{1}]
    assert c.scene0.meshes[0].morph is not None and c.scene0.meshes[2].morph is None
    _, d1 = mo.posed("one_of_three")
    n0, n1 = host_scene_array(c.scene0.desc, 2, NODE_DT), host_scene_array(d1, 2, NODE_DT)
    for i in (0, 2):
        a, b = _slices(c.scene0, i)[4:]
        assert n0[a: a + b].tobytes() == n1[a: a + b].tobytes()


def test_shared_mesh_has_five_instances_of_the_posed_mesh():
    c = mo.case("shared_mesh")
    assert [m for m, _, _ in c.scene0.instances][:5] == [0] * 5
    a0, a1 = mc.local_aabbs(c.scene0), mc.local_aabbs(mo.posed("shared_mesh")[0])
    assert all(a0[i].tobytes() != a1[i].tobytes() for i in range(5))


def test_the_morphed_emitter_moves_areas_alias_table_and_light_bvh():
    c = mo.case("emissive_morph")
    d0, d1 = c.scene0.desc, mo.posed("emissive_morph")[1]
    assert d0.emissives.count == d1.emissives.count >= 2
    for idx, dt in ((3, np.dtype((np.void, 8))), (8, np.dtype((np.void, 64))), (7, NODE_DT)):
        assert host_scene_array(d0, idx, dt).tobytes() != host_scene_array(d1, idx, dt).tobytes(), idx


def test_flat_zero_holds_zeros_of_both_signs():
    c = mo.case("flat_zero")
    s1, d1 = mo.posed("flat_zero")
    z = np.ascontiguousarray(s1.meshes[0].positions[:, 2])
    assert (z == 0.0).all() and np.signbit(z).any() and not np.signbit(z).all()
    assert (np.asarray(c.poses[0][0]) > 0).all()
    dz = c.scene0.meshes[0].morph.position_deltas[:, :, 2]
    assert (dz.view(np.uint32) == 0x80000000).all()
    # the rule's sign (the last vertex's zero) is not what a sign-blind fold from +0 would give for both bounds
    box = sn.bounds(s1.meshes[0].positions)
    assert box[2] == 0.0 and box[5] == 0.0
    assert np.signbit(box[2]) == np.signbit(z[-1])
    assert (s1.meshes[0].positions[:, :2] > 0).all()


def test_keep_normals_and_no_normal_deltas_leave_the_normals():
    for name in ("keep_normals", "no_normal_deltas"):
        c = mo.case(name)
        s1, _ = mo.posed(name)
        assert np.asarray(s1.meshes[0].normals, np.float32).tobytes() == \
            np.asarray(c.scene0.meshes[0].normals, np.float32).tobytes(), name
        assert np.asarray(s1.meshes[0].positions).tobytes() != np.asarray(c.scene0.meshes[0].positions).tobytes()
    assert mo.case("keep_normals").keep_normals == (0,) and mo.case("keep_normals").scene0.meshes[0].morph.normal_deltas is not None
    assert mo.case("no_normal_deltas").keep_normals == () and mo.case("no_normal_deltas").scene0.meshes[0].morph.normal_deltas is None


def test_the_skin_cases_morph_under_a_skin():
    c = mo.case("skin_65")
    assert len(c.scene0.meshes[0].positions) == 65 and c.skinned == [0]
    assert all(len(mo.active_of(p[0][0])) == mo.B for p in c.poses)
    c = mo.case("skin_scaled")
    _, joints = c.poses[0][0]
    scales = [np.linalg.svd(j.reshape(4, 4).T[:3, :3].astype(np.float64), compute_uv=False) for j in joints]
    assert max(s[0] / s[2] for s in scales) > 1.5


def test_scene_morphed_carries_the_morph_and_the_skin_along():
    c = mo.case("skin_65")
    s1, _ = mo.posed("skin_65")
    assert s1.meshes[0].morph is c.scene0.meshes[0].morph and s1.meshes[0].skin is c.scene0.meshes[0].skin
    again = s1.posed({}).meshes[0]
    assert again.morph is c.scene0.meshes[0].morph
