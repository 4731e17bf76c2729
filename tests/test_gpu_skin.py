"""hk_set_mesh_skins / hk_skin_meshes at their size and shape edges: the cases of tests/skin_cases.py (each proven to sit
on its edge by tests/test_skin_cases.py, without a GPU) uploaded in their bind pose, their skins registered, posed on the
device, and all nine arrays compared byte for byte with the host builder's for Scene.posed(...): the scene whose posed
meshes hold hks_skin_vertices' output (itself held to tests/skin_numpy.py by tests/test_skin_independent.py).  Frames,
traced rays and counters against the CPU oracle on that host scene.

What each case exists for in csrc/hk_dynamic.hip:
  verts_3 .. verts_65          k_skin_vertices' last wave partly filled / full / one lane into the next
  verts_256 / verts_257        one / two workgroups of k_skin_vertices, one / two strides of k_skin_bounds' loop
  tris_1281                    k_build_mesh_bvh<false> (global memory) fed from the staged streams the device wrote
  many_skins                   12 meshes in one call: the table search, palettes at offsets 0, 1, 3, 10, 266, ..., index 255
  one_of_three                 an unposed skinned mesh and an unskinned mesh keep their bytes
  shared_mesh                  k_skin_bounds writes all five instances' rows
  emissive_skin                areas, alias table, surface_area and the light BVH follow the posed triangles
  scaled_joint                 the inverse transpose in the normals
  flat_zero                    zeros of both signs in shape boxes, sibling boxes and the posed Aabb
  keep_normals                 normals = NULL: MeshUpdate::has_normals = 0 on the device path
The caller's local_aabbs rows of a posed mesh's instances are filled with a wrong box in every test: they are ignored.
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.
"""
import ctypes

import numpy as np
import pytest

import mesh_cases as mc
import skin_cases as sc
from parity import host_scene_array, renderer
from scene_edits import (INST_DT, EditFrames, assert_mesh_rebuild_bitwise, assert_slices_kept,
                         assert_traces_equal_fresh, caller_stream, models_and_aabbs, ptr, raw_call, raw_renderer)
from skin_cases import caller_aabbs

pytestmark = pytest.mark.gpu


def _register(r, name, stream=None):
    c = sc.case(name)
    r.set_mesh_skins(c.scene0, c.skinned, c.keep_normals, stream=stream)


def _pose(r, name, k=0, stream=None, **kw):
    c = sc.case(name)
    pose = c.poses[k]
    kw.setdefault("local_aabbs", caller_aabbs(c.scene0, set(pose)))
    r.skin_meshes(c.scene0, pose, stream=stream, **kw)


def _posed_renderer(name, size=None, **kw):
    r = renderer(sc.case(name).scene0, size, **kw)
    _register(r, name)
    _pose(r, name)
    return r


@pytest.mark.parametrize("name", list(sc.CASES))
def test_posed_arrays_match_host_builder(name):
    """Upload the bind pose, register, pose: every array equals the host builder's for the posed scene, the BLAS
    topology included.  one_of_three: the unposed meshes' slices also equal the bind pose's."""
    c = sc.case(name)
    r = _posed_renderer(name)
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    if name == "one_of_three":
        assert_slices_kept(r, c.scene0, (0, 2))
    r.close()


@pytest.mark.parametrize("name", sc.SECOND_POSE_CASES)
def test_second_pose_on_dirty_scratch(name):
    """Another pose from the same bind pose: the staged streams, palettes, shape boxes, index buffers and segment lists
    are reused as the first pose left them."""
    r = _posed_renderer(name)
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    _pose(r, name, 1)
    assert_mesh_rebuild_bitwise(r, sc.posed(name, 1)[1])
    r.close()


def test_pose_then_update_back_then_pose_again():
    """hk_update_meshes with the bind pose from the host puts the arrays back; the resident streams are untouched by it,
    and the same pose gives the same arrays again."""
    name = "verts_257"
    c = sc.case(name)
    r = _posed_renderer(name)
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    r.update_meshes(c.scene0, c.skinned, local_aabbs=mc.local_aabbs(c.scene0))
    assert_mesh_rebuild_bitwise(r, c.scene0.desc)
    _pose(r, name)
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    r.close()


def _rerigged(scene, i, joints, seed):
    """A copy of the scene whose mesh i carries another seeded rig of `joints` joints, and a palette for it."""
    from hikari_amd import Mesh, Scene
    rng = np.random.default_rng([sc.SEED, seed])
    m = scene.meshes[i]
    s = Scene()
    s.meshes = list(scene.meshes)
    s.meshes[i] = sc.rig(Mesh(m.positions, m.normals, m.uvs, m.indices, m.topology), rng, joints)
    s.materials, s.instances = scene.materials, scene.instances
    return s, sc.palette(rng, joints, sc.cell_of(m))


def test_registering_again_with_another_rig():
    """The same mesh with other indices, weights and joint count, then a smaller set than before (capacity beside
    size): each registration replaces the whole set."""
    name = "many_skins"
    c = sc.case(name)
    r = _posed_renderer(name)
    other, pal = _rerigged(c.scene0, 3, 9, 1)
    r.set_mesh_skins(other, [3])
    # the other eleven stay as the first pose left them (their boxes are the caller's now: the posed ones); mesh 3 is
    # the new rig's pose of the bind pose
    host = sc.posed(name)[0].posed({})
    host.meshes[3] = other.posed({3: pal}).meshes[3]
    r.skin_meshes(other, {3: pal}, local_aabbs=caller_aabbs(host, {3}))
    assert_mesh_rebuild_bitwise(r, host.build())
    from hikari_amd import HikariError
    with pytest.raises(HikariError, match="no registered skin"):
        r.skin_meshes(c.scene0, {0: c.poses[0][0]}, local_aabbs=caller_aabbs(c.scene0, {0}))
    r.close()


def test_add_meshes_keeps_the_skins_and_set_meshes_and_upload_drop_them():
    from hikari_amd import HikariError, plane_mesh
    name = "one_of_three"
    c = sc.case(name)
    s0 = c.scene0
    r = renderer(s0)
    _register(r, name)
    r.add_meshes([plane_mesh(0.3)])
    _pose(r, name)
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1], longer=True)
    # the same list again, the appended mesh left out: the slices stay where they are, and the set is dropped all the same
    entries = [(s0.mesh_index(i), len(s0.meshes[i].positions)) for i in range(len(s0.meshes))]
    posed_scene = sc.posed(name)[0]
    r.set_meshes(posed_scene, entries, previous=list(range(len(s0.instances))), local_aabbs=mc.local_aabbs(posed_scene))
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    for again in ("set_meshes", "upload"):
        if again == "upload":
            r.upload_scene(s0)
        with pytest.raises(HikariError, match="no registered skin"):
            _pose(r, name)
        assert_mesh_rebuild_bitwise(r, sc.posed(name)[1] if again == "set_meshes" else s0.desc)
        _register(r, name)
        _pose(r, name)
        assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    r.close()


def _frames(name, options=None, wavefront=False):
    d1 = sc.posed(name)[1]
    with EditFrames(sc.case(name).scene0, sc.camera_for(name), sc.FRAME_SIZE, floor=0.1, finite=True, options=options,
                     wavefront=wavefront) as fr:
        _register(fr.r, name)
        _pose(fr.r, name)
        assert_mesh_rebuild_bitwise(fr.r, d1)
        fr.set_scene(d1)
        fr.frames(2)


@pytest.mark.parametrize("name", sc.FRAME_CASES)
def test_frames_after_a_pose_match_oracle(name):
    """Two 32 x 24 frames against the oracle on the posed host scene (the oracle sees the bind pose, then the posed
    scene; one thread, spatial reuse off, the racy scatter targets within their tolerance) and the ray counters."""
    _frames(name)


def test_frames_with_the_scene_staged_in_lds():
    _frames("scaled_joint", {"lds_scene": 1})


def test_frames_with_the_wavefront_pass():
    _frames("emissive_skin", wavefront=True)


def test_traced_rays_after_a_pose_equal_a_fresh_context():
    """256 seeded rays through hk_trace after the pose, against a context that uploaded the posed scene."""
    name = "shared_mesh"
    c = sc.case(name)
    s1 = sc.posed(name)[0]
    r = _posed_renderer(name, sc.FRAME_SIZE)
    fresh = renderer(s1, sc.FRAME_SIZE)
    assert_traces_equal_fresh(r, fresh, sc.SEED, len(s1.instances))
    fresh.close()
    r.close()


# ------------------------------------------------------------------ refusals
def _index(scene, i, index=None):
    from hikari_amd import _abi
    v, pr, n0, nc = scene.mesh_index(i) if index is None else index
    return _abi.hk_mesh_index(v, pr, (ctypes.c_uint32 * 2)(n0, nc))


def _raw_skins(r, skins, n=None):
    from hikari_amd import _abi
    arr = (_abi.hk_mesh_skin * max(1, len(skins)))(*skins) if skins is not None else None
    return raw_call(r, "hk_set_mesh_skins", arr, (0 if skins is None else len(skins)) if n is None else n, None)


def _raw_pose(r, scene, poses, n=None, count=None, models=True, aabbs=True):
    from hikari_amd import _abi
    m, a = models_and_aabbs(scene)
    arr = (_abi.hk_skin_pose * max(1, len(poses)))(*poses) if poses is not None else None
    return raw_call(r, "hk_skin_meshes", arr, (0 if poses is None else len(poses)) if n is None else n, ptr(m, models),
                    ptr(a, aabbs), len(m) if count is None else count, None)


def test_refusals_leave_the_context_and_the_skin_set_as_they_were():
    """Every refusal in the two headers' comments returns its code with a message; nothing changed: the arrays still
    equal the bind pose's, and the skin set registered before is still the one a pose then uses."""
    from hikari_amd import HikariRenderer, _abi
    name = "one_of_three"
    c = sc.case(name)
    s0 = c.scene0
    keep = []

    def skin(i, vertex_count=None, index=None, joint_count=None, null=None, bad_index=None):
        m = s0.meshes[i]
        p = np.ascontiguousarray(m.positions, np.float32)
        nr = np.ascontiguousarray(m.normals, np.float32)
        ix = np.ascontiguousarray(m.skin.joint_indices, np.uint16).copy()
        w = np.ascontiguousarray(m.skin.joint_weights, np.float32)
        if bad_index is not None:
            ix[-1, 3] = bad_index
        keep.extend([p, nr, ix, w])
        ptr = {"positions": p.ctypes.data, "normals": nr.ctypes.data, "joint_indices": ix.ctypes.data,
               "joint_weights": w.ctypes.data}
        if null:
            ptr[null] = None
        return _abi.hk_mesh_skin(_index(s0, i, index), len(p) if vertex_count is None else vertex_count, ptr["positions"],
                                 ptr["normals"], ptr["joint_indices"], ptr["joint_weights"],
                                 m.skin.joint_count if joint_count is None else joint_count)

    def pose(i, joints=None, joint_count=None, null=False):
        j = np.ascontiguousarray(c.poses[0][1] if joints is None else joints, np.float32)
        keep.append(j)
        return _abi.hk_skin_pose(_index(s0, i), None if null else j.ctypes.data, len(j) if joint_count is None else joint_count)

    empty = HikariRenderer(0)
    rc, msg = _raw_skins(empty, [skin(1)])
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    rc, msg = _raw_pose(empty, s0, [pose(1)])
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()

    r = renderer(s0)
    _register(r, name)
    v, pr, n0, nc = s0.mesh_index(1)
    nv = len(s0.meshes[1].positions)
    top = int(s0.meshes[1].indices.max())
    refused_skins = [
        ("null list", dict(skins=None, n=1), "null"),
        ("null positions", dict(skins=[skin(1, null="positions")]), "null pointer"),
        ("null indices", dict(skins=[skin(1, null="joint_indices")]), "null pointer"),
        ("null weights", dict(skins=[skin(1, null="joint_weights")]), "null pointer"),
        ("not a mesh: vertex", dict(skins=[skin(1, index=(v + 1, pr, n0, nc))]), "not a known mesh slice"),
        ("not a mesh: node", dict(skins=[skin(1, index=(v, pr, n0 + 3, nc - 3))]), "not a known mesh slice"),
        ("too few vertices", dict(skins=[skin(1, vertex_count=top)]), "vertex indices"),
        ("into the next mesh", dict(skins=[skin(1, vertex_count=nv + 1)]), "past its vertex slice"),
        ("no joints", dict(skins=[skin(1, joint_count=0)]), "joint_count is outside"),
        ("too many joints", dict(skins=[skin(1, joint_count=65537)]), "joint_count is outside"),
        ("index == joint_count", dict(skins=[skin(1, bad_index=5)]), ">= joint_count"),
        ("twice", dict(skins=[skin(1), skin(0), skin(1)]), "listed twice"),
    ]
    for label, kw, text in refused_skins:
        rc, msg = _raw_skins(r, **kw)
        assert rc == _abi.HK_ERR_INVALID and text in msg, (label, rc, msg)
    other = sc.palette(np.random.default_rng(sc.SEED), 3, 0.1)
    refused_poses = [
        ("null list", dict(poses=None, n=1), "null"),
        ("null joints", dict(poses=[pose(1, null=True)]), "null pointer"),
        ("null models", dict(poses=[pose(1)], models=False), "null"),
        ("null aabbs", dict(poses=[pose(1)], aabbs=False), "null"),
        ("count", dict(poses=[pose(1)], count=len(s0.instances) - 1), "every instance"),
        ("no skin", dict(poses=[pose(2)]), "no registered skin"),
        ("joint count", dict(poses=[pose(1, joint_count=4)]), "differs from the registered skin's"),
        ("twice", dict(poses=[pose(1), pose(0, joints=other), pose(1)]), "poses a mesh twice"),
    ]
    for label, kw, text in refused_poses:
        rc, msg = _raw_pose(r, s0, **kw)
        assert rc == _abi.HK_ERR_INVALID and text in msg, (label, rc, msg)
        assert_mesh_rebuild_bitwise(r, s0.desc)
    # n == 0 is hk_update_instances
    rc, msg = _raw_pose(r, s0, [], n=0)
    assert rc == 0, msg
    assert_mesh_rebuild_bitwise(r, s0.desc)
    # the set registered before the refusals is still there
    _pose(r, name)
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    # an empty list drops it
    rc, msg = _raw_skins(r, [], n=0)
    assert rc == 0, msg
    rc, msg = _raw_pose(r, s0, [pose(1)])
    assert rc == _abi.HK_ERR_INVALID and "no registered skin" in msg
    r.close()


def test_a_mesh_whose_nodes_are_not_3k_minus_2_cannot_be_skinned():
    """A scene uploaded with a mesh slice of one node less than 3k - 2: its skin is refused, another mesh's is taken."""
    from hikari_amd import _abi
    c = sc.case("one_of_three")
    s0 = c.scene0
    d0 = s0.desc
    inst = np.frombuffer(host_scene_array(d0, 4, INST_DT).tobytes(), np.uint32).reshape(-1, 44).copy()
    v, pr, n0, nc = s0.mesh_index(1)
    assert inst[1, 40:44].tolist() == [v, pr, n0, nc]
    inst[1, 43] = nc - 1
    desc = _abi.hk_scene_desc.from_buffer_copy(d0)
    desc.instances.data = inst.ctypes.data
    r = raw_renderer(desc)
    m = s0.meshes[1]
    p, ix = np.ascontiguousarray(m.positions, np.float32), np.ascontiguousarray(m.skin.joint_indices, np.uint16)
    w = np.ascontiguousarray(m.skin.joint_weights, np.float32)
    bad = _abi.hk_mesh_skin(_index(s0, 1, (v, pr, n0, nc - 1)), len(p), p.ctypes.data, None, ix.ctypes.data,
                            w.ctypes.data, m.skin.joint_count)
    rc, msg = _raw_skins(r, [bad])
    assert rc == _abi.HK_ERR_INVALID and "3k - 2" in msg, (rc, msg)
    r.set_mesh_skins(s0, [0])
    r.close()


def test_a_singular_model_fails_after_the_rebuild():
    from hikari_amd import HikariError
    name = "verts_65"
    c = sc.case(name)
    r = renderer(c.scene0)
    _register(r, name)
    models = c.scene0.instance_models().copy()
    models[0, 4:8] = 0.0  # a zero column
    with pytest.raises(HikariError, match="singular instance transform"):
        _pose(r, name, models=models)
    _pose(r, name)
    assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
    r.close()


def test_pose_on_a_caller_stream():
    """tris_1281 registered and posed on a stream of the caller's (scene_edits.caller_stream): both calls wait for their
    stream once, so the arrays are complete when hk_skin_meshes returns; the test synchronises the stream all the same."""
    name = "tris_1281"
    r = renderer(sc.case(name).scene0)
    with caller_stream() as (s, sync):
        _register(r, name, stream=s)
        _pose(r, name, stream=s)
        sync()
        assert_mesh_rebuild_bitwise(r, sc.posed(name)[1])
        r.close()


def test_kernel_timing_names_the_pose():
    name = "verts_64"
    r = renderer(sc.case(name).scene0)
    _register(r, name)
    r.enable_kernel_timing(True)
    _pose(r, name)
    r.sync()
    assert "skin_meshes" in r.kernel_timing()
    r.close()


def test_plugin_forwards_both_calls():
    from hikari_amd import HikariPlugin
    name = "keep_normals"
    c = sc.case(name)
    p = HikariPlugin(c.scene0)
    p.set_mesh_skins(c.scene0, c.skinned, c.keep_normals)
    p.skin_meshes(c.scene0, c.poses[0], local_aabbs=caller_aabbs(c.scene0, set(c.poses[0])))
    assert_mesh_rebuild_bitwise(p.renderer, sc.posed(name)[1])
    p.renderer.close()
