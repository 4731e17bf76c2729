"""hk_set_mesh_morphs / hk_morph_meshes at their size and shape edges: the cases of tests/morph_cases.py (each proven to
sit on its edge by tests/test_morph_cases.py, without a GPU) uploaded as their base, their morphs (and skins) registered,
posed on the device, and all nine arrays compared byte for byte with the host builder's for Scene.morphed(...): the scene
whose posed meshes hold hks_morph_vertices' output, passed through hks_skin_vertices where the pose gives joints (both
held to their numpy restatements by tests/test_morph_independent.py).  The two refits against Scene.refitted and
Scene.refitted_instances over that scene; frames and counters against the CPU oracle on it.

What each case exists for in csrc/hk_dynamic.hip:
  verts_3 .. verts_65          k_morph_vertices' last wave partly filled / full / one lane into the next
  verts_256 / verts_257        one / two workgroups of k_morph_vertices, one / two strides of k_skin_bounds' loop
  active_0 .. active_B+1       no trip, a partial batch, B - 1, a whole batch, a whole batch and one more
  targets_256                  the largest target index in the delta offset
  tris_1281                    k_build_mesh_bvh<false> (global memory) fed from the staged streams the device wrote
  many_morphs                  12 meshes in one call: the table search, the delta offsets of both streams, the active ranges
  one_of_three                 an unposed morphed mesh and an unmorphed mesh keep their bytes
  shared_mesh                  k_skin_bounds writes all five instances' rows (its slices from the MorphSource table)
  emissive_morph               areas, alias table, surface_area and the light BVH follow the posed triangles
  flat_zero                    zeros of both signs in shape boxes, sibling boxes and the posed Aabb
  keep_normals                 normals = NULL: MeshUpdate::has_normals = 0 on the device path
  no_normal_deltas             normal_deltas = NULL: the base normals copied
  skin_65 / skin_scaled        skin_vertex after the fold, the palettes beside the active list
The caller's local_aabbs rows of a posed mesh's instances are filled with a wrong box in every test: they are ignored.
The shared checks (arrays, frames, stream, raw calls) are tests/scene_edits.py's.
"""
import ctypes

import numpy as np
import pytest

import mesh_cases as mc
import morph_cases as mo
import skin_cases as sc
from morph_cases import caller_aabbs
from parity import renderer
from scene_edits import (EditFrames, assert_mesh_rebuild_bitwise, assert_scene_is, assert_slices_kept, caller_stream,
                         device_arrays, models_and_aabbs, ptr, raw_call)

pytestmark = pytest.mark.gpu


def _register(r, name, stream=None):
    c = mo.case(name)
    r.set_mesh_morphs(c.scene0, c.morphed, c.keep_normals, stream=stream)
    if c.skinned:
        r.set_mesh_skins(c.scene0, c.skinned, c.keep_normals, stream=stream)


def _pose(r, name, k=0, stream=None, **kw):
    c = mo.case(name)
    pose = c.poses[k]
    kw.setdefault("local_aabbs", caller_aabbs(c.scene0, set(pose)))
    r.morph_meshes(c.scene0, pose, stream=stream, **kw)


def _posed_renderer(name, size=None, **kw):
    r = renderer(mo.case(name).scene0, size, **kw)
    _register(r, name)
    _pose(r, name)
    return r


@pytest.mark.parametrize("name", list(mo.CASES))
def test_posed_arrays_match_host_builder(name):
    """Upload the base, register, pose: every array and count equals the host builder's for the morphed scene, the BLAS
    topology included.  one_of_three: the unposed meshes' slices also equal the base's."""
    c = mo.case(name)
    r = _posed_renderer(name)
    assert_mesh_rebuild_bitwise(r, mo.posed(name)[1])
    assert_scene_is(r, mo.posed(name)[1])
    if name == "one_of_three":
        assert_slices_kept(r, c.scene0, (0, 2))
    r.close()


@pytest.mark.parametrize("name", mo.SECOND_POSE_CASES)
def test_second_pose_on_dirty_scratch(name):
    """Another pose from the same base: the staged streams, palettes, active list, shape boxes, index buffers and
    segment lists are reused as the first pose left them."""
    r = _posed_renderer(name)
    assert_mesh_rebuild_bitwise(r, mo.posed(name)[1])
    _pose(r, name, 1)
    assert_mesh_rebuild_bitwise(r, mo.posed(name, 1)[1])
    r.close()


@pytest.mark.parametrize("name", mo.REFIT_CASES)
def test_the_two_refits(name):
    """refit=True: the arrays are Scene.refitted(base desc, Scene.morphed(...)); then refit="all" with the second pose
    (or the first again): Scene.refitted_instances over the refitted scene."""
    from hikari_amd import Scene
    c = mo.case(name)
    r = renderer(c.scene0)
    _register(r, name)
    _pose(r, name, refit=True)
    want = Scene.refitted(c.scene0.desc, mo.posed(name)[0], list(c.poses[0]))
    assert_mesh_rebuild_bitwise(r, want)
    k = len(c.poses) - 1
    _pose(r, name, k, refit="all")
    blas = Scene.refitted(c.scene0.desc, mo.posed(name, k)[0], list(c.poses[k]))
    assert_scene_is(r, Scene.refitted_instances(want, blas))
    _pose(r, name, 0)  # and a rebuild gives the host builder's trees again
    assert_mesh_rebuild_bitwise(r, mo.posed(name)[1])
    r.close()


def _frames(name, options=None):
    d1 = mo.posed(name)[1]
    with EditFrames(mo.case(name).scene0, mo.camera_for(name), mo.FRAME_SIZE, floor=0.1, finite=True,
                    options=options) as fr:
        _register(fr.r, name)
        _pose(fr.r, name)
        assert_mesh_rebuild_bitwise(fr.r, d1)
        fr.set_scene(d1)
        fr.frames(2)


@pytest.mark.parametrize("lds_scene", [0, 1, 2])
@pytest.mark.parametrize("name", mo.FRAME_CASES)
def test_frames_after_a_pose_match_oracle(name, lds_scene):
    """Two frames against the oracle on the morphed host scene (one thread, spatial reuse off, the racy scatter targets
    within their tolerance) and the ray counters, with the scene staged in LDS or not."""
    _frames(name, {"lds_scene": lds_scene})


def test_registering_again_smaller_then_larger():
    """A smaller set than before (the block keeps its capacity beside its size), then a larger one (a new block): each
    registration replaces the whole set."""
    from hikari_amd import HikariError
    name = "many_morphs"
    c = mo.case(name)
    r = _posed_renderer(name)
    r.set_mesh_morphs(c.scene0, [3])
    host = mo.posed(name)[0].posed({})
    w = mo.weights(np.random.default_rng([mo.SEED, 99]), c.scene0.meshes[3].morph.target_count)
    host.meshes[3] = c.scene0.morphed({3: w}).meshes[3]
    r.morph_meshes(c.scene0, {3: w}, local_aabbs=caller_aabbs(host, {3}))
    assert_mesh_rebuild_bitwise(r, host.build())
    with pytest.raises(HikariError, match="no registered morph"):
        r.morph_meshes(c.scene0, {0: c.poses[0][0]}, local_aabbs=caller_aabbs(host, {0}))
    r.set_mesh_morphs(c.scene0, c.morphed)
    _pose(r, name, 1)
    assert_mesh_rebuild_bitwise(r, mo.posed(name, 1)[1])
    r.close()


def test_add_meshes_and_set_instances_keep_the_set_and_set_meshes_and_upload_drop_it():
    from hikari_amd import HikariError, plane_mesh
    name = "one_of_three"
    c = mo.case(name)
    s0 = c.scene0
    r = renderer(s0)
    _register(r, name)
    r.add_meshes([plane_mesh(0.3)])
    r.set_instances(s0, previous=list(range(len(s0.instances))), local_aabbs=mc.local_aabbs(s0))
    _pose(r, name)
    assert_mesh_rebuild_bitwise(r, mo.posed(name)[1], longer=True)
    # the same list again, the appended mesh left out: the slices stay where they are, and the set is dropped all the same
    entries = [(s0.mesh_index(i), len(s0.meshes[i].positions)) for i in range(len(s0.meshes))]
    posed_scene = mo.posed(name)[0]
    r.set_meshes(posed_scene, entries, previous=list(range(len(s0.instances))), local_aabbs=mc.local_aabbs(posed_scene))
    assert_mesh_rebuild_bitwise(r, mo.posed(name)[1])
    for again in ("set_meshes", "upload"):
        if again == "upload":
            r.upload_scene(s0)
        with pytest.raises(HikariError, match="no registered morph"):
            _pose(r, name)
        assert_mesh_rebuild_bitwise(r, mo.posed(name)[1] if again == "set_meshes" else s0.desc)
        _register(r, name)
        _pose(r, name)
        assert_mesh_rebuild_bitwise(r, mo.posed(name)[1])
    r.close()


# ------------------------------------------------------------------ refusals
def _index(scene, i, index=None):
    from hikari_amd import _abi
    v, pr, n0, nc = scene.mesh_index(i) if index is None else index
    return _abi.hk_mesh_index(v, pr, (ctypes.c_uint32 * 2)(n0, nc))


def _raw_morphs(r, morphs, n=None):
    from hikari_amd import _abi
    arr = (_abi.hk_mesh_morph * max(1, len(morphs)))(*morphs) if morphs is not None else None
    return raw_call(r, "hk_set_mesh_morphs", arr, (0 if morphs is None else len(morphs)) if n is None else n, None)


def _raw_pose(r, scene, poses, n=None, count=None, models=True, aabbs=True, entry="hk_morph_meshes"):
    from hikari_amd import _abi
    m, a = models_and_aabbs(scene)
    arr = (_abi.hk_morph_pose * max(1, len(poses)))(*poses) if poses is not None else None
    return raw_call(r, entry, arr, (0 if poses is None else len(poses)) if n is None else n, ptr(m, models),
                    ptr(a, aabbs), len(m) if count is None else count, None)


def _skin_scene(scene, i, joints, normals=True):
    """A copy of the scene whose mesh i carries a seeded rig of `joints` joints (and no normals, if asked), and a
    palette for it."""
    from hikari_amd import Mesh, Scene
    rng = np.random.default_rng([mo.SEED, 7, joints])
    m = scene.meshes[i]
    s = Scene()
    s.meshes = list(scene.meshes)
    s.meshes[i] = sc.rig(Mesh(m.positions, m.normals, m.uvs, m.indices, m.topology, None, m.morph), rng, joints)
    s.materials, s.instances = scene.materials, scene.instances
    return s, sc.palette(rng, joints, mo.cell_of(m))


def test_refusals_leave_the_context_and_the_morph_set_as_they_were():
    """Every refusal in the header's comments returns its code with a message; nothing changed: all nine arrays are byte
    for byte what they were, and the morph set registered before is still the one a pose then uses."""
    from hikari_amd import HikariRenderer, _abi
    name = "one_of_three"
    c = mo.case(name)
    s0 = c.scene0
    keep = []

    def morph(i, vertex_count=None, index=None, targets=None, null=None):
        m = s0.meshes[i]
        p = np.ascontiguousarray(m.positions, np.float32)
        nr = np.ascontiguousarray(m.normals, np.float32)
        dp = np.ascontiguousarray(m.morph.position_deltas, np.float32)
        dn = np.ascontiguousarray(m.morph.normal_deltas, np.float32)
        keep.extend([p, nr, dp, dn])
        at = {"positions": p.ctypes.data, "normals": nr.ctypes.data, "position_deltas": dp.ctypes.data,
              "normal_deltas": dn.ctypes.data}
        if null:
            at[null] = None
        return _abi.hk_mesh_morph(_index(s0, i, index), len(p) if vertex_count is None else vertex_count, at["positions"],
                                  at["normals"], len(dp) if targets is None else targets, at["position_deltas"],
                                  at["normal_deltas"])

    def pose(i, weights=None, targets=None, null=False, joints=None, joint_count=None):
        w = np.ascontiguousarray(c.poses[0][1] if weights is None else weights, np.float32)
        j = None if joints is None else np.ascontiguousarray(joints, np.float32)
        keep.extend([w, j])
        return _abi.hk_morph_pose(_index(s0, i), None if null else w.ctypes.data, len(w) if targets is None else targets,
                                  None if j is None else j.ctypes.data,
                                  (0 if j is None else len(j)) if joint_count is None else joint_count)

    empty = HikariRenderer(0)
    rc, msg = _raw_morphs(empty, [morph(1)])
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    rc, msg = _raw_pose(empty, s0, [pose(1)])
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()

    r = renderer(s0)
    _register(r, name)
    skinned, pal = _skin_scene(s0, 1, 5)
    r.set_mesh_skins(skinned, [1])
    before = device_arrays(r)
    v, pr, n0, nc = s0.mesh_index(1)
    nv = len(s0.meshes[1].positions)
    top = int(s0.meshes[1].indices.max())
    refused_morphs = [
        ("null list", dict(morphs=None, n=1), "null"),
        ("null positions", dict(morphs=[morph(1, null="positions")]), "null pointer"),
        ("null deltas", dict(morphs=[morph(1, null="position_deltas")]), "null pointer"),
        ("normal deltas alone", dict(morphs=[morph(1, null="normals")]), "normal_deltas without normals"),
        ("no targets", dict(morphs=[morph(1, targets=0)]), "target_count is outside"),
        ("too many targets", dict(morphs=[morph(1, targets=257)]), "target_count is outside"),
        ("not a mesh: vertex", dict(morphs=[morph(1, index=(v + 1, pr, n0, nc))]), "not a known mesh slice"),
        ("not a mesh: node", dict(morphs=[morph(1, index=(v, pr, n0 + 3, nc - 3))]), "not a known mesh slice"),
        ("too few vertices", dict(morphs=[morph(1, vertex_count=top)]), "vertex indices"),
        ("into the next mesh", dict(morphs=[morph(1, vertex_count=nv + 1)]), "past its vertex slice"),
        ("twice", dict(morphs=[morph(1), morph(0), morph(1)]), "listed twice"),
    ]
    for label, kw, text in refused_morphs:
        rc, msg = _raw_morphs(r, **kw)
        assert rc == _abi.HK_ERR_INVALID and text in msg, (label, rc, msg)
    bare, bare_pal = _skin_scene(s0, 1, 3)
    refused_poses = [
        ("null list", dict(poses=None, n=1), "null"),
        ("null weights", dict(poses=[pose(1, null=True)]), "null pointer"),
        ("null models", dict(poses=[pose(1)], models=False), "null"),
        ("null aabbs", dict(poses=[pose(1)], aabbs=False), "null"),
        ("count", dict(poses=[pose(1)], count=len(s0.instances) - 1), "every instance"),
        ("no morph", dict(poses=[pose(2)]), "no registered morph"),
        ("target count", dict(poses=[pose(1, targets=4)]), "differs from the registered morph's"),
        ("no skin", dict(poses=[pose(0, weights=np.ones(2), joints=pal)]), "no registered skin"),
        ("joint count", dict(poses=[pose(1, joints=pal, joint_count=4)]), "differs from the registered skin's"),
        ("twice", dict(poses=[pose(1), pose(0, weights=np.ones(2)), pose(1)]), "poses a mesh twice"),
    ]
    for entry in ("hk_morph_meshes", "hk_morph_meshes_refit", "hk_morph_meshes_refit_all"):
        for label, kw, text in refused_poses:
            rc, msg = _raw_pose(r, s0, entry=entry, **kw)
            assert rc == _abi.HK_ERR_INVALID and text in msg and msg.startswith(entry), (entry, label, rc, msg)
            assert device_arrays(r) == before, (entry, label)
    # a skin registered without normals under a morph registered with them
    r.set_mesh_skins(bare, [1], keep_normals=(1,))
    rc, msg = _raw_pose(r, s0, [pose(1, joints=bare_pal)])
    assert rc == _abi.HK_ERR_INVALID and "disagree on whether normals are rewritten" in msg, (rc, msg)
    assert device_arrays(r) == before
    # n == 0 is hk_update_instances
    rc, msg = _raw_pose(r, s0, [], n=0)
    assert rc == 0, msg
    assert_mesh_rebuild_bitwise(r, s0.desc)
    # the set registered before the refusals is still there
    _pose(r, name)
    assert_mesh_rebuild_bitwise(r, mo.posed(name)[1])
    # an empty list drops it
    rc, msg = _raw_morphs(r, [], n=0)
    assert rc == 0, msg
    rc, msg = _raw_pose(r, s0, [pose(1)])
    assert rc == _abi.HK_ERR_INVALID and "no registered morph" in msg
    r.close()


def test_pose_on_a_caller_stream():
    """tris_1281 registered and posed on a stream of the caller's: both calls wait for their stream once, so the arrays
    are complete when hk_morph_meshes returns; the test synchronises the stream all the same."""
    name = "tris_1281"
    r = renderer(mo.case(name).scene0)
    with caller_stream() as (s, sync):
        _register(r, name, stream=s)
        _pose(r, name, stream=s)
        sync()
        assert_mesh_rebuild_bitwise(r, mo.posed(name)[1])
        r.close()


def test_kernel_timing_names_the_pose_and_the_refit_spans():
    name = "verts_64"
    r = renderer(mo.case(name).scene0)
    _register(r, name)
    r.enable_kernel_timing(True)
    _pose(r, name)
    _pose(r, name, refit=True)
    r.sync()
    names = r.kernel_timing()
    assert "morph_meshes" in names and "refit_morph_vertices" in names and "refit_morph_bounds" in names
    r.close()


def test_plugin_forwards_both_calls():
    from hikari_amd import HikariPlugin
    name = "keep_normals"
    c = mo.case(name)
    p = HikariPlugin(c.scene0)
    p.set_mesh_morphs(c.scene0, c.morphed, c.keep_normals)
    p.morph_meshes(c.scene0, c.poses[0], local_aabbs=caller_aabbs(c.scene0, set(c.poses[0])))
    assert_mesh_rebuild_bitwise(p.renderer, mo.posed(name)[1])
    p.renderer.close()


def test_the_skin_set_is_untouched_by_a_morph_call():
    """skin_cases.one_of_three with a morph on its unskinned mesh 2: after hk_morph_meshes on mesh 2, hk_skin_meshes on
    mesh 1 still gives the skin case's arrays (with mesh 2 morphed), and the morph set survives the skin call."""
    from hikari_amd import Mesh, Scene
    name = "one_of_three"
    c = sc.case(name)
    rng = np.random.default_rng([mo.SEED, 5])
    m = c.scene0.meshes[2]
    s0 = Scene()
    s0.meshes = list(c.scene0.meshes)
    s0.meshes[2] = mo.targets(Mesh(m.positions, m.normals, m.uvs, m.indices, m.topology), rng, 3, mo.cell_of(m))
    s0.materials, s0.instances = c.scene0.materials, c.scene0.instances
    s0.build()
    w = mo.weights(rng, 3)
    r = renderer(s0)
    r.set_mesh_skins(s0, c.skinned, c.keep_normals)
    r.set_mesh_morphs(s0, [2])
    morphed = s0.morphed({2: w})
    r.morph_meshes(s0, {2: w}, local_aabbs=caller_aabbs(s0, {2}))
    assert_mesh_rebuild_bitwise(r, morphed.build())
    both = morphed.posed(c.poses[0])
    r.skin_meshes(s0, c.poses[0], local_aabbs=caller_aabbs(morphed, set(c.poses[0])))
    assert_mesh_rebuild_bitwise(r, both.build())
    w2 = mo.weights(rng, 3, [1])
    again = both.posed({})
    again.meshes[2] = s0.morphed({2: w2}).meshes[2]
    r.morph_meshes(s0, {2: w2}, local_aabbs=caller_aabbs(again, {2}))
    assert_mesh_rebuild_bitwise(r, again.build())
    r.close()
