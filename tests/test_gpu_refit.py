"""hk_refit_meshes / hk_skin_meshes_refit at their size and shape edges: the cases of tests/refit_cases.py (each proven to
sit on its edge by tests/test_refit_cases.py, without a GPU) uploaded as scene0 and refit to scene1's vertices.  All nine
arrays byte for byte Scene.refitted(...): scene1 as the host builds it, except the asset nodes, which are the slices the
device held before passed through hks_refit_nodes (itself held to tests/refit_numpy.py by
tests/test_refit_independent.py), the leaves carrying their triangle's box as on the device.  Frames, G-buffers, traced
rays and counters against the CPU oracle on that scene.

What each case exists for in csrc/hk_dynamic.hip:
  tris_1, tris_2               k_refit_small with nothing but a leaf / two entry nodes; k_refit_large not launched
  small_32 / small_35          no large node (the list stays empty) / the first range past REFIT_SMALL: one listed node
  tris_1281, tris_2600         hundreds of large nodes, ranges the 256 threads stride over more than once
  deep_17, deep_65             chain-shaped trees: small ranges inside large ones, every level a large node
  many_meshes                  40 slices in one call: refit_mesh_of's search, slices with and without large nodes
  one_of_three                 the unlisted slices keep their bytes
  neg_zero, coincident_300     zeros of both signs under an unordered fold; the `halves` tree
  folded                       a deformation far from the pose the tree was built for
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.
"""
import ctypes

import numpy as np
import pytest

import mesh_cases as mc
import refit_cases as rc
import skin_cases as sc
from parity import NODE_DT, assert_rebuild_bitwise, host_scene_array, renderer
from scene_edits import (EditFrames, assert_mesh_arrays, assert_mesh_rebuild_bitwise, assert_scene_is,
                         assert_slices_kept, assert_traces_equal_fresh, caller_stream, models_and_aabbs, ptr, raw_call,
                         raw_renderer)
from skin_cases import caller_aabbs

pytestmark = pytest.mark.gpu


def _refit(r, name, which=1, stream=None, refit=True, **kw):
    scene = rc.update_source(name, which)
    r.update_meshes(scene, rc.listed(name), local_aabbs=mc.local_aabbs(scene), stream=stream, refit=refit, **kw)


def _expect(desc0, scene1, ids):
    from hikari_amd import Scene
    return Scene.refitted(desc0, scene1, ids)


# ------------------------------------------------------------------ arrays
@pytest.mark.parametrize("name", rc.ARRAY_CASES)
def test_refit_arrays_match_the_refitted_scene(name):
    """Upload scene0, refit the listed meshes to scene1's vertices: every array equals the refitted desc, array 2 with
    the device's leaf boxes.  one_of_three: the unlisted meshes' slices also equal scene0's."""
    scene0, scene1 = rc.case(name)
    r = renderer(scene0)
    _refit(r, name)
    assert_mesh_rebuild_bitwise(r, rc.refitted(name))
    if name == "one_of_three":
        assert_slices_kept(r, scene0, (0, 2))
    r.close()


@pytest.mark.parametrize("name", rc.REPEAT_CASES)
def test_repeated_refits(name):
    """A second refit back to scene0's vertices equals refitted(desc0, scene0): a refit of a refit is the direct one (the
    boxes are derived from the leaves alone), on the scratch and the list the first call left."""
    scene0, scene1 = rc.case(name)
    r = renderer(scene0)
    _refit(r, name)
    assert_mesh_rebuild_bitwise(r, rc.refitted(name))
    _refit(r, name, 0)
    direct = _expect(scene0.desc, scene0, rc.listed(name))
    assert_mesh_rebuild_bitwise(r, direct)
    chained = _expect(rc.refitted(name), scene0, rc.listed(name))
    assert host_scene_array(chained, 2, NODE_DT).tobytes() == host_scene_array(direct, 2, NODE_DT).tobytes()
    _refit(r, name)
    assert_mesh_rebuild_bitwise(r, rc.refitted(name))
    r.close()


@pytest.mark.parametrize("name", ["tris_1281", "many_meshes"])
def test_rebuild_after_refit_and_refit_after_rebuild(name):
    """hk_update_meshes after a refit gives the host-built scene1; hk_refit_meshes after that keeps the NEW topology."""
    scene0, scene1 = rc.case(name)
    r = renderer(scene0)
    _refit(r, name)
    assert_mesh_rebuild_bitwise(r, rc.refitted(name))
    _refit(r, name, refit=False)
    assert_mesh_rebuild_bitwise(r, rc.built1(name))
    _refit(r, name, 0)
    assert_mesh_rebuild_bitwise(r, _expect(rc.built1(name), scene0, rc.listed(name)))
    r.close()


def test_one_context_several_scenes():
    r = renderer(rc.case("tris_2")[0])
    for k, name in enumerate(("tris_2", "many_meshes", "small_35")):
        if k:
            r.upload_scene(rc.case(name)[0])
        _refit(r, name)
        assert_mesh_rebuild_bitwise(r, rc.refitted(name))
    r.close()


def test_no_meshes_is_update_instances():
    name = "one_of_three"
    scene0, scene1 = rc.case(name)
    r = renderer(scene0)
    r.update_meshes(scene1, [], local_aabbs=mc.local_aabbs(scene0), refit=True)
    assert_mesh_rebuild_bitwise(r, scene0.desc)
    r.close()


# ------------------------------------------------------------------ frames
def _frames(name, options=None, wavefront=False):
    scene0, scene1 = rc.case(name)
    d1 = rc.refitted(name)
    # (the floor: "at least 0.2" and "more than 0.2" are one thing at 32 x 24, where 0.2 of the frame is 153.6 pixels)
    with EditFrames(scene0, rc.camera_for(name), rc.FRAME_SIZE, floor=0.2, options=options, wavefront=wavefront) as fr:
        _refit(fr.r, name)
        assert_mesh_rebuild_bitwise(fr.r, d1)
        fr.set_scene(d1)
        fr.frames(2)


@pytest.mark.parametrize("name", rc.FRAME_CASES)
def test_frames_after_refit_match_oracle(name):
    """After the array check, two 32 x 24 frames against the oracle on the refitted desc (one thread, spatial reuse off,
    the racy scatter targets within their tolerance) and the ray counters: what is derived from the refit BLAS (leaf
    boxes, wide layout, collapsed walk nodes) is what the frames walk."""
    _frames(name)


@pytest.mark.parametrize("options", [{"lds_scene": 0}, {"lds_scene": 1}, {"lds_scene": 2}, {"leaf_collapse": 0}],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", rc.VARIANT_CASES)
def test_frames_under_staging_and_collapse_options(name, options):
    _frames(name, options)


def test_frames_with_the_wavefront_pass():
    _frames("emissive_mesh", wavefront=True)


def test_traced_rays_after_the_refit_equal_a_fresh_context():
    """256 seeded rays through hk_trace after the refit, against a context that uploaded the refitted desc."""
    name = "shared_mesh"
    scene0, scene1 = rc.case(name)
    r = renderer(scene0, rc.FRAME_SIZE)
    _refit(r, name)
    fresh = raw_renderer(rc.refitted(name), rc.FRAME_SIZE)
    assert_traces_equal_fresh(r, fresh, rc.SEED, len(scene1.instances))
    fresh.close()
    r.close()


# ------------------------------------------------------------------ skins
def _skin_expect(name, k=0):
    c = sc.case(name)
    return _expect(c.scene0.desc, sc.posed(name, k)[0], list(c.poses[k]))


def _pose(r, name, k=0, stream=None, refit=True):
    c = sc.case(name)
    pose = c.poses[k]
    r.skin_meshes(c.scene0, pose, local_aabbs=caller_aabbs(c.scene0, set(pose)), stream=stream, refit=refit)


@pytest.mark.parametrize("name", sc.FRAME_CASES)
def test_skin_refit_arrays_and_frames(name):
    """Bind pose uploaded, skins registered, posed with refit=True: the arrays are refitted(bind desc, Scene.posed(...)),
    and two frames equal the oracle's on it."""
    c = sc.case(name)
    want = _skin_expect(name)
    with EditFrames(c.scene0, sc.camera_for(name), mc.FRAME_SIZE) as fr:
        fr.r.set_mesh_skins(c.scene0, c.skinned, c.keep_normals)
        _pose(fr.r, name)
        assert_mesh_rebuild_bitwise(fr.r, want)
        fr.set_scene(want)
        fr.frames(2)


def test_pose_a_refit_pose_b_refit_pose_b_rebuild():
    name = "tris_1281"
    c = sc.case(name)
    r = renderer(c.scene0)
    r.set_mesh_skins(c.scene0, c.skinned, c.keep_normals)
    _pose(r, name, 0)
    assert_mesh_rebuild_bitwise(r, _skin_expect(name, 0))
    _pose(r, name, 1)
    assert_mesh_rebuild_bitwise(r, _skin_expect(name, 1))
    _pose(r, name, 1, refit=False)
    assert_mesh_rebuild_bitwise(r, sc.posed(name, 1)[1])
    _pose(r, name, 0)  # and a refit on the rebuilt tree keeps it
    assert_mesh_rebuild_bitwise(r, _expect(sc.posed(name, 1)[1], sc.posed(name, 0)[0], list(c.poses[0])))
    r.close()


# ------------------------------------------------------------------ after scene edits
def test_refit_of_a_mesh_appended_and_spawned():
    """mesh_add_cases' then_update: the mesh hk_add_meshes appended and hk_set_instances spawned, refit in its slice
    past the uploaded arrays."""
    import mesh_add_cases as ac
    name = "then_update"
    c = ac.case(name)
    r = renderer(c.scenes[0])
    last = len(c.scenes) - 1
    for k in list(ac.steps(name))[1:]:
        ac.add(r, name, k)
        ac.spawn(r, name, k)
    scene, ids = c.update
    r.update_meshes(scene, ids, local_aabbs=ac.local_aabbs(scene), refit=True)
    want = _expect(ac.built(name, last), scene, ids)
    assert_rebuild_bitwise(r, want)
    assert_mesh_arrays(r, want, ac.added_so_far(name, last))
    rebuilt = ac.built_update(name)
    assert host_scene_array(want, 2, NODE_DT).tobytes() != host_scene_array(rebuilt, 2, NODE_DT).tobytes()
    r.close()


def test_refit_of_a_slice_moved_by_set_meshes():
    """mesh_set_cases' then_update: the mesh hk_set_meshes moved to another place in the arrays, refit there."""
    import mesh_set_cases as ms
    name = "then_update"
    c = ms.case(name)
    r = renderer(c.scenes[0])
    last = len(c.scenes) - 1
    for k in list(ms.steps(name))[1:]:
        ms.step(r, name, k)
    kind, scene, ids = c.after
    assert kind == "update"
    r.update_meshes(scene, ids, local_aabbs=ms.local_aabbs(scene), refit=True)
    assert_scene_is(r, _expect(ms.built(name, last), scene, ids), ms.host_slices(name, last))
    r.close()


# ------------------------------------------------------------------ refusals
def _raw_refit(r, scene, ups, count=None, models=True, aabbs=True):
    from hikari_amd import _abi
    m, a = models_and_aabbs(scene)
    arr = (_abi.hk_mesh_update * max(1, len(ups)))(*ups) if ups is not None else None
    return raw_call(r, "hk_refit_meshes", arr, 0 if ups is None else len(ups), ptr(m, models), ptr(a, aabbs),
                    len(m) if count is None else count, None)


def test_refusals_leave_the_context_usable():
    """hk_update_meshes' refusals under hk_refit_meshes' own name; nothing was changed: the arrays still equal scene0's,
    and a refit then succeeds and matches."""
    from hikari_amd import HikariRenderer, _abi
    name = "one_of_three"
    scene0, scene1 = rc.case(name)
    keep = []

    def entry(i, vertex_count=None, index=None, positions=True):
        mesh = scene1.meshes[i]
        p = np.ascontiguousarray(mesh.positions, np.float32)
        n = np.ascontiguousarray(mesh.normals, np.float32)
        keep.extend([p, n])
        v, pr, n0, nc = scene1.mesh_index(i) if index is None else index
        return _abi.hk_mesh_update(_abi.hk_mesh_index(v, pr, (ctypes.c_uint32 * 2)(n0, nc)),
                                   len(p) if vertex_count is None else vertex_count,
                                   p.ctypes.data if positions else None, n.ctypes.data)

    empty = HikariRenderer(0)
    rc_, msg = _raw_refit(empty, scene1, [entry(1)])
    assert rc_ == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()

    r = renderer(scene0)
    v, pr, n0, nc = scene1.mesh_index(1)
    nv = len(scene1.meshes[1].positions)
    top = int(scene1.meshes[1].indices.max())
    refused = [
        ("null list", dict(ups=None), "hk_refit_meshes: null"),
        ("null models", dict(ups=[entry(1)], models=False), "hk_refit_meshes: null"),
        ("null aabbs", dict(ups=[entry(1)], aabbs=False), "hk_refit_meshes: null"),
        ("null positions", dict(ups=[entry(1, positions=False)]), "hk_refit_meshes: mesh 0 has no positions"),
        ("count", dict(ups=[entry(1)], count=len(scene1.instances) - 1), "hk_refit_meshes needs every instance"),
        ("not a mesh: vertex", dict(ups=[entry(1, index=(v + 1, pr, n0, nc))]), "not an instanced mesh"),
        ("not a mesh: node", dict(ups=[entry(1, index=(v, pr, n0 + 3, nc - 3))]), "not an instanced mesh"),
        ("too few vertices", dict(ups=[entry(1, vertex_count=top)]), "vertex indices"),
        ("into the next mesh", dict(ups=[entry(1, vertex_count=nv + 1)]), "past its vertex slice"),
        ("twice", dict(ups=[entry(1), entry(0), entry(1)]), "hk_refit_meshes: mesh 2 is listed twice"),
    ]
    for label, kw, text in refused:
        rc_, msg = _raw_refit(r, scene1, **kw)
        assert rc_ == _abi.HK_ERR_INVALID and text in msg, (label, rc_, msg)
        assert_mesh_rebuild_bitwise(r, scene0.desc)
    _refit(r, name)
    assert_mesh_rebuild_bitwise(r, rc.refitted(name))
    r.close()


def test_skin_refit_refusals_and_a_singular_model():
    from hikari_amd import HikariError
    name = "one_of_three"
    c = sc.case(name)
    r = renderer(c.scene0)
    pose = c.poses[0]
    with pytest.raises(HikariError, match="hk_skin_meshes_refit: pose 0 names a mesh with no registered skin"):
        _pose(r, name)
    r.set_mesh_skins(c.scene0, c.skinned, c.keep_normals)
    i, joints = next(iter(pose.items()))
    with pytest.raises(HikariError, match="hk_skin_meshes_refit: pose 0: joint_count"):
        r.skin_meshes(c.scene0, {i: joints[:-1]}, local_aabbs=caller_aabbs(c.scene0, {i}), refit=True)
    assert_mesh_rebuild_bitwise(r, c.scene0.desc)
    models = c.scene0.instance_models().copy()
    models[0, 4:8] = 0.0  # a zero column
    with pytest.raises(HikariError, match="singular instance transform"):
        r.skin_meshes(c.scene0, pose, models=models, local_aabbs=caller_aabbs(c.scene0, set(pose)), refit=True)
    _pose(r, name)
    assert_mesh_rebuild_bitwise(r, _skin_expect(name))
    r.close()


# ------------------------------------------------------------------ streams and forwarding
def test_refit_on_a_caller_stream():
    name = "tris_1281"
    scene0, scene1 = rc.case(name)
    r = renderer(scene0)
    with caller_stream() as (s, sync):
        _refit(r, name, stream=s)
        sync()
        assert_mesh_rebuild_bitwise(r, rc.refitted(name))
        r.close()


def test_plugin_forwards_refit():
    from hikari_amd import HikariPlugin
    name = "strip"
    scene0, scene1 = rc.case(name)
    p = HikariPlugin(scene0)
    p.update_meshes(scene1, rc.listed(name), local_aabbs=mc.local_aabbs(scene1), refit=True)
    assert_mesh_rebuild_bitwise(p.renderer, rc.refitted(name))
    p.renderer.close()
    c = sc.case("keep_normals")
    p = HikariPlugin(c.scene0)
    p.set_mesh_skins(c.scene0, c.skinned, c.keep_normals)
    p.skin_meshes(c.scene0, c.poses[0], local_aabbs=caller_aabbs(c.scene0, set(c.poses[0])), refit=True)
    assert_mesh_rebuild_bitwise(p.renderer, _skin_expect("keep_normals"))
    p.renderer.close()
