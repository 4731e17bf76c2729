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
"""
import ctypes

import numpy as np
import pytest

import mesh_cases as mc
import refit_cases as rc
import skin_cases as sc
from parity import RACY, canon_plane, compare_frame, hip_runtime, host_scene_array, passes
from parity import renderer
from test_gpu_mesh_update import NODE_DT, PRIM_DT, VERTEX_DT, _expected_asset_nodes, assert_mesh_rebuild_bitwise
from test_gpu_skin import caller_aabbs

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
        want = _expected_asset_nodes(scene0.desc)
        for i in (0, 2):
            v, p, n0, nc = scene0.mesh_index(i)
            nv, k = len(scene0.meshes[i].positions), (nc + 2) // 3
            for idx, dt, a, n, host in ((0, VERTEX_DT, v, nv, None), (1, PRIM_DT, p, k, None), (2, NODE_DT, n0, nc, want)):
                h = host_scene_array(scene0.desc, idx, dt) if host is None else host
                g = r.scene_array(idx, dt, len(h))
                assert h[a: a + n].tobytes() == g[a: a + n].tobytes(), (i, idx)
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
    from hikari_amd import HikariSettings, Upscale, frame_inputs, load_noise
    from oracle import Oracle
    scene0, scene1 = rc.case(name)
    d1 = rc.refitted(name)
    cam, lights = rc.camera_for(name)
    w, h = rc.FRAME_SIZE
    r = renderer(scene0, (w, h), options=options, wavefront=wavefront)
    _refit(r, name)
    assert_mesh_rebuild_bitwise(r, d1)
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False)
    o = Oracle(scene0.desc, load_noise(), w, h, 1.0, threads=1)
    o.set_scene(d1)
    s = st.to_c()
    errors = []
    for f in range(2):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi)
        compare_frame(r, o, f, errors, racy=RACY)
    assert not errors, "\n".join(errors[:10])
    assert r.counters() == o.counters()
    depth = canon_plane(11, o.output(11)).view(np.float32).reshape(h, w, 4)[..., 3]
    assert (depth > 0).mean() >= 0.2  # the view covers the mesh
    o.close()
    r.close()


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


def _raw_renderer(desc, size):
    """A context that uploaded a desc as it is."""
    from hikari_amd import HikariRenderer
    r = HikariRenderer(0)
    r.set_noise()
    assert r._L.hk_scene_upload(r.ctx, ctypes.byref(desc)) == 0
    r.resize(*size, 1.0)
    return r


def test_traced_rays_after_the_refit_equal_a_fresh_context():
    """256 seeded rays through hk_trace after the refit, against a context that uploaded the refitted desc."""
    name = "shared_mesh"
    scene0, scene1 = rc.case(name)
    rng = np.random.default_rng(rc.SEED)
    n = 256
    org = rng.uniform([-1.5, 0.0, 1.0], [1.5, 2.0, 4.0], (n, 3))
    d = rng.uniform([-1.5, 0.0, -0.5], [1.5, 2.0, 0.2], (n, 3)) - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d], axis=1).astype(np.float32)
    early = np.where(rng.random(n) < 0.5, 0.0, 65535.0).astype(np.float32)
    excl = rng.integers(0, len(scene1.instances) + 1, n).astype(np.uint32)
    r = renderer(scene0, rc.FRAME_SIZE)
    _refit(r, name)
    fresh = _raw_renderer(rc.refitted(name), rc.FRAME_SIZE)
    a, b = r.trace(rays, None, early, excl), fresh.trace(rays, None, early, excl)
    assert np.array_equal(a, b)
    assert (b[:, 3] < len(scene1.instances)).mean() > 0.3  # many of them hit
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
    from hikari_amd import HikariSettings, Upscale, frame_inputs, load_noise
    from oracle import Oracle
    c = sc.case(name)
    w, h = mc.FRAME_SIZE
    r = renderer(c.scene0, (w, h))
    r.set_mesh_skins(c.scene0, c.skinned, c.keep_normals)
    _pose(r, name)
    want = _skin_expect(name)
    assert_mesh_rebuild_bitwise(r, want)
    cam, lights = sc.camera_for(name)
    o = Oracle(c.scene0.desc, load_noise(), w, h, 1.0, threads=1)
    o.set_scene(want)
    s = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False).to_c()
    errors = []
    for f in range(2):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi)
        compare_frame(r, o, f, errors, racy=RACY)
    assert not errors, "\n".join(errors[:10])
    assert r.counters() == o.counters()
    o.close()
    r.close()


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
    from test_gpu_mesh_add import _add, _added_so_far, _set, assert_mesh_arrays
    from parity import assert_rebuild_bitwise
    name = "then_update"
    c = ac.case(name)
    r = renderer(c.scenes[0])
    last = len(c.scenes) - 1
    for k in list(ac.steps(name))[1:]:
        _add(r, name, k)
        _set(r, name, k)
    scene, ids = c.update
    r.update_meshes(scene, ids, local_aabbs=ac.local_aabbs(scene), refit=True)
    want = _expect(ac.built(name, last), scene, ids)
    assert_rebuild_bitwise(r, want)
    assert_mesh_arrays(r, want, _added_so_far(name, last))
    rebuilt = ac.built_update(name)
    assert host_scene_array(want, 2, NODE_DT).tobytes() != host_scene_array(rebuilt, 2, NODE_DT).tobytes()
    r.close()


def test_refit_of_a_slice_moved_by_set_meshes():
    """mesh_set_cases' then_update: the mesh hk_set_meshes moved to another place in the arrays, refit there."""
    import mesh_set_cases as ms
    from test_gpu_mesh_set import _host_slices, _step, assert_scene_is
    name = "then_update"
    c = ms.case(name)
    r = renderer(c.scenes[0])
    last = len(c.scenes) - 1
    for k in list(ms.steps(name))[1:]:
        _step(r, name, k)
    kind, scene, ids = c.after
    assert kind == "update"
    r.update_meshes(scene, ids, local_aabbs=ms.local_aabbs(scene), refit=True)
    assert_scene_is(r, _expect(ms.built(name, last), scene, ids), _host_slices(name, last))
    r.close()


# ------------------------------------------------------------------ refusals
def _raw_refit(r, scene, ups, count=None, models=True, aabbs=True):
    from hikari_amd import _abi
    m = np.ascontiguousarray(scene.instance_models(), np.float32)
    a = np.ascontiguousarray(mc.local_aabbs(scene), np.float32)
    arr = (_abi.hk_mesh_update * max(1, len(ups)))(*ups) if ups is not None else None
    rc_ = r._L.hk_refit_meshes(r.ctx, arr, 0 if ups is None else len(ups), m.ctypes.data if models else None,
                               a.ctypes.data if aabbs else None, len(m) if count is None else count, None)
    return rc_, r._L.hk_last_error(r.ctx).decode()


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
    hip = hip_runtime()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    _refit(r, name, stream=s)
    assert hip.hipStreamSynchronize(s) == 0
    assert_mesh_rebuild_bitwise(r, rc.refitted(name))
    r.close()
    assert hip.hipStreamDestroy(s) == 0


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
