"""hk_update_meshes at its size, shape and depth edges: the cases of tests/mesh_cases.py (each proven to sit on its edge
by tests/test_mesh_cases.py, without a GPU) uploaded as scene0, updated to scene1's vertices, and the rewritten vertex
and primitive arrays, the rebuilt BLAS and everything the instance rebuild derives from them compared byte for byte with
the host builder's; frames, G-buffers, traced rays and counters against the CPU oracle on the host-built scene1.

The branch of csrc/hk_dynamic.hip each case exists for:
  tris_1, tris_2               k_build_mesh_bvh with a lone leaf / one split
  tris_128 / tris_129          the per-thread split alone / coop_split entered at the root, COOP_MIN
  tris_256 / tris_257          one / two 256-chunks of coop_split's ballot ranking
  tris_1280 / tris_1281        k_build_mesh_bvh<true> (LDS-staged) / <false> (global memory), BVH_LDS_SHAPES
  tris_2600                    the global build with several levels of big segments
  many_meshes                  40 meshes in one call: workgroups past the first in both build launches, on scratch
                               slices past 0; k_update_mesh_geometry's search over the table
  one_of_three                 the unlisted meshes' vertex, primitive and node bytes stay
  shared_mesh                  one mesh, five instances
  emissive_mesh                areas, alias table, surface_area and the light BVH follow the new triangles
  coincident_100 / _300        `halves` in split_segment / in coop_split
  degenerate, neg_zero         zero-area triangles, repeated vertices; zeros of both signs in the shape boxes
  strip, keep_normals          a TriangleStrip's primitives; normals = NULL
  deepen_16 / _17, shallower,  `levels`: the BLAS part of the G-buffer walk's stack bound rises to 16 / 17 / 65 and
  too_deep                     falls again
"""
import ctypes

import numpy as np
import pytest

import mesh_cases as mc
from parity import (NODE_DT, RACY, assert_rebuild_bitwise, canon_plane, compare_frame, hip_runtime, host_scene_array,
                    mismatch_report, passes, renderer)

pytestmark = pytest.mark.gpu

DEPTH_SIZE = (64, 48)
VERTEX_DT, PRIM_DT = np.dtype((np.void, 32)), np.dtype((np.void, 48))


def _update(r, name, which=1, stream=None, **kw):
    scene = mc.update_source(name, which)
    r.update_meshes(scene, mc.listed(name), local_aabbs=mc.local_aabbs(scene), stream=stream, **kw)


# ---- the leaf boxes of the device's asset nodes, restated: k_fill_blas_leaves takes vmin(a, vmin(b, c)) and
# vmax(a, vmax(b, c)) of the triangle's corners with the device's fminf / fmaxf, which order -0 below +0
def _device_min(p):
    m = p.min(axis=1)
    zero, neg = m == 0.0, (p.view(np.uint32) == 0x80000000).any(axis=1)
    m[zero & neg], m[zero & ~neg] = -0.0, 0.0
    return m


def _device_max(p):
    m = p.max(axis=1)
    zero, pos = m == 0.0, (p.view(np.uint32) == 0).any(axis=1)
    m[zero & pos], m[zero & ~pos] = 0.0, -0.0
    return m


def _expected_asset_nodes(desc):
    """The host's asset nodes with each instanced mesh's leaves carrying their triangle's box."""
    nodes = host_scene_array(desc, 2, NODE_DT).copy()
    corners = np.ascontiguousarray(
        np.frombuffer(host_scene_array(desc, 1, PRIM_DT).tobytes(), np.float32).reshape(-1, 3, 4)[:, :, :3])
    for _, prim, n0, nc in set(mc.mesh_slices(desc)):
        part = nodes[n0: n0 + nc]
        leaf = part["entry"] >= 0x80000000
        tri = corners[prim + (part["entry"][leaf] - 0x80000000)]
        part["min"][leaf], part["max"][leaf] = _device_min(tri), _device_max(tri)
    return nodes


def assert_mesh_rebuild_bitwise(r, desc):
    """Vertices and primitives byte for byte the host's; the asset nodes: entry / exit everywhere, inner nodes whole,
    each leaf the byte image of its triangle's box; and assert_rebuild_bitwise for what the instance rebuild derives
    (instances, alias table, emissives, light BVH, TLAS)."""
    for idx, dt in ((0, VERTEX_DT), (1, PRIM_DT)):
        h = host_scene_array(desc, idx, dt)
        assert h.tobytes() == r.scene_array(idx, dt, len(h)).tobytes(), f"array {idx} differs"
    want = _expected_asset_nodes(desc)
    got = r.scene_array(2, NODE_DT, len(want))
    assert np.array_equal(want["entry"], got["entry"]) and np.array_equal(want["exit"], got["exit"])
    assert want.tobytes() == got.tobytes()
    assert_rebuild_bitwise(r, desc)


def test_device_min_max_restate_the_sign_of_zero():
    p = np.array([[[0.0, -0.0, 1.0], [-0.0, -0.0, 2.0], [0.0, -0.0, 0.0]]], np.float32)
    assert _device_min(p).view(np.uint32).tolist() == [[0x80000000, 0x80000000, 0]]
    assert _device_max(p).view(np.uint32).tolist() == [[0, 0x80000000, 0x40000000]]


@pytest.mark.parametrize("name", mc.ARRAY_CASES)
def test_rebuilt_arrays_match_host_builder(name):
    """Upload scene0, update the listed meshes to scene1's vertices: every array equals the host builder's for scene1,
    the BLAS topology included.  one_of_three: the unlisted meshes' slices also equal scene0's."""
    scene0, scene1 = mc.case(name)
    r = renderer(scene0)
    _update(r, name)
    assert_mesh_rebuild_bitwise(r, mc.built1(name))
    if name == "one_of_three":
        for i in (0, 2):
            v, p, n0, nc = scene0.mesh_index(i)
            nv, k = len(scene0.meshes[i].positions), (nc + 2) // 3
            want = _expected_asset_nodes(scene0.desc)
            for idx, dt, a, n, host in ((0, VERTEX_DT, v, nv, None), (1, PRIM_DT, p, k, None), (2, NODE_DT, n0, nc, want)):
                h = host_scene_array(scene0.desc, idx, dt) if host is None else host
                g = r.scene_array(idx, dt, len(h))
                assert h[a: a + n].tobytes() == g[a: a + n].tobytes(), (i, idx)
    r.close()


@pytest.mark.parametrize("name", mc.SECOND_UPDATE_CASES)
def test_second_update_on_dirty_scratch(name):
    """A second update back to scene0's vertices: the shape boxes, index buffers and segment lists are reused as the
    first update left them."""
    scene0, scene1 = mc.case(name)
    r = renderer(scene0)
    _update(r, name)
    assert_mesh_rebuild_bitwise(r, mc.built1(name))
    _update(r, name, 0)
    assert_mesh_rebuild_bitwise(r, scene0.desc)
    r.close()


def test_one_context_several_scenes():
    """One context: tris_2, many_meshes and tris_2 again, each uploaded and updated: the scratch and the per-mesh
    tables follow the uploaded scene."""
    r = renderer(mc.case("tris_2")[0])
    for k, name in enumerate(("tris_2", "many_meshes", "tris_2")):
        if k:
            r.upload_scene(mc.case(name)[0])
        _update(r, name)
        assert_mesh_rebuild_bitwise(r, mc.built1(name))
    r.close()


def _frames(name, options=None, wavefront=False):
    from hikari_amd import HikariSettings, Upscale, frame_inputs, load_noise
    from oracle import Oracle
    scene0, scene1 = mc.case(name)
    d1 = mc.built1(name)
    cam, lights = mc.camera_for(name)
    w, h = mc.FRAME_SIZE
    r = renderer(scene0, (w, h), options=options, wavefront=wavefront)
    _update(r, name)
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
    assert (depth > 0).mean() > 0.2  # the view covers the mesh
    lit = canon_plane(10, o.output(10)).view(np.float16).astype(np.float32)
    assert np.isfinite(lit).all()
    o.close()
    r.close()


@pytest.mark.parametrize("name", mc.FRAME_CASES)
def test_frames_after_rebuild_match_oracle(name):
    """After the array check, two 32 x 24 frames against the oracle on the host-built scene1 (the oracle sees scene0,
    then scene1; one thread, spatial reuse off, the racy scatter targets within their tolerance) and the ray counters:
    what is derived from the rebuilt BLAS (leaf boxes, wide layout, collapsed walk nodes) is what the frames walk."""
    _frames(name)


@pytest.mark.parametrize("options", [{"lds_scene": 0}, {"lds_scene": 1}, {"lds_scene": 2}, {"leaf_collapse": 0}],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", mc.VARIANT_CASES)
def test_frames_under_staging_and_collapse_options(name, options):
    _frames(name, options)


def test_frames_with_the_wavefront_pass():
    _frames("emissive_mesh", wavefront=True)


def test_traced_rays_after_the_update_equal_a_fresh_context():
    """256 seeded rays through hk_trace after the update, against a context that uploaded scene1."""
    name = "shared_mesh"
    scene0, scene1 = mc.case(name)
    mc.built1(name)
    rng = np.random.default_rng(mc.SEED)
    n = 256
    org = rng.uniform([-1.5, 0.0, 1.0], [1.5, 2.0, 4.0], (n, 3))
    d = rng.uniform([-1.5, 0.0, -0.5], [1.5, 2.0, 0.2], (n, 3)) - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d], axis=1).astype(np.float32)
    early = np.where(rng.random(n) < 0.5, 0.0, 65535.0).astype(np.float32)
    excl = rng.integers(0, len(scene1.instances) + 1, n).astype(np.uint32)
    r = renderer(scene0, mc.FRAME_SIZE)
    _update(r, name)
    fresh = renderer(scene1, mc.FRAME_SIZE)
    a, b = r.trace(rays, None, early, excl), fresh.trace(rays, None, early, excl)
    assert np.array_equal(a, b)
    assert (b[:, 3] < len(scene1.instances)).mean() > 0.3  # many of them hit
    fresh.close()
    r.close()


def _gbuffer_planes(x, fi):
    x.render_gbuffer(fi)
    return [canon_plane(oid, x.output(oid)) for oid in (11, 12, 13, 14)]


def _assert_planes(got, want, label):
    for k, (a, b) in enumerate(zip(got, want)):
        m = mismatch_report(a, b, f"{label}: output {11 + k}")
        assert not m, m


@pytest.mark.parametrize("name", ["deepen_16", "deepen_17", "shallower"])
def test_blas_depth_changed_by_an_update(name):
    """deepen_16 / deepen_17: the update turns a shallow BLAS into one that puts the stack bound on 16 (every LDS level
    of the shallow walk) and 17 (the deep walk); shallower: the deepest mesh becomes shallow and the bound is the other
    mesh's.  The G-buffer planes 11..14 after the update equal the oracle's on scene1 in the default context and under
    gbuffer_stack_full and gbuffer_deep, and a fresh context's that uploaded scene1."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    scene0, scene1 = mc.case(name)
    d1 = mc.built1(name)
    cam, lights = mc.camera_for(name)
    w, h = DEPTH_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    o = Oracle(d1, load_noise(), w, h, 1.0)
    want = _gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.005  # some of it is in view
    fresh = renderer(scene1, (w, h))
    _assert_planes(_gbuffer_planes(fresh, fi), want, f"{name} fresh")
    fresh.close()
    for opts in ({}, {"gbuffer_stack_full": 1}, {"gbuffer_deep": 1}):
        r = renderer(scene0, (w, h), options=opts)
        _update(r, name)
        assert_mesh_rebuild_bitwise(r, d1)
        _assert_planes(_gbuffer_planes(r, fi), want, f"{name} {opts}")
        r.close()
    o.close()


def test_update_to_a_blas_too_deep_and_back():
    """Stack bound 65: the update succeeds and its arrays match the host; hk_render_gbuffer then refuses with the text a
    fresh context on scene1 gives.  The update back to scene0's vertices lowers the bound again (the maximum over the
    meshes as rebuilt, not over what they have been): the G-buffer renders and matches the oracle."""
    from hikari_amd import HikariError, frame_inputs, load_noise
    from oracle import Oracle
    name = "too_deep"
    scene0, scene1 = mc.case(name)
    d1 = mc.built1(name)
    cam, lights = mc.camera_for(name)
    w, h = DEPTH_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    r = renderer(scene0, (w, h))
    _update(r, name)
    assert_mesh_rebuild_bitwise(r, d1)
    with pytest.raises(HikariError, match="too deep for the G-buffer traversal stack") as updated:
        r.render_gbuffer(fi)
    fresh = renderer(scene1, (w, h))
    with pytest.raises(HikariError, match="too deep for the G-buffer traversal stack") as uploaded:
        fresh.render_gbuffer(fi)
    assert str(updated.value) == str(uploaded.value)
    fresh.close()
    _update(r, name, 0)
    assert_mesh_rebuild_bitwise(r, scene0.desc)
    o = Oracle(scene0.desc, load_noise(), w, h, 1.0)
    want = _gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.1
    _assert_planes(_gbuffer_planes(r, fi), want, "back on scene0")
    o.close()
    r.close()


def _raw_update(r, scene, ups, count=None, models=True, aabbs=True):
    """hk_update_meshes with a hand-made list: its return code and message."""
    from hikari_amd import _abi
    m = np.ascontiguousarray(scene.instance_models(), np.float32)
    a = np.ascontiguousarray(mc.local_aabbs(scene), np.float32)
    arr = (_abi.hk_mesh_update * max(1, len(ups)))(*ups) if ups is not None else None
    rc = r._L.hk_update_meshes(r.ctx, arr, 0 if ups is None else len(ups), m.ctypes.data if models else None,
                               a.ctypes.data if aabbs else None, len(m) if count is None else count, None)
    return rc, r._L.hk_last_error(r.ctx).decode()


def test_refusals_leave_the_context_usable():
    """Every refusal of the header returns its code with a message; nothing was changed: the arrays still equal
    scene0's, and an update with scene0's own data then succeeds and matches."""
    from hikari_amd import HikariRenderer, _abi
    name = "one_of_three"
    scene0, scene1 = mc.case(name)
    keep = []

    def entry(i, vertex_count=None, index=None, positions=True, scene=scene1):
        mesh = scene.meshes[i]
        p = np.ascontiguousarray(mesh.positions, np.float32)
        n = np.ascontiguousarray(mesh.normals, np.float32)
        keep.extend([p, n])
        v, pr, n0, nc = scene.mesh_index(i) if index is None else index
        return _abi.hk_mesh_update(_abi.hk_mesh_index(v, pr, (ctypes.c_uint32 * 2)(n0, nc)),
                                   len(p) if vertex_count is None else vertex_count,
                                   p.ctypes.data if positions else None, n.ctypes.data)

    empty = HikariRenderer(0)
    rc, msg = _raw_update(empty, scene1, [entry(1)])
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()

    r = renderer(scene0)
    v, pr, n0, nc = scene1.mesh_index(1)
    nv = len(scene1.meshes[1].positions)
    top = int(scene1.meshes[1].indices.max())
    refused = [
        ("null list", dict(ups=None), "null"),
        ("null models", dict(ups=[entry(1)], models=False), "null"),
        ("null aabbs", dict(ups=[entry(1)], aabbs=False), "null"),
        ("null positions", dict(ups=[entry(1, positions=False)]), "positions"),
        ("count", dict(ups=[entry(1)], count=len(scene1.instances) - 1), "every instance"),
        ("not a mesh: vertex", dict(ups=[entry(1, index=(v + 1, pr, n0, nc))]), "not an instanced mesh"),
        ("not a mesh: primitive", dict(ups=[entry(1, index=(v, pr + 1, n0, nc))]), "not an instanced mesh"),
        ("not a mesh: node", dict(ups=[entry(1, index=(v, pr, n0 + 3, nc - 3))]), "not an instanced mesh"),
        ("too few vertices", dict(ups=[entry(1, vertex_count=top)]), "vertex indices"),
        ("into the next mesh", dict(ups=[entry(1, vertex_count=nv + 1)]), "past its vertex slice"),
        ("twice", dict(ups=[entry(1), entry(0), entry(1)]), "listed twice"),
    ]
    for label, kw, text in refused:
        rc, msg = _raw_update(r, scene1, **kw)
        assert rc == _abi.HK_ERR_INVALID and text in msg, (label, rc, msg)
        assert_mesh_rebuild_bitwise(r, scene0.desc)
    # the last mesh's vertex slice ends with the array
    last = len(scene1.meshes) - 1
    rc, msg = _raw_update(r, scene1, [entry(last, vertex_count=len(scene1.meshes[last].positions) + 1)])
    assert rc == _abi.HK_ERR_INVALID and "past its vertex slice" in msg
    _update(r, name, 0)
    assert_mesh_rebuild_bitwise(r, scene0.desc)
    _update(r, name)
    assert_mesh_rebuild_bitwise(r, mc.built1(name))
    r.close()


def test_a_mesh_whose_nodes_are_not_3k_minus_2_is_refused():
    """A scene uploaded with a mesh slice of one node less than 3k - 2: hk_update_meshes refuses that mesh, and still
    takes the other one."""
    from hikari_amd import HikariRenderer, _abi
    name = "one_of_three"
    scene0, scene1 = mc.case(name)
    d0 = scene0.desc
    inst = np.frombuffer(host_scene_array(d0, 4, np.dtype((np.void, 176))).tobytes(), np.uint32).reshape(-1, 44).copy()
    v, pr, n0, nc = scene0.mesh_index(1)
    assert inst[1, 40:44].tolist() == [v, pr, n0, nc]
    inst[1, 43] = nc - 1
    desc = _abi.hk_scene_desc.from_buffer_copy(d0)
    desc.instances.data = inst.ctypes.data
    r = HikariRenderer(0)
    r.set_noise()
    assert r._L.hk_scene_upload(r.ctx, ctypes.byref(desc)) == 0
    p = np.ascontiguousarray(scene1.meshes[1].positions, np.float32)
    up = _abi.hk_mesh_update(_abi.hk_mesh_index(v, pr, (ctypes.c_uint32 * 2)(n0, nc - 1)), len(p), p.ctypes.data, None)
    rc, msg = _raw_update(r, scene0, [up])
    assert rc == _abi.HK_ERR_INVALID and "3k - 2" in msg, (rc, msg)
    r.update_meshes(scene0, [0], local_aabbs=mc.local_aabbs(scene0))
    r.close()


def test_a_singular_model_fails_as_in_update_instances():
    from hikari_amd import HikariError
    name = "tris_129"
    scene0, scene1 = mc.case(name)
    r = renderer(scene0)
    models = scene1.instance_models().copy()
    models[0, 4:8] = 0.0  # a zero column
    with pytest.raises(HikariError, match="singular instance transform"):
        _update(r, name, models=models)
    _update(r, name)
    assert_mesh_rebuild_bitwise(r, mc.built1(name))
    r.close()


def test_update_on_a_caller_stream():
    """tris_1281 with update_meshes(..., stream=s) on a stream of the caller's, created in the HIP runtime the library
    loads (parity.hip_runtime): hk_update_meshes waits for its stream once, so the arrays are complete when it returns;
    the test synchronises s all the same."""
    name = "tris_1281"
    scene0, scene1 = mc.case(name)
    r = renderer(scene0)
    hip = hip_runtime()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    _update(r, name, stream=s)
    assert hip.hipStreamSynchronize(s) == 0
    assert_mesh_rebuild_bitwise(r, mc.built1(name))
    r.close()
    assert hip.hipStreamDestroy(s) == 0


def test_plugin_forwards_update_meshes():
    from hikari_amd import HikariPlugin
    name = "strip"
    scene0, scene1 = mc.case(name)
    p = HikariPlugin(scene0)
    p.update_meshes(scene1, mc.listed(name), local_aabbs=mc.local_aabbs(scene1))
    assert_mesh_rebuild_bitwise(p.renderer, mc.built1(name))
    p.renderer.close()
