"""hk_update_meshes at its size, shape and depth edges: the cases of tests/mesh_cases.py (each proven to sit on its edge
by tests/test_mesh_cases.py, without a GPU) uploaded as scene0, updated to scene1's vertices, and the rewritten vertex
and primitive arrays, the rebuilt BLAS and everything the instance rebuild derives from them compared byte for byte with
the host builder's; frames, G-buffers, traced rays and counters against the CPU oracle on the host-built scene1.  The
shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.

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
from parity import host_scene_array, renderer
from scene_edits import (DEPTH_SIZE, INST_DT, EditFrames, assert_mesh_rebuild_bitwise, assert_planes,
                         assert_slices_kept, assert_traces_equal_fresh, caller_stream, gbuffer_planes, models_and_aabbs,
                         ptr, raw_call, raw_renderer)

pytestmark = pytest.mark.gpu


def _update(r, name, which=1, stream=None, **kw):
    scene = mc.update_source(name, which)
    r.update_meshes(scene, mc.listed(name), local_aabbs=mc.local_aabbs(scene), stream=stream, **kw)


@pytest.mark.parametrize("name", mc.ARRAY_CASES)
def test_rebuilt_arrays_match_host_builder(name):
    """Upload scene0, update the listed meshes to scene1's vertices: every array equals the host builder's for scene1,
    the BLAS topology included.  one_of_three: the unlisted meshes' slices also equal scene0's."""
    scene0, scene1 = mc.case(name)
    r = renderer(scene0)
    _update(r, name)
    assert_mesh_rebuild_bitwise(r, mc.built1(name))
    if name == "one_of_three":
        assert_slices_kept(r, scene0, (0, 2))
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
    scene0, scene1 = mc.case(name)
    d1 = mc.built1(name)
    with EditFrames(scene0, mc.camera_for(name), mc.FRAME_SIZE, floor=0.2, finite=True, options=options,
                     wavefront=wavefront) as fr:
        _update(fr.r, name)
        assert_mesh_rebuild_bitwise(fr.r, d1)
        fr.set_scene(d1)
        fr.frames(2)


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
    r = renderer(scene0, mc.FRAME_SIZE)
    _update(r, name)
    fresh = renderer(scene1, mc.FRAME_SIZE)
    assert_traces_equal_fresh(r, fresh, mc.SEED, len(scene1.instances))
    fresh.close()
    r.close()


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
    want = gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.005  # some of it is in view
    fresh = renderer(scene1, (w, h))
    assert_planes(gbuffer_planes(fresh, fi), want, f"{name} fresh")
    fresh.close()
    for opts in ({}, {"gbuffer_stack_full": 1}, {"gbuffer_deep": 1}):
        r = renderer(scene0, (w, h), options=opts)
        _update(r, name)
        assert_mesh_rebuild_bitwise(r, d1)
        assert_planes(gbuffer_planes(r, fi), want, f"{name} {opts}")
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
    want = gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.1
    assert_planes(gbuffer_planes(r, fi), want, "back on scene0")
    o.close()
    r.close()


def _raw_update(r, scene, ups, count=None, models=True, aabbs=True):
    """hk_update_meshes with a hand-made list: its return code and message."""
    from hikari_amd import _abi
    m, a = models_and_aabbs(scene)
    arr = (_abi.hk_mesh_update * max(1, len(ups)))(*ups) if ups is not None else None
    return raw_call(r, "hk_update_meshes", arr, 0 if ups is None else len(ups), ptr(m, models), ptr(a, aabbs),
                    len(m) if count is None else count, None)


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
    from hikari_amd import _abi
    name = "one_of_three"
    scene0, scene1 = mc.case(name)
    d0 = scene0.desc
    inst = np.frombuffer(host_scene_array(d0, 4, INST_DT).tobytes(), np.uint32).reshape(-1, 44).copy()
    v, pr, n0, nc = scene0.mesh_index(1)
    assert inst[1, 40:44].tolist() == [v, pr, n0, nc]
    inst[1, 43] = nc - 1
    desc = _abi.hk_scene_desc.from_buffer_copy(d0)
    desc.instances.data = inst.ctypes.data
    r = raw_renderer(desc)
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
    """tris_1281 with update_meshes(..., stream=s) on a stream of the caller's (scene_edits.caller_stream):
    hk_update_meshes waits for its stream once, so the arrays are complete when it returns; the test synchronises s all
    the same."""
    name = "tris_1281"
    scene0, scene1 = mc.case(name)
    r = renderer(scene0)
    with caller_stream() as (s, sync):
        _update(r, name, stream=s)
        sync()
        assert_mesh_rebuild_bitwise(r, mc.built1(name))
        r.close()


def test_plugin_forwards_update_meshes():
    from hikari_amd import HikariPlugin
    name = "strip"
    scene0, scene1 = mc.case(name)
    p = HikariPlugin(scene0)
    p.update_meshes(scene1, mc.listed(name), local_aabbs=mc.local_aabbs(scene1))
    assert_mesh_rebuild_bitwise(p.renderer, mc.built1(name))
    p.renderer.close()
