"""hk_add_meshes: the cases of tests/mesh_add_cases.py (each proven to sit where its name says by
tests/test_mesh_add_cases.py, without a GPU) uploaded as step 0; each step's meshes appended on the GPU and then spawned
with hk_set_instances.  The appended vertices and primitives byte for byte the host builder's, the BLAS with its
topology, the earlier slices and arrays 3-8 untouched by the add, everything the instance rebuild derives afterwards;
frames, G-buffers, traced rays and counters against the CPU oracle on the host-built scenes.
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.

The branch of csrc/hk_dynamic.hip or csrc/hk_runtime.hip each case exists for is listed in mesh_add_cases.py."""
import numpy as np
import pytest

import instance_set_cases as ic
import mesh_add_cases as ac
from parity import assert_rebuild_bitwise, renderer
from scene_edits import (DEPTH_SIZE, ELEM_DT, EditFrames, assert_mesh_arrays, assert_planes, assert_traces_equal_fresh,
                         caller_stream, device_arrays, gbuffer_planes, raw_call)

pytestmark = pytest.mark.gpu


def _add_and_check(r, name, k):
    """Step k's hk_add_meshes alone: the returned slices are the host's, arrays 0-2 the host's for the pool with the
    new meshes, their earlier elements and arrays 3-8 byte for byte what the device held before, counts 3-8 too."""
    counts = r.scene_counts()
    old_low, old_high = device_arrays(r, range(3)), device_arrays(r, range(3, 9))
    slices = ac.add(r, name, k)
    assert slices == [tuple(int(x) for x in s) for s in ac.new_slices(name, k)]
    desc = ac.add_only(name, k).desc
    assert r.scene_counts() == ic.desc_counts(desc) and r.scene_counts()[3:] == counts[3:]
    assert_mesh_arrays(r, desc, ac.added_so_far(name, k))
    for i, before in enumerate(old_low):
        now = r.scene_array(i, ELEM_DT[i], r.scene_counts()[i])
        assert now[:counts[i]].tobytes() == before, f"array {i}: an earlier slice changed"
    assert device_arrays(r, range(3, 9)) == old_high
    assert_rebuild_bitwise(r, ac.built(name, k - 1))


def _set_and_check(r, name, k, stream=None):
    ac.spawn(r, name, k, stream)
    desc = ac.built(name, k)
    assert r.scene_counts() == ic.desc_counts(desc)
    assert_rebuild_bitwise(r, desc)
    assert_mesh_arrays(r, desc, ac.added_so_far(name, k))


@pytest.mark.parametrize("name", list(ac.CASES))
def test_added_and_spawned_arrays_match_host_builder(name):
    """Upload step 0; for every step the add alone (arrays 0-2 the host's, everything else as it was), then the set
    (all nine arrays and counts the host build's for that step)."""
    c = ac.case(name)
    r = renderer(c.scenes[0])
    for k in list(ac.steps(name))[1:]:
        _add_and_check(r, name, k)
        _set_and_check(r, name, k)
    if c.update is not None:
        scene, ids = c.update
        r.update_meshes(scene, ids, local_aabbs=ac.local_aabbs(scene))
        desc = ac.built_update(name)
        assert r.scene_counts() == ic.desc_counts(desc)
        assert_rebuild_bitwise(r, desc)
        assert_mesh_arrays(r, desc, ac.added_so_far(name, len(c.scenes) - 1))
    r.close()


# ------------------------------------------------------------------ capacity
def _grown(need, cap):
    return max(need, cap + cap // 2)


def test_capacity_grows_keeps_and_resets():
    """three_calls: the capacities of arrays 0-2 follow the header's rule (counts against capacities): they grow in
    the first and second call and do not move in the third; hk_set_instances' arrays are not touched by an add; a
    re-upload resets them to the counts."""
    name = "three_calls"
    c = ac.case(name)
    r = renderer(c.scenes[0])
    counts, cap = r.scene_counts(), r.scene_capacity()
    assert cap == [max(1, n) for n in counts]
    seen = [cap]
    for k in list(ac.steps(name))[1:]:
        before = r.scene_capacity()
        ac.add(r, name, k)
        after, counts = r.scene_capacity(), r.scene_counts()
        assert all(n <= m for n, m in zip(counts, after))
        assert after[:3] == [m if n <= m else _grown(n, m) for n, m in zip(counts[:3], before[:3])]
        assert after[3:] == before[3:]
        seen.append(after)
        _set_and_check(r, name, k)
        assert r.scene_capacity()[:3] == after[:3]
    assert all(b > a for a, b in zip(seen[0][:3], seen[1][:3]))
    assert all(b > a for a, b in zip(seen[1][:3], seen[2][:3]))
    assert seen[3][:3] == seen[2][:3] and all(n < m for n, m in zip(r.scene_counts()[:3], seen[3][:3]))
    r.upload_scene(c.scenes[0])
    assert r.scene_capacity() == [max(1, n) for n in ic.desc_counts(c.scenes[0].desc)]
    _add_and_check(r, name, 1)
    _set_and_check(r, name, 1)
    r.close()


# ------------------------------------------------------------------ frames
def _frames(name, options=None, wavefront=False, after_add=False):
    """Per step: the add (after_add: then two 32 x 24 frames against the oracle still on the scene before, the picture
    being untouched), the set, and two frames against the oracle on the host-built scene (Oracle.set_scene; one thread,
    spatial reuse off, the racy scatter targets within their tolerance); equal ray counters at the end."""
    with EditFrames(ac.case(name).scenes[0], ac.camera_for(name), ac.FRAME_SIZE, floor=0.05, finite=True,
                     options=options, wavefront=wavefront) as fr:
        for k in list(ac.steps(name))[1:]:
            _add_and_check(fr.r, name, k)
            if after_add:
                fr.frames(2, f"step {k} after the add")
            _set_and_check(fr.r, name, k)
            fr.set_scene(ac.built(name, k))
            fr.frames(2, f"step {k} after the set")


@pytest.mark.parametrize("name", [n for n in ac.FRAME_CASES if n != "stage_edge_add"])
def test_frames_after_add_and_spawn_match_oracle(name):
    _frames(name, after_add=name == "emissive_new")


@pytest.mark.parametrize("options", ac.STAGE_OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_frames_across_the_staging_limit(options):
    """stage_edge_add: the add alone takes the light plan out of LDS staging (the staging decision follows the counts
    of arrays 0-2); the frames after it equal the oracle's on the scene before, those after the spawn the new one's."""
    _frames("stage_edge_add", options, after_add=True)


@pytest.mark.parametrize("name", ac.NO_COLLAPSE_CASES)
def test_frames_without_leaf_collapse(name):
    _frames(name, {"leaf_collapse": 0})


def test_frames_with_the_wavefront_pass():
    _frames(ac.WAVEFRONT_CASE, wavefront=True)


# ------------------------------------------------------------------ stack bound
def test_stack_bound_moves_with_the_spawn_not_the_add():
    """deep_new: the G-buffer planes after the add equal the oracle's on the scene before (a deep mesh nobody carries
    leaves the bound alone), those after the spawn the oracle's on the new scene, whose bound is 17: in the default
    context and under gbuffer_stack_full and gbuffer_deep.  The context offers no read-back of the bound itself: the
    equality of the planes under the three walk variants the bound selects among is the proxy for it."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    name = "deep_new"
    c = ac.case(name)
    cam, lights = ac.camera_for(name)
    w, h = DEPTH_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    o = Oracle(c.scenes[0].desc, load_noise(), w, h, 1.0)
    before = gbuffer_planes(o, fi)
    o.set_scene(ac.built(name, 1))
    after = gbuffer_planes(o, fi)
    assert any((a != b).any() for a, b in zip(before, after))  # the new mesh is in view
    o.close()
    for opts in ac.STACK_OPTIONS:
        r = renderer(c.scenes[0], (w, h), options=opts)
        assert_planes(gbuffer_planes(r, fi), before, f"{opts} uploaded")
        _add_and_check(r, name, 1)
        assert_planes(gbuffer_planes(r, fi), before, f"{opts} after the add")
        _set_and_check(r, name, 1)
        assert_planes(gbuffer_planes(r, fi), after, f"{opts} after the spawn")
        r.close()


# ------------------------------------------------------------------ rays
def test_traced_rays_after_add_and_spawn_equal_a_fresh_context():
    """256 seeded rays through hk_trace after add + spawn, against a context that uploaded the final scene."""
    name = "strip_odd"
    c = ac.case(name)
    final = c.scenes[1]
    ac.built(name, 1)
    r = renderer(c.scenes[0], ac.FRAME_SIZE)
    ac.add(r, name, 1)
    ac.spawn(r, name, 1)
    fresh = renderer(final, ac.FRAME_SIZE)
    b = assert_traces_equal_fresh(r, fresh, ac.SEED, len(final.instances))
    new = {len(final.instances) - 1, len(final.instances) - 2}
    assert np.isin(b[:, 3], list(new)).any()  # some of them a new mesh
    fresh.close()
    r.close()


# ------------------------------------------------------------------ refusals
def _raw_add(r, descs, n=None, slices=True):
    """hk_add_meshes with a hand-made list: its return code and message."""
    from hikari_amd import _abi
    count = len(descs) if n is None and descs is not None else (n or 0)
    arr = (_abi.hk_mesh_desc * max(1, count))(*(descs or [])) if descs is not None else None
    out = (_abi.hk_mesh_index * max(1, count))()
    return raw_call(r, "hk_add_meshes", arr, count, out if slices else None, None)


def test_refusals_leave_the_context_usable():
    """Every refusal of the header returns its code with hks_add_mesh's error in the message; nothing was changed:
    arrays 0-2, the counts and the capacities are the uploaded scene's, and a valid call then matches the host."""
    from hikari_amd import HikariRenderer, _abi
    from test_mesh_add_cases import refusals
    name = "pool_tail"
    c = ac.case(name)
    keep = []
    cases = refusals(keep)
    good = cases[2][1][:1]
    empty = HikariRenderer(0)
    rc, msg = _raw_add(empty, good)
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()
    r = renderer(c.scenes[0])
    cap = r.scene_capacity()
    for label, descs, n, text in cases + [("null slices", good, None, "null slices")]:
        rc, msg = _raw_add(r, descs, n, slices=label != "null slices")
        assert rc == _abi.HK_ERR_INVALID and text in msg and "hk_add_meshes" in msg, (label, rc, msg)
        assert r.scene_counts() == ic.desc_counts(c.scenes[0].desc) and r.scene_capacity() == cap
        assert_mesh_arrays(r, c.scenes[0].desc, [])
    assert_rebuild_bitwise(r, c.scenes[0].desc)
    _add_and_check(r, name, 1)
    _set_and_check(r, name, 1)
    r.close()


# ------------------------------------------------------------------ stream, plugin
def test_add_on_a_caller_stream():
    """tris_1281 with add_meshes(..., stream=s) and set_instances on a stream of the caller's
    (scene_edits.caller_stream): hk_add_meshes waits for its stream once, so the arrays are complete when it returns;
    the test synchronises s all the same."""
    name = "tris_1281"
    r = renderer(ac.case(name).scenes[0])
    with caller_stream() as (s, sync):
        assert ac.add(r, name, 1, stream=s) == [tuple(int(x) for x in v) for v in ac.new_slices(name, 1)]
        sync()
        assert_mesh_arrays(r, ac.add_only(name, 1).desc, ac.added_so_far(name, 1))
        _set_and_check(r, name, 1, stream=s)
        sync()
        r.close()


def test_plugin_forwards_add_meshes():
    from hikari_amd import HikariPlugin
    name = "shared_vertices"
    c = ac.case(name)
    p = HikariPlugin(c.scenes[0])
    assert p.add_meshes(c.new[1]) == [tuple(int(x) for x in v) for v in ac.new_slices(name, 1)]
    assert_mesh_arrays(p.renderer, ac.add_only(name, 1).desc, ac.added_so_far(name, 1))
    p.set_instances(c.scenes[1], previous=c.previous[1])
    assert p.renderer.scene_counts() == ic.desc_counts(ac.built(name, 1))
    assert_rebuild_bitwise(p.renderer, ac.built(name, 1))
    p.renderer.close()
