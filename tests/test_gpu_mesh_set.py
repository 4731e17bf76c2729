"""hk_set_meshes: the cases of tests/mesh_set_cases.py (each proven to sit where its name says by
tests/test_mesh_set_cases.py, without a GPU) uploaded as step 0; each step's mesh list and instance set given to the GPU
in one call.  The returned slices, all nine counts and all nine arrays byte for byte the host builder's for that step;
frames, G-buffers, motion vectors, traced rays and counters against the CPU oracle on the host-built scenes.
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.

The branch of csrc/hk_dynamic.hip or csrc/hk_runtime.hip each case exists for is listed in mesh_set_cases.py."""
import numpy as np
import pytest

import instance_set_cases as ic
import mesh_set_cases as sc
from parity import renderer
from scene_edits import (DEPTH_SIZE, MOTION_PLANES, EditFrames, assert_mesh_arrays, assert_planes, assert_scene_is,
                         assert_traces_equal_fresh, caller_stream, device_arrays, gbuffer_planes, ptr, raw_call)

pytestmark = pytest.mark.gpu


def _step_and_check(r, name, k, stream=None):
    """Step k's call: the returned slices are the host's, and every listed slice is registered, so every leaf carries
    its box."""
    assert sc.step(r, name, k, stream) == sc.host_slices(name, k)
    assert_scene_is(r, sc.built(name, k), sc.host_slices(name, k))


def _after_and_check(r, name):
    c = sc.case(name)
    last = len(c.scenes) - 1
    registered = sc.host_slices(name, last)
    kind = c.after[0]
    if kind == "add":
        _, new, scene = c.after
        got = r.add_meshes(new)
        assert got == [scene.mesh_index(i) for i in range(len(scene.meshes) - len(new), len(scene.meshes))]
        where = {key: i for i, key in enumerate(c.scenes[last].keys)}
        r.set_instances(scene, previous=[where.get(key) for key in scene.keys], local_aabbs=sc.local_aabbs(scene))
        registered = registered + got
    elif kind == "update":
        _, scene, ids = c.after
        r.update_meshes(scene, ids, local_aabbs=sc.local_aabbs(scene))
    else:
        _, scene, previous = c.after
        r.set_instances(scene, previous=previous, local_aabbs=sc.local_aabbs(scene))
    assert_scene_is(r, sc.built_after(name), registered)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_arrays_after_every_step_match_host_builder(name):
    """Upload step 0; after every step all nine arrays and counts are the host build's for that step; then the case's
    `after` call, if any, leaves the host build's arrays too."""
    c = sc.case(name)
    r = renderer(c.scenes[0])
    for k in list(sc.steps(name))[1:]:
        _step_and_check(r, name, k)
    if c.after is not None:
        _after_and_check(r, name)
    r.close()


def test_identity_keeps_every_byte():
    name = "identity"
    r = renderer(sc.case(name).scenes[0])
    before = device_arrays(r)
    _step_and_check(r, name, 1)
    now = device_arrays(r)
    # (array 2's leaves: the quad's and both meshes' were registered by the upload already; the TLAS's too)
    assert now == before
    r.close()


# ------------------------------------------------------------------ capacity
def test_capacity_never_falls_and_the_second_call_fits():
    """shrink_then_grow: the counts of arrays 0-2 fall in the first step and rise in the second, below the uploaded
    ones; the capacities (counts against capacities, as the header puts it) stay what the upload left in both.  A
    re-upload resets them to the counts."""
    name = "shrink_then_grow"
    c = sc.case(name)
    r = renderer(c.scenes[0])
    cap = r.scene_capacity()
    assert cap == [max(1, n) for n in r.scene_counts()]
    for k in (1, 2):
        _step_and_check(r, name, k)
        assert r.scene_capacity()[:3] == cap[:3]
        assert all(n < m for n, m in zip(r.scene_counts()[:3], cap[:3]))
    r.upload_scene(c.scenes[0])
    assert r.scene_capacity() == [max(1, n) for n in ic.desc_counts(c.scenes[0].desc)]
    _step_and_check(r, name, 1)
    r.close()


def test_capacity_grows_by_the_rule_and_back_and_forth_fits():
    """insert_front grows all three arrays: max(count, 1.5 x capacity); swapping back to the base list and forth again
    fits, and leaves the host's arrays each time."""
    name = "insert_front"
    c = sc.case(name)
    r = renderer(c.scenes[0])
    before = r.scene_capacity()
    _step_and_check(r, name, 1)
    counts, grown = r.scene_counts(), r.scene_capacity()
    assert grown[:3] == [max(n, m + m // 2) for n, m in zip(counts[:3], before[:3])]
    s0, s1 = c.scenes
    back = [(s1.mesh_index(k), len(m.positions)) for k, m in enumerate(s1.meshes) if any(m is o for o in s0.meshes)]
    where = {key: i for i, key in enumerate(s1.keys)}
    got = r.set_meshes(s0, back, previous=[where.get(key) for key in s0.keys], local_aabbs=sc.local_aabbs(s0))
    assert got == sc.host_slices(name, 0)
    assert_scene_is(r, sc.built(name, 0), got)
    assert r.scene_capacity()[:3] == grown[:3]
    _step_and_check(r, name, 1)
    assert r.scene_capacity()[:3] == grown[:3]
    r.close()


# ------------------------------------------------------------------ frames
def _frames(name, options=None, wavefront=False):
    """Two 32 x 24 frames on step 0, then two after each step, against the oracle on the host-built scene
    (Oracle.set_scene; one thread, spatial reuse off, the racy scatter targets within their tolerance), the reservoir
    history carried across the steps; equal ray counters at the end.  Where a survivor moves (replace_*) the instance
    count stays, so the oracle's previous models by index and the call's `previous` agree."""
    with EditFrames(sc.case(name).scenes[0], sc.camera_for(name), sc.FRAME_SIZE, floor=0.05, finite=True,
                     options=options, wavefront=wavefront) as fr:
        for k in sc.steps(name):
            if k:
                _step_and_check(fr.r, name, k)
                fr.set_scene(sc.built(name, k))
            fr.frames(2, f"step {k}")


@pytest.mark.parametrize("name", sc.FRAME_CASES)
def test_frames_after_each_step_match_oracle(name):
    _frames(name)


@pytest.mark.parametrize("options", sc.STAGE_OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_frames_across_the_staging_limit(options):
    """stage_edge_drop: the drop alone brings the light plan back within LDS staging (the staging decision follows the
    counts of arrays 0-2)."""
    _frames("stage_edge_drop", options)


@pytest.mark.parametrize("name", sc.NO_COLLAPSE_CASES)
def test_frames_without_leaf_collapse(name):
    _frames(name, {"leaf_collapse": 0})


def test_frames_with_the_wavefront_pass():
    _frames(sc.WAVEFRONT_CASE, wavefront=True)


# ------------------------------------------------------------------ motion vectors, stack bound
@pytest.mark.parametrize("name", list(sc.REPLACE))
def test_motion_vectors_span_a_replacement(name):
    """The replaced mesh's instance moves in the step and carries `previous`: the G-buffer after the call, velocity
    plane (15) included, equals the oracle's, which keeps the previous models by index while the count stays."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    c = sc.case(name)
    cam, lights = sc.camera_for(name)
    w, h = sc.FRAME_SIZE
    fis = [frame_inputs(f, cam, lights, w, h) for f in (0, 1)]
    o = Oracle(c.scenes[0].desc, load_noise(), w, h, 1.0)
    gbuffer_planes(o, fis[0], MOTION_PLANES)
    o.set_scene(sc.built(name, 1))
    want = gbuffer_planes(o, fis[1], MOTION_PLANES)
    velocity = want[4].view(np.float32).reshape(h, w, 4)[..., :2]
    assert (velocity != 0).any()  # the moving instance is in view
    r = renderer(c.scenes[0], (w, h))
    gbuffer_planes(r, fis[0], MOTION_PLANES)
    _step_and_check(r, name, 1)
    assert_planes(gbuffer_planes(r, fis[1], MOTION_PLANES), want, name)
    o.close()
    r.close()


def test_stack_bound_falls_with_the_drop():
    """deep_dropped: the G-buffer planes before equal the oracle's on the base scene, whose bound is 17, those after
    the oracle's on the scene without the deep mesh: in the default context and under gbuffer_stack_full and
    gbuffer_deep (the walk variants the bound selects among)."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    name = "deep_dropped"
    c = sc.case(name)
    cam, lights = sc.camera_for(name)
    w, h = DEPTH_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    o = Oracle(c.scenes[0].desc, load_noise(), w, h, 1.0)
    before = gbuffer_planes(o, fi)
    o.set_scene(sc.built(name, 1))
    after = gbuffer_planes(o, fi)
    assert any((a != b).any() for a, b in zip(before, after))  # the deep mesh was in view
    o.close()
    for opts in sc.STACK_OPTIONS:
        r = renderer(c.scenes[0], (w, h), options=opts)
        assert_planes(gbuffer_planes(r, fi), before, f"{opts} uploaded")
        _step_and_check(r, name, 1)
        assert_planes(gbuffer_planes(r, fi), after, f"{opts} after the drop")
        r.close()


# ------------------------------------------------------------------ rays
def test_traced_rays_after_a_step_equal_a_fresh_context():
    """256 seeded rays through hk_trace after many_meshes' step, against a context that uploaded the final scene."""
    name = "many_meshes"
    c = sc.case(name)
    final = c.scenes[1]
    sc.built(name, 1)
    r = renderer(c.scenes[0], sc.FRAME_SIZE)
    sc.step(r, name, 1)
    fresh = renderer(final, sc.FRAME_SIZE)
    b = assert_traces_equal_fresh(r, fresh, sc.SEED, len(final.instances), top=3.0)
    assert (b[:, 3][b[:, 3] < len(final.instances)] >= 2).any()  # some of them a mesh of the rack
    fresh.close()
    r.close()


# ------------------------------------------------------------------ refusals
def _raw_set(r, entries, n, descs, count, models, aabbs, slices=True):
    """hk_set_meshes with hand-made arguments: its return code and message."""
    from hikari_amd import _abi
    out = (_abi.hk_mesh_index * max(1, n))()
    return raw_call(r, "hk_set_meshes", entries, n, out if slices else None, descs, ptr(models), ptr(aabbs), count, None,
                    None)


def test_refusals_leave_the_context_usable():
    """Every refusal of the header returns its code and message and changes nothing: the nine arrays, the counts and
    the capacities are the uploaded scene's and the G-buffer's picture is what it was; a valid call then matches the
    host."""
    from hikari_amd import HikariRenderer, _abi, frame_inputs, instance_descs
    from hikari_amd.plugin import _mesh_entries
    from test_mesh_set_cases import kept, new
    from test_mesh_add_cases import refusals as add_refusals
    name = "pooled_kept"
    c = sc.case(name)
    s0, s1 = c.scenes
    q, a, u1, u2 = (s0.mesh_index(k) for k in range(4))
    nv = [len(m.positions) for m in s0.meshes]
    need_a = int(np.asarray(s0.meshes[1].indices).max()) + 1
    good, hold = _mesh_entries(sc.entries(name, 1))
    n_good = len(s1.meshes)
    models = np.ascontiguousarray(s1.instance_models(), np.float32).reshape(-1, 16)
    aabbs = np.ascontiguousarray(sc.local_aabbs(s1), np.float32).reshape(-1, 6)
    set1, n1 = instance_descs(s1, c.previous[1]), len(s1.instances)

    def arr(entries):
        from hikari_amd import _abi
        return (_abi.hk_mesh_entry * max(1, len(entries)))(*entries), len(entries)

    keep = []
    lists = [("null list", None, 1, "null mesh list"), ("no meshes", arr([])[0], 0, "empty mesh list")]
    for label, descs, n, text in add_refusals(keep)[2:]:
        lists.append((label, *arr([kept(*q, nv[0])] + [new(d, keep) for d in descs]), text.replace("mesh 1", "mesh 2")))
    lists += [
        ("not 3k - 2", *arr([kept(q[0], q[1], q[2], q[3] + 1, nv[0])]), "kept slice refused: its BLAS is not 3k - 2"),
        ("part of a known slice", *arr([kept(a[0], a[1] + 1, a[2] + 3, a[3] - 3, nv[1])]),
         "mesh 0: kept slice refused: it partly overlaps another mesh slice"),
        ("nodes past", *arr([kept(u2[0], u2[1], u2[2] + 3, u2[3], nv[3])]), "kept slice refused: its nodes reach past"),
        ("below vertex_need", *arr([kept(*q, nv[0]), kept(*a, need_a - 1)]), "mesh 1: vertex_count does not cover"),
        ("past the vertex array", *arr([kept(*u2, nv[3] + 1)]), "vertex_count reaches past the vertex array"),
        ("into another kept slice", *arr([kept(*a, nv[1] + 1), kept(*u1, nv[2])]),
         "mesh 1: vertex_count reaches into another kept slice's vertices"),
        ("kept twice", *arr([kept(*q, nv[0]), kept(*a, nv[1]), kept(*q, nv[0])]), "mesh 2: the slice is kept twice"),
    ]
    bad_material = instance_descs(s1, c.previous[1])
    bad_material[1].material = 999
    sets = [
        ("mesh not in the list", instance_descs(s0, None), len(s0.instances), "its mesh is not in the new list"),
        ("previous out of range", instance_descs(s1, [99] * n1), n1, "previous is not an index of the set before"),
        ("previous twice", instance_descs(s1, [0] * n1), n1, "previous is used twice"),
        ("material", bad_material, n1, "instance 1: material index out of range"),
        ("empty set", set1, 0, "an empty instance set"),
        ("null set", None, n1, "null pointer"),
    ]
    empty = HikariRenderer(0)
    rc, msg = _raw_set(empty, good, n_good, set1, n1, models, aabbs)
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()

    cam, lights = sc.camera_for(name)
    w, h = sc.FRAME_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    r = renderer(s0, (w, h))
    picture = gbuffer_planes(r, fi, MOTION_PLANES)
    cap, arrays = r.scene_capacity(), device_arrays(r)

    def unchanged(label):
        assert r.scene_counts() == ic.desc_counts(s0.desc) and r.scene_capacity() == cap, label
        assert device_arrays(r) == arrays, label
        assert_planes(gbuffer_planes(r, fi, MOTION_PLANES), picture, label)

    for label, entries, n, text in lists:
        m_, a_ = models[: len(s0.instances)], aabbs[: len(s0.instances)]
        rc, msg = _raw_set(r, entries, n, instance_descs(s0, None), len(s0.instances), m_, a_)
        assert rc == _abi.HK_ERR_INVALID and text in msg and "hk_set_meshes" in msg, (label, rc, msg)
        unchanged(label)
    for label, descs, count, text in sets:
        rc, msg = _raw_set(r, good, n_good, descs, count, models, aabbs)
        assert rc == _abi.HK_ERR_INVALID and text in msg and "hk_set_meshes" in msg, (label, rc, msg)
        unchanged(label)
    rc, msg = _raw_set(r, good, n_good, set1, n1, models, aabbs, slices=False)
    assert rc == _abi.HK_ERR_INVALID and "null slices" in msg
    rc, msg = _raw_set(r, good, n_good, set1, n1, None, aabbs)
    assert rc == _abi.HK_ERR_INVALID and "null pointer" in msg
    unchanged("null pointers")
    assert_planes(gbuffer_planes(r, fi, MOTION_PLANES), picture, "after the refusals")
    assert_mesh_arrays(r, s0.desc, [])
    _step_and_check(r, name, 1)
    r.close()


# ------------------------------------------------------------------ stream, plugin
def test_set_on_a_caller_stream():
    """replace_across_lds with set_meshes(..., stream=s) on a stream of the caller's (scene_edits.caller_stream): the
    call waits for its stream, so the arrays are complete when it returns; the test synchronises s all the same."""
    name = "replace_across_lds"
    r = renderer(sc.case(name).scenes[0])
    with caller_stream() as (s, sync):
        _step_and_check(r, name, 1, stream=s)
        sync()
        r.close()


def test_plugin_forwards_set_meshes():
    from hikari_amd import HikariPlugin
    name = "drop_middle"
    c = sc.case(name)
    p = HikariPlugin(c.scenes[0])
    got = p.set_meshes(c.scenes[1], sc.entries(name, 1), previous=c.previous[1])
    assert got == sc.host_slices(name, 1)
    assert_scene_is(p.renderer, sc.built(name, 1), got)
    p.renderer.close()
