"""hk_set_instances: the cases of tests/instance_set_cases.py (each proven to sit where its name says by
tests/test_instance_set_cases.py, without a GPU) uploaded as step 0 and set to each later step; the rebuilt alias table,
instances, TLAS, light BVH and emissives compared byte for byte with the host builder's, the counts with its desc's,
frames, G-buffers and counters against the CPU oracle on the host-built scene.
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.

The branch of csrc/hk_dynamic.hip or csrc/hk_runtime.hip each case exists for is listed in instance_set_cases.py."""
import copy
import ctypes
import gc

import numpy as np
import pytest

import instance_set_cases as ic
from parity import hip_runtime, renderer
from scene_edits import (MOTION_PLANES, EditFrames, assert_mesh_rebuild_bitwise, assert_planes, assert_scene_is,
                         gbuffer_planes, raw_call)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ic.CASES))
def test_rebuilt_arrays_match_host_builder(name):
    """Upload step 0, then set every later step in turn: after each the arrays and counts equal the host builder's
    for that step (three-step cases come back or go on over grown, dirty buffers and scratch)."""
    c = ic.case(name)
    r = renderer(c.scenes[0])
    assert r.scene_counts() == ic.desc_counts(c.scenes[0].desc)
    for k in list(ic.steps(name))[1:]:
        ic.apply(r, name, k)
        assert_scene_is(r, ic.built(name, k), meshes=False, materials=c.materials)
    r.close()


def test_one_context_another_upload_resets_the_capacity():
    """from_one_129 grows every array; uploading to_one's scene and setting its step on the same context starts from
    that upload's sizes."""
    r = renderer(ic.case("from_one_129").scenes[0])
    ic.apply(r, "from_one_129", 1)
    assert_scene_is(r, ic.built("from_one_129", 1), meshes=False, materials=False)
    r.upload_scene(ic.case("to_one").scenes[0])
    ic.apply(r, "to_one", 1)
    assert_scene_is(r, ic.built("to_one", 1), meshes=False, materials=False)
    r.close()


# ------------------------------------------------------------------ frames
def _frames(name, options=None):
    """Two 32 x 24 frames on step 0, then two after each set, against the oracle (Oracle.set_scene with the host-built
    desc; one thread, spatial reuse off): the racy scatter targets within their tolerance, everything else bit-exact,
    and equal ray counters.  No survivor moves in these cases, so the oracle's restart of the previous models on a
    changed count and the mapping agree."""
    c = ic.case(name)
    with EditFrames(c.scenes[0], ic.camera_for(name), ic.FRAME_SIZE, floor=0.05, options=options) as fr:
        for k in ic.steps(name):
            if k:
                ic.apply(fr.r, name, k)
                assert_scene_is(fr.r, ic.built(name, k), meshes=False, materials=c.materials)
                fr.set_scene(ic.built(name, k))
            fr.frames(2, f"step {k}")


@pytest.mark.parametrize("name", [n for n in ic.FRAME_CASES if n not in ("stage_edge", "deeper_blas")])
def test_frames_before_and_after_match_oracle(name):
    _frames(name)


@pytest.mark.parametrize("options", ic.STAGE_OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_frames_across_the_staging_limit(options):
    _frames("stage_edge", options)


@pytest.mark.parametrize("options", ic.STACK_OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
def test_frames_across_the_lds_stack_levels(options):
    _frames("deeper_blas", options)


# ------------------------------------------------------------------ previous models
def _moved_copy(scene, seed):
    """The scene's pool and instance list with every instance moved a little (seeded)."""
    rng = np.random.default_rng(seed)
    out = copy.copy(scene)
    out._h, out.desc = None, None
    out.instances = []
    for mesh, mat, m in scene.instances:
        t = np.eye(4)
        t[:3, 3] = rng.uniform(-0.15, 0.15, 3)
        out.instances.append((mesh, mat, t @ m))
    return out


@pytest.mark.parametrize("name", ["despawn_middle", "spawn_copies"])
def test_previous_models_follow_the_mapping(name):
    """A despawn with moving survivors, and a spawn beside moving survivors.  The oracle keeps previous models by index
    while the count stays, so it runs one G-buffer on P (the new instance list, the survivors with their old models, the
    new entities with their current ones) and then takes the new scene; the GPU uploads the old scene, renders one
    G-buffer and sets the new list with the mapping.  The next G-buffer's planes 11..15 (15: velocity) are equal."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    c = ic.case(name)
    old, previous = c.scenes[0], c.previous[1]
    new = _moved_copy(c.scenes[1], [ic.SEED, 77])
    p = copy.copy(new)
    p._h, p.desc = None, None
    p.instances = [(mesh, mat, m if previous[i] is None else old.instances[previous[i]][2])
                   for i, (mesh, mat, m) in enumerate(new.instances)]
    cam, lights = ic.camera_for(name)
    w, h = ic.FRAME_SIZE
    fis = [frame_inputs(f, cam, lights, w, h) for f in (0, 1)]
    o = Oracle(p.build(), load_noise(), w, h, 1.0)
    gbuffer_planes(o, fis[0], MOTION_PLANES)
    o.set_scene(new.build())
    want = gbuffer_planes(o, fis[1], MOTION_PLANES)
    velocity = want[4].view(np.float32).reshape(h, w, 4)[..., :2]
    assert (velocity != 0).any()  # a moving survivor is in view
    r = renderer(old, (w, h))
    gbuffer_planes(r, fis[0], MOTION_PLANES)
    r.set_instances(new, previous=previous, local_aabbs=ic.local_aabbs(new))
    assert_scene_is(r, new.desc, meshes=False, materials=False)
    assert_planes(gbuffer_planes(r, fis[1], MOTION_PLANES), want, name)
    o.close()
    r.close()


# ------------------------------------------------------------------ the other two updates afterwards
def test_updates_after_a_set_take_the_current_set():
    """After spawn_pooled's set: hk_update_instances with the new count, and hk_update_meshes on the mesh the set
    change instanced first; both leave the host builder's arrays."""
    name = "spawn_pooled"
    c = ic.case(name)
    r = renderer(c.scenes[0])
    ic.apply(r, name, 1)
    moved = _moved_copy(c.scenes[1], [ic.SEED, 78])
    r.update_instances(moved.instance_models(), ic.local_aabbs(moved))
    assert_scene_is(r, moved.build(), meshes=False, materials=False)
    with pytest.raises(Exception, match="every instance"):
        r.update_instances(c.scenes[0].instance_models(), ic.local_aabbs(c.scenes[0]))  # the count before the set
    deformed = copy.copy(moved)
    deformed._h, deformed.desc = None, None
    deformed.meshes = list(moved.meshes)
    mesh = copy.copy(moved.meshes[1])
    rng = np.random.default_rng([ic.SEED, 79])
    mesh.positions = (mesh.positions + rng.uniform(-0.02, 0.02, mesh.positions.shape) * [1.0, 0.0, 1.0]).astype(np.float32)
    deformed.meshes[1] = mesh
    r.update_meshes(deformed, [1], local_aabbs=ic.local_aabbs(deformed))
    assert_mesh_rebuild_bitwise(r, deformed.build())
    assert r.scene_counts() == ic.desc_counts(deformed.desc)
    r.close()


# ------------------------------------------------------------------ refusals
def _raw_set(r, scene, entries, count=None, models=True, aabbs=True, set_=True):
    """hk_set_instances with a hand-made list: its return code and message."""
    from hikari_amd import _abi
    n = len(entries)
    m = np.ascontiguousarray(np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (max(1, n), 1)))
    a = np.ascontiguousarray(np.tile(np.array([[0, 0, 0, 0.1, 0.0, 0.1]], np.float32), (max(1, n), 1)))
    arr = (_abi.hk_instance_desc * max(1, n))(*entries)
    return raw_call(r, "hk_set_instances", arr if set_ else None, m.ctypes.data if models else None,
                    a.ctypes.data if aabbs else None, n if count is None else count, None, None)


def test_refusals_leave_the_context_usable():
    """Every refusal of the header returns its code with a message; nothing was changed: the arrays still equal step
    0's, and a valid set then succeeds and matches."""
    from hikari_amd import HikariRenderer, _abi
    name = "spawn_pooled"
    c = ic.case(name)
    scene = c.scenes[0]
    n_v, n_p, n_n = ic.desc_counts(scene.desc)[:3]

    def entry(index, material=0, previous=_abi.HK_INSTANCE_NEW):
        v, p, n0, nc = index
        return _abi.hk_instance_desc(_abi.hk_mesh_index(v, p, (ctypes.c_uint32 * 2)(n0, nc)), material, previous)

    quad, pooled, last = (scene.mesh_index(i) for i in range(3))
    empty = HikariRenderer(0)
    rc, msg = _raw_set(empty, scene, [entry(quad)])
    assert rc == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()

    r = renderer(scene)
    v, p, n0, nc = pooled
    old_n = len(scene.instances)
    refused = [
        ("null set", dict(entries=[entry(quad)], set_=False), "null"),
        ("null models", dict(entries=[entry(quad)], models=False), "null"),
        ("null aabbs", dict(entries=[entry(quad)], aabbs=False), "null"),
        ("count 0", dict(entries=[entry(quad)], count=0), "empty instance set"),
        ("material", dict(entries=[entry(quad, len(scene.materials))]), "material index out of range"),
        ("not 3k - 2", dict(entries=[entry((v, p, n0, nc - 1))]), "3k - 2"),
        ("overlap", dict(entries=[entry((v, p + 1, n0 + 3, nc))]), "partly overlaps"),
        ("part of a known slice", dict(entries=[entry((last[0], last[1] + 1, last[2] + 3, last[3] - 3))]), "partly overlaps"),
        ("primitives past", dict(entries=[entry((last[0], n_p - 1, last[2], last[3]))]), "past the primitive array"),
        ("nodes past", dict(entries=[entry((last[0], last[1], n_n - 1, last[3]))]), "past the asset nodes"),
        ("vertex indices past", dict(entries=[entry((n_v - 1, p, n0, nc))]), "past the vertex array"),
        ("previous out of range", dict(entries=[entry(quad, previous=old_n)]), "not an index of the set before"),
        ("previous twice", dict(entries=[entry(quad, previous=1), entry(quad, previous=1)]), "used twice"),
    ]
    for label, kw, text in refused:
        rc, msg = _raw_set(r, scene, **kw)
        assert rc == _abi.HK_ERR_INVALID and text in msg, (label, rc, msg)
        assert_scene_is(r, scene.desc, meshes=False, materials=False)
    ic.apply(r, name, 1)
    assert_scene_is(r, ic.built(name, 1), meshes=False, materials=False)
    r.close()


def test_a_singular_model_fails_and_a_valid_set_repairs_it():
    from hikari_amd import HikariError
    name = "despawn_middle"
    c = ic.case(name)
    r = renderer(c.scenes[0])
    models = c.scenes[1].instance_models().copy()
    models[2, 4:8] = 0.0  # a zero column
    with pytest.raises(HikariError, match="singular instance transform"):
        ic.apply(r, name, 1, models=models)
    assert r.scene_counts() == ic.desc_counts(ic.built(name, 1))  # the set is the new one
    # the same entities again: every instance maps to itself
    r.set_instances(c.scenes[1], previous=list(range(len(models))), local_aabbs=ic.local_aabbs(c.scenes[1]))
    assert_scene_is(r, ic.built(name, 1), meshes=False, materials=False)
    r.close()


# ------------------------------------------------------------------ capacity
def test_a_steady_toggle_allocates_nothing():
    """Despawn one instance and spawn it back: after the first round, ten more rounds leave the device's free memory
    where it was (hipMemGetInfo counts the whole device, so another process can move it: one undisturbed window of
    three is asked for; a call that allocated would move it in every window)."""
    name = "despawn_middle"
    c = ic.case(name)
    back = [c.previous[1].index(i) if i in c.previous[1] else None for i in range(len(c.scenes[0].instances))]
    r = renderer(c.scenes[0])
    hip = hip_runtime()
    hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    def toggle():
        ic.apply(r, name, 1)
        r.set_instances(c.scenes[0], previous=back, local_aabbs=ic.local_aabbs(c.scenes[0]))

    toggle()
    gc.collect()
    windows = []
    for _ in range(3):
        before = free_bytes()
        for _ in range(10):
            toggle()
        windows.append(free_bytes() - before)
        if windows[-1] == 0:
            break
    assert 0 in windows, windows
    assert_scene_is(r, c.scenes[0].desc, meshes=False, materials=False)
    r.close()


def test_a_set_past_the_capacity_grows_by_half_and_stays():
    """spawn_copies 4 -> 6 takes arrays 3, 4, 5, 7 and 8 past the capacity the upload gave them: each grows to
    max(count, capacity + capacity // 2) and the others keep theirs; the way back and a second way forward fit."""
    name = "there_and_back"
    c = ic.case(name)
    r = renderer(c.scenes[0])
    before = r.scene_capacity()
    assert before == [max(1, n) for n in ic.desc_counts(c.scenes[0].desc)]
    ic.apply(r, name, 1)
    counts, after = r.scene_counts(), r.scene_capacity()
    for i in (3, 4, 5, 7, 8):
        assert counts[i] > before[i], (i, counts, before)  # (the case: every one of them has to grow)
        assert after[i] == max(counts[i], before[i] + before[i] // 2), (i, counts, before, after)
    for i in (0, 1, 2, 6):
        assert after[i] == before[i], (i, before, after)
    ic.apply(r, name, 2)
    assert r.scene_capacity() == after
    ic.apply(r, name, 1)
    assert r.scene_capacity() == after
    assert_scene_is(r, ic.built(name, 1), meshes=False, materials=False)
    r.close()


def test_plugin_forwards_set_instances():
    from hikari_amd import HikariPlugin
    name = "emitter_on"
    c = ic.case(name)
    p = HikariPlugin(c.scenes[0])
    p.set_instances(c.scenes[1], previous=c.previous[1])
    assert_scene_is(p.renderer, ic.built(name, 1), meshes=False, materials=False)
    p.renderer.close()
