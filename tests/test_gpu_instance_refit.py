"""hk_refit_instances / hk_refit_meshes_all / hk_skin_meshes_refit_all at their size and shape edges: the cases of
tests/instance_refit_cases.py (each proven to sit on its edge by tests/test_instance_refit_cases.py, without a GPU)
uploaded as scene0 and refit to scene1's models.  All nine arrays byte for byte Scene.refitted_instances(...): scene1 as
the host builds it, except the TLAS and the light BVH, which are the trees the device held before passed through
hks_refit_boxes (itself held to tests/refit_boxes_numpy.py by tests/test_instance_refit_independent.py) with the leaves
carrying their instance's box as on the device, and every node_index, which is the kept tree's.  Frames, G-buffers and
counters against the CPU oracle on that scene.

What each case exists for in csrc/hk_dynamic.hip:
  n1_m0, n1_m1, n2             a lone TLAS leaf without / with a lone light-BVH leaf: a table of one / two trees, nothing
                               to fold, k_refit_trees_large not launched; one pair of entry nodes
  tlas_at_32 / tlas_at_35      no large node / the first range past REFIT_SMALL in tree 0 of the table
  lights_at_32 / lights_at_35  the same in tree 1, whose nodes lie behind tree 0's in the launch and in the list
  no_large, many_large         the list stays empty / hundreds of large nodes of both trees in one list, ranges the 256
                               threads stride over more than once
  over_256, over_lds           a refit that follows k_build_bvh<true> / <false>
  deep                         a chain at the G-buffer stack's deepest level: every upper level a large node
  swapped, coincident          the stalest tree; every shape box equal
  neg_zero, unchanged          zeros of both signs under an unordered fold; the boxes the tree was built from
  moving                       frames across the call: previous models, motion vectors
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.
"""
import copy

import numpy as np
import pytest

import dynamic_cases as dc
import instance_refit_cases as ic
from parity import NODE_DT, assert_rebuild_bitwise, host_scene_array, renderer
from scene_edits import (EditFrames, assert_mesh_arrays, assert_planes, assert_scene_is, caller_stream, gbuffer_planes,
                         models_and_aabbs, ptr, raw_call)

pytestmark = pytest.mark.gpu


def _refit(r, scene, stream=None, refit=True):
    r.update_instances(scene.instance_models(), scene.instance_local_aabbs(), stream, refit=refit)


def _expect(desc0, scene1):
    from hikari_amd import Scene
    return Scene.refitted_instances(desc0, scene1)


# ------------------------------------------------------------------ arrays
@pytest.mark.parametrize("name", ic.ARRAY_CASES)
def test_refit_arrays_match_the_refitted_scene(name):
    scene0, scene1 = ic.case(name)
    r = renderer(scene0)
    _refit(r, scene1)
    assert_scene_is(r, ic.refitted(name))
    if ic.COUNTS[name][0] > 2 and name != "unchanged":  # and the kept tree is not the one a rebuild gives
        want, built = ic.refitted(name), ic.built1(name)
        assert host_scene_array(want, 5, NODE_DT).tobytes() != host_scene_array(built, 5, NODE_DT).tobytes()
    r.close()


# ------------------------------------------------------------------ sequences
@pytest.mark.parametrize("name", ic.REPEAT_CASES)
def test_repeated_refits(name):
    """A second refit back to scene0's models equals refitted(desc0, scene0): a refit of a refit is the direct one (the
    boxes are derived from the leaves alone), on the scratch, the list and the counter the first call left; and a third
    forth again."""
    scene0, scene1 = ic.case(name)
    r = renderer(scene0)
    _refit(r, scene1)
    assert_scene_is(r, ic.refitted(name))
    _refit(r, scene0)
    assert_scene_is(r, _expect(scene0.desc, scene0))
    _refit(r, scene1)
    assert_scene_is(r, ic.refitted(name))
    r.close()


@pytest.mark.parametrize("name", ic.BUILD_CASES)
def test_refit_after_rebuild_and_rebuild_after_refit(name):
    """hk_update_instances after a refit gives the host-built scene1 (hks_build's trees again); hk_refit_instances after
    that keeps the NEW topology, the one the device built."""
    scene0, scene1 = ic.case(name)
    r = renderer(scene0)
    _refit(r, scene1)
    assert_scene_is(r, ic.refitted(name))
    _refit(r, scene1, refit=False)
    assert_scene_is(r, ic.built1(name))
    _refit(r, scene0)
    assert_scene_is(r, _expect(ic.built1(name), scene0))
    _refit(r, scene0, refit=False)
    assert_scene_is(r, scene0.desc)
    r.close()


def _moved_copy(scene, seed):
    """The scene with every instance nudged by a seeded transform: a new Scene object, not built."""
    rng = np.random.default_rng([ic.SEED, seed])
    out = copy.copy(scene)
    out._h, out.desc = None, None
    out.instances = [(mesh, mat, t @ np.asarray(m, np.float64))
                     for (mesh, mat, m), t in zip(scene.instances, ic._nudged([np.eye(4)] * len(scene.instances), rng))]
    return out


def test_refit_after_set_instances():
    """instance_set_cases' spawn_pooled: the set hk_set_instances spawned into, then moved by a refit: the trees of the
    set's build are kept, over its counts."""
    import instance_set_cases as sc
    name = "spawn_pooled"
    c = sc.case(name)
    r = renderer(c.scenes[0])
    sc.apply(r, name, 1)
    assert_scene_is(r, sc.built(name, 1), meshes=False, materials=c.materials)
    moved = _moved_copy(c.scenes[1], 1)
    r.update_instances(moved.instance_models(), sc.local_aabbs(moved), refit=True)
    want = _expect(sc.built(name, 1), moved)
    assert r.scene_counts() == sc.desc_counts(want)
    assert_rebuild_bitwise(r, want)
    r.close()


def test_refit_after_add_meshes_and_a_spawn():
    """mesh_add_cases' then_update: a mesh appended by hk_add_meshes and spawned by hk_set_instances, then every
    instance moved by a refit."""
    import mesh_add_cases as ac
    name = "then_update"
    c = ac.case(name)
    r = renderer(c.scenes[0])
    last = len(c.scenes) - 1
    for k in list(ac.steps(name))[1:]:
        ac.add(r, name, k)
        ac.spawn(r, name, k)
    moved = _moved_copy(c.scenes[last], 2)
    r.update_instances(moved.instance_models(), ac.local_aabbs(moved), refit=True)
    want = _expect(ac.built(name, last), moved)
    assert_rebuild_bitwise(r, want)
    assert_mesh_arrays(r, want, ac.added_so_far(name, last))
    r.close()


def test_refit_meshes_all_is_the_composition():
    """hk_refit_meshes_all: the listed BLAS refit (Scene.refitted) and both instance trees refit over the deformed
    scene's boxes (Scene.refitted_instances of that desc); hk_refit_meshes on the same context then rebuilds the
    instance trees and keeps the BLAS."""
    import mesh_cases as mc
    import refit_cases as rc
    from hikari_amd import Scene
    name = "emissive_mesh"
    scene0, scene1 = rc.case(name)
    r = renderer(scene0)
    source = rc.update_source(name, 1)
    r.update_meshes(source, rc.listed(name), local_aabbs=mc.local_aabbs(source), refit="all")
    assert_scene_is(r, Scene.refitted_instances(scene0.desc, rc.refitted(name)))
    r.update_meshes(source, rc.listed(name), local_aabbs=mc.local_aabbs(source), refit=True)
    assert_scene_is(r, rc.refitted(name))
    r.close()


def test_skin_meshes_refit_all_is_the_composition():
    import skin_cases as sc
    from hikari_amd import Scene
    name = sc.FRAME_CASES[0]
    c = sc.case(name)
    r = renderer(c.scene0)
    r.set_mesh_skins(c.scene0, c.skinned, c.keep_normals)
    pose = c.poses[0]
    r.skin_meshes(c.scene0, pose, local_aabbs=sc.caller_aabbs(c.scene0, set(pose)), refit="all")
    blas = Scene.refitted(c.scene0.desc, sc.posed(name, 0)[0], list(pose))
    assert_scene_is(r, Scene.refitted_instances(c.scene0.desc, blas))
    r.close()


# ------------------------------------------------------------------ frames
def _frames(name, options=None, wavefront=False, before=0):
    """`before` frames on scene0, the refit, then two 64 x 48 frames, each against the oracle (one thread, spatial reuse
    off, the racy scatter targets within their tolerance; the oracle takes the refitted desc by set_scene, which keeps
    its previous models as the context keeps its own), and the ray counters: what is derived from the refit TLAS (leaf
    boxes, wide layout, collapsed walk nodes) and the refit light BVH is what the frames walk."""
    scene0, scene1 = ic.case(name)
    d1 = ic.refitted(name)
    with EditFrames(scene0, ic.camera_for(name), ic.FRAME_SIZE, floor=0.02, options=options, wavefront=wavefront) as fr:
        fr.frames(before)
        _refit(fr.r, scene1)
        assert_scene_is(fr.r, d1)
        fr.set_scene(d1)
        fr.frames(1)
        if before:  # the frame after the call: the instances moved on screen since the one before
            depth, velocity = fr.oracle_plane(11)[..., 3], fr.oracle_plane(15)[..., :2]
            assert (np.abs(velocity[depth > 0]) > 1e-4).any()
        fr.frames(1)


@pytest.mark.parametrize("name", ic.FRAME_CASES)
def test_frames_after_refit_match_oracle(name):
    _frames(name)


def test_frames_of_a_moving_pair_with_previous_models():
    """Two frames on scene0, then the refit: the first frame after it reprojects with scene0's models as the previous
    ones (hk_refit_instances marks the models dirty as hk_update_instances does)."""
    _frames(ic.VARIANT_CASE, before=2)


@pytest.mark.parametrize("options", [{"lds_scene": 0}, {"lds_scene": 1}, {"lds_scene": 2}, {"leaf_collapse": 0}],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_frames_under_staging_and_collapse_options(options):
    _frames(ic.VARIANT_CASE, options)


def test_frames_with_the_wavefront_pass():
    _frames(ic.VARIANT_CASE, wavefront=True)


def test_the_deep_chain_is_walked_at_its_own_depth():
    """deep: the kept TLAS is a chain whose stack bound is 64, the models a rebuild would give a shallow tree for.  The
    G-buffer planes equal the oracle's on the refitted desc in the default context and with gbuffer_stack_full and
    gbuffer_deep: the bound is still the chain's."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    scene0, scene1 = ic.case("deep")
    d1 = ic.refitted("deep")
    cam, lights = ic.camera_for("deep")
    w, h = ic.FRAME_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    o = Oracle(d1, load_noise(), w, h, 1.0)
    want = gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.02
    for opts in ({}, {"gbuffer_stack_full": 1}, {"gbuffer_deep": 1}):
        r = renderer(scene0, (w, h), options=opts)
        _refit(r, scene1)
        assert_scene_is(r, d1)
        assert_planes(gbuffer_planes(r, fi), want, f"deep {opts}")
        r.close()
    o.close()


def test_the_stack_bound_is_unchanged_by_the_call():
    """dynamic_cases' too_deep: a rebuild makes the TLAS one level too deep for the G-buffer walk, which refuses.  A
    refit back to scene0's shallow models keeps that tree and that bound: the same refusal, word for word.  The
    rebuild to the same models then lowers the bound and the G-buffer renders."""
    from hikari_amd import HikariError, frame_inputs
    scene0, scene1 = dc.case("too_deep")
    cam, lights = dc.camera_for("too_deep")
    w, h = ic.FRAME_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    r = renderer(scene0, (w, h))
    _refit(r, scene1, refit=False)
    with pytest.raises(HikariError, match="too deep for the G-buffer traversal stack") as rebuilt:
        r.render_gbuffer(fi)
    _refit(r, scene0)
    assert_scene_is(r, _expect(dc.built1("too_deep"), scene0))
    with pytest.raises(HikariError, match="too deep for the G-buffer traversal stack") as kept:
        r.render_gbuffer(fi)
    assert str(kept.value) == str(rebuilt.value) and "depth > 64" in str(kept.value)
    _refit(r, scene0, refit=False)
    r.render_gbuffer(fi)
    r.close()


# ------------------------------------------------------------------ refusals
def _raw(r, scene, count=None, models=True, aabbs=True):
    m, a = models_and_aabbs(scene, scene.instance_local_aabbs())
    return raw_call(r, "hk_refit_instances", ptr(m, models), ptr(a, aabbs), len(m) if count is None else count, None)


def test_refusals_leave_the_context_usable():
    """hk_update_instances' refusals under hk_refit_instances' own name; nothing was changed: the arrays still equal
    scene0's, and a refit then succeeds and matches.  A singular model is refused after the device has seen it, as by
    hk_update_instances; the next refit succeeds and matches."""
    from hikari_amd import HikariError, HikariRenderer, _abi
    name = "over_256"
    scene0, scene1 = ic.case(name)
    empty = HikariRenderer(0)
    rc_, msg = _raw(empty, scene1)
    assert rc_ == _abi.HK_ERR_STATE and "no scene" in msg
    empty.close()
    assert _abi.lib().hk_refit_instances(None, None, None, 0, None) == _abi.HK_ERR_INVALID

    r = renderer(scene0)
    for label, kw in (("null models", dict(models=False)), ("null aabbs", dict(aabbs=False))):
        rc_, _ = _raw(r, scene1, **kw)
        assert rc_ == _abi.HK_ERR_INVALID, label
        assert_scene_is(r, scene0.desc)
    for count in (len(scene1.instances) - 1, len(scene1.instances) + 1, 0):
        rc_, msg = _raw(r, scene1, count=count)
        assert rc_ == _abi.HK_ERR_INVALID and "hk_refit_instances needs every instance" in msg, count
        assert_scene_is(r, scene0.desc)
    models = scene1.instance_models().copy()
    models[17, 4:8] = 0.0  # a zero column
    with pytest.raises(HikariError, match="singular instance transform"):
        r.update_instances(models, scene1.instance_local_aabbs(), refit=True)
    _refit(r, scene1)
    assert_scene_is(r, ic.refitted(name))
    r.close()


# ------------------------------------------------------------------ state
def test_refit_on_a_caller_stream():
    name = "many_large"
    scene0, scene1 = ic.case(name)
    r = renderer(scene0)
    with caller_stream() as (s, sync):
        _refit(r, scene1, stream=s)
        sync()
        assert_scene_is(r, ic.refitted(name))
        r.close()


def test_plugin_forwards_refit():
    import mesh_cases as mc
    import refit_cases as rc
    from hikari_amd import HikariPlugin, Scene
    name = "moving"
    scene0, scene1 = ic.case(name)
    p = HikariPlugin(scene0)
    p.update_instances(scene1.instance_models(), scene1.instance_local_aabbs(), refit=True)
    assert_scene_is(p.renderer, ic.refitted(name))
    p.renderer.close()
    name = "strip"
    scene0, scene1 = rc.case(name)
    p = HikariPlugin(scene0)
    p.update_meshes(scene1, rc.listed(name), local_aabbs=mc.local_aabbs(scene1), refit="all")
    assert_scene_is(p.renderer, Scene.refitted_instances(scene0.desc, rc.refitted(name)))
    p.renderer.close()


def test_a_steady_refit_keeps_the_capacity():
    name = "over_lds"
    scene0, scene1 = ic.case(name)
    r = renderer(scene0)
    before = r.scene_capacity()
    for scene in (scene1, scene0, scene1):
        _refit(r, scene)
        assert r.scene_capacity() == before
    assert_scene_is(r, ic.refitted(name))
    r.close()
