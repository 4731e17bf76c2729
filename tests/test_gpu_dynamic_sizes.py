"""hk_update_instances at its size, shape and depth edges: the cases of tests/dynamic_cases.py (each proven to sit on
its edge by tests/test_dynamic_cases.py, without a GPU) uploaded as scene0, updated to scene1's transforms, and the
rebuilt instance, alias, emissive, light-BVH and TLAS arrays compared byte for byte with the host builder's; frames,
G-buffers and counters against the CPU oracle on the host-built scene1.

The branch of csrc/hk_dynamic.hip each case exists for:
  tlas_1, tlas_2                 k_build_bvh with a lone leaf / one split; no emitter (tlas_1: the rebuild without
                                 emissive kernels)
  tlas_128 / tlas_129            the per-thread split (split_segment) alone / the cooperative split (coop_split)
                                 entered at the root, COOP_MIN
  tlas_256 / tlas_257            one / two 256-chunks of coop_split's ballot ranking, the cursor carried over
  tlas_1280 / tlas_1281          k_build_bvh<true> (shapes and indices staged in LDS) / k_build_bvh<false> (global
                                 memory), BVH_LDS_SHAPES
  tlas_2600                      the global build with several levels of big segments
  big_overflow                   more than BIG_MAX big segments on a level: push() turns the further ones over to
                                 the per-thread split
  lights_1 .. lights_300,        the light BVH: a lone leaf, one split, the cooperative path (more than 128
  all_emitters                   emitters), a second ballot chunk; every instance an emitter
  alias_1, alias_64 / alias_65   k_update_emissives: one / two wave chunks of the over / under compaction
  alias_3072 / alias_3073        the alias stacks in LDS / in global scratch, ALIAS_LDS
  two_large                      two emitters on the global stacks, the second at a scratch offset other than 0
  skewed, regular,               a long over chain; probabilities of exactly 1 (in neither list); a zero-area
  one_degenerate                 triangle (probability 0)
  coincident_100 / _300          the `halves` branch of split_segment / of coop_split
  clustered                      SAH splits first, `halves` below them
  equal_spacing                  tied SAH costs: `cost < best_cost` keeps the first
  mirrored .. scale_1e4          k_update_instances / k_emissive_areas under transforms far from the usual ones
  neg_zero                       min / max of zeros of both signs, in k_update_instances and in the box joins
  deep_lds_edge .. too_deep      `levels`, the TLAS part of the G-buffer walk's stack bound: 16, 17, 64 and 65
  singular                       the singular flag
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.
"""
import numpy as np
import pytest

import dynamic_cases as dc
from parity import assert_rebuild_bitwise, renderer
from scene_edits import DEPTH_SIZE, EditFrames, assert_planes, caller_stream, gbuffer_planes

pytestmark = pytest.mark.gpu


def _update(r, scene, stream=None):
    r.update_instances(scene.instance_models(), scene.instance_local_aabbs(), stream)


@pytest.mark.parametrize("name", dc.ARRAY_CASES)
def test_rebuilt_arrays_match_host_builder(name):
    """Upload scene0, update to scene1's transforms: every rebuilt array equals the host builder's for scene1, byte
    for byte (the TLAS with the instance boxes in its leaves), tree topology included."""
    scene0, scene1 = dc.case(name)
    r = renderer(scene0)
    _update(r, scene1)
    assert_rebuild_bitwise(r, dc.built1(name))
    r.close()


@pytest.mark.parametrize("name", dc.SECOND_UPDATE_CASES)
def test_second_update_on_dirty_scratch(name):
    """A second update back to scene0's transforms: the index buffers, segment lists and alias stacks are reused
    as the first update left them."""
    scene0, scene1 = dc.case(name)
    r = renderer(scene0)
    _update(r, scene1)
    assert_rebuild_bitwise(r, dc.built1(name))
    _update(r, scene0)
    assert_rebuild_bitwise(r, scene0.desc)
    r.close()


@pytest.mark.parametrize("name", dc.FRAME_CASES)
def test_frames_after_rebuild_match_oracle(name):
    """After the array check, two 32 x 24 frames against the oracle on the host-built scene1, as
    test_ladder_instance_update_matches_host_rebuild renders them (the oracle sees scene0, then scene1; one thread,
    spatial reuse off, the racy scatter targets within their tolerance), and the ray counters: what is derived from
    the rebuilt TLAS (leaf boxes, wide layout, collapsed walk nodes) and from the rebuilt alias and emissive tables."""
    scene0, scene1 = dc.case(name)
    d1 = dc.built1(name)
    with EditFrames(scene0, dc.camera_for(name), dc.FRAME_SIZE, floor=0.2) as fr:
        _update(fr.r, scene1)
        assert_rebuild_bitwise(fr.r, d1)
        fr.set_scene(d1)
        fr.frames(2)


@pytest.mark.parametrize("name", ["deep_lds_edge", "deep_over_lds", "deep_at_limit"])
def test_tlas_deepened_by_an_update(name):
    """An update turns a shallow TLAS into one whose stack bound is 16 (every LDS level of the shallow walk), 17 (the
    first scene of the deep walk) or 64 (the last the walk takes): the G-buffer planes 11..14 after it equal the
    oracle's on scene1, in the default context and in contexts with gbuffer_stack_full and gbuffer_deep."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    scene0, scene1 = dc.case(name)
    d1 = dc.built1(name)
    cam, lights = dc.camera_for(name)
    w, h = DEPTH_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    o = Oracle(d1, load_noise(), w, h, 1.0)
    want = gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.005  # some of them are in view
    for opts in ({}, {"gbuffer_stack_full": 1}, {"gbuffer_deep": 1}):
        r = renderer(scene0, (w, h), options=opts)
        _update(r, scene1)
        assert_rebuild_bitwise(r, d1)
        assert_planes(gbuffer_planes(r, fi), want, f"{name} {opts}")
        r.close()
    o.close()


def test_update_to_a_tlas_too_deep_for_the_gbuffer_walk():
    """Stack bound 65: the update itself succeeds and its arrays match the host; hk_render_gbuffer then refuses, naming
    the depth, exactly as a fresh context does that uploaded scene1 (the device's level count and the host's
    scene_stack_need agree on the side of 64); an update back to scene0's transforms renders and matches the oracle."""
    from hikari_amd import HikariError, frame_inputs, load_noise
    from oracle import Oracle
    scene0, scene1 = dc.case("too_deep")
    d1 = dc.built1("too_deep")
    cam, lights = dc.camera_for("too_deep")
    w, h = DEPTH_SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    r = renderer(scene0, (w, h))
    _update(r, scene1)
    assert_rebuild_bitwise(r, d1)
    with pytest.raises(HikariError, match="too deep for the G-buffer traversal stack") as updated:
        r.render_gbuffer(fi)
    fresh = renderer(scene1, (w, h))
    with pytest.raises(HikariError, match="too deep for the G-buffer traversal stack") as uploaded:
        fresh.render_gbuffer(fi)
    assert str(updated.value) == str(uploaded.value) and "depth > 64" in str(updated.value)
    fresh.close()
    _update(r, scene0)
    assert_rebuild_bitwise(r, scene0.desc)
    o = Oracle(scene0.desc, load_noise(), w, h, 1.0)
    want = gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.1
    assert_planes(gbuffer_planes(r, fi), want, "back on scene0")
    o.close()
    r.close()


def test_singular_transform_is_refused_and_the_context_stays_usable():
    """hk_update_instances with a transform of determinant 0 fails with the host builder's message; an update with
    scene0's own transforms then succeeds, its arrays match scene0's host build and a G-buffer matches the oracle."""
    from hikari_amd import HikariError, frame_inputs, load_noise
    from oracle import Oracle
    scene0, scene1 = dc.case("singular")
    cam, lights = dc.camera_for("singular")
    w, h = DEPTH_SIZE
    r = renderer(scene0, (w, h))
    with pytest.raises(HikariError, match="singular instance transform"):
        _update(r, scene1)
    _update(r, scene0)
    assert_rebuild_bitwise(r, scene0.desc)
    fi = frame_inputs(0, cam, lights, w, h)
    o = Oracle(scene0.desc, load_noise(), w, h, 1.0)
    want = gbuffer_planes(o, fi)
    assert (want[0].view(np.float32).reshape(h, w, 4)[..., 3] > 0).mean() > 0.1
    assert_planes(gbuffer_planes(r, fi), want, "after the refused update")
    o.close()
    r.close()


def test_one_context_several_scenes():
    """One context: a 2-instance scene, a 2600-instance scene and the 2-instance scene again, each uploaded and
    updated; the arrays match at every step (the update's scratch grows with the scene and is released at upload)."""
    r = renderer(dc.case("tlas_2")[0])
    for k, name in enumerate(("tlas_2", "tlas_2600", "tlas_2")):
        scene0, scene1 = dc.case(name)
        if k:
            r.upload_scene(scene0)
        _update(r, scene1)
        assert_rebuild_bitwise(r, dc.built1(name))
    r.close()


def test_update_on_a_caller_stream():
    """tlas_1281 with update_instances(..., stream=s) on a stream of the caller's (scene_edits.caller_stream).
    hk_update_instances is documented to wait for its stream once (the singular check), so the rebuilt arrays are
    complete when it returns, and hk_read_scene_array, which synchronises only the context's own stream before a
    blocking copy, reads them whole; the test synchronises s first all the same.  torch.cuda.current_stream().cuda_stream,
    which bench.py passes, is handle 0, the context's own stream that every other test here runs on."""
    scene0, scene1 = dc.case("tlas_1281")
    r = renderer(scene0)
    with caller_stream() as (s, sync):
        _update(r, scene1, s)
        sync()
        assert_rebuild_bitwise(r, dc.built1("tlas_1281"))
        r.close()
