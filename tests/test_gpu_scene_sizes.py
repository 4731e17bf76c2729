"""GPU parity on the scene ladder (tests/scene_ladder.py): scenes whose staged sizes sit on the edges of the LDS
scene staging — the second round of stage_scene's copy loop (16384 bytes), the last staged and first unstaged
sizes of either plan (LDS_SCENE_MAX = 32768), a staged G-buffer walk with and without room for its LDS stack
(49152) — and scenes with no emitter, an odd alias table, several emitters, a single triangle.  Every rung bit
for bit against the CPU oracle, whose frames are computed once per rung (scene_ladder.reference) and shared by all
the cases here.  tests/test_scene_ladder.py proves each rung's position without a GPU.
"""
import numpy as np
import pytest

import scene_ladder as sl
from parity import (NODE_DT, RACY, assert_instance_update_matches_host, canon_plane, compare_frame, host_scene_array,
                    moved, pair, passes, renderer, run_frames)

pytestmark = pytest.mark.gpu


def _rung_against_reference(name, bounces=1, wavefront=False):
    """A renderer of the rung over the ladder's frames against the stored oracle frames and counters."""
    from hikari_amd import frame_inputs
    scene, cam, lights = sl.built(name)
    r = renderer(scene, sl.SIZE, wavefront=wavefront)
    run_frames(r, sl.reference(name, bounces), sl.ladder_settings(bounces).to_c(),
               (frame_inputs(f, cam, lights, *sl.SIZE) for f in range(sl.FRAMES)))


@pytest.mark.parametrize("lds", [1, 0, 2], ids=["lds_default", "lds_off", "lds_all"])
@pytest.mark.parametrize("name", list(sl.RUNGS))
def test_ladder_rung_bit_exact(hk_options, name, lds):
    """Every rung at 64 x 48, ratio 1, frames 0..5 with emissive and indirect spatial reuse and the denoiser: planes
    0..16, reservoir buffers 0..9 and the ray counters, with the scene staged where the defaults stage it, nowhere,
    and in every traversal kernel."""
    hk_options["lds_scene"] = lds
    _rung_against_reference(name)


@pytest.mark.parametrize("variant", list(sl.LAUNCH_VARIANTS))
@pytest.mark.parametrize("name", sl.VARIANT_RUNGS)
def test_ladder_launch_variants_bit_exact(hk_options, name, variant):
    """The light passes' other launches on the rungs around both staging edges, each with lds_scene = 2: merged and
    unmerged, the fused direct / emissive launch, its 4-wave kernels on a small frame, the separate 4-wave direct
    kernel, persistent waves, the compacted walks, spatial reuse without view planes, the multi-bounce indirect
    kernel and the wavefront indirect pass; and, with the staging setting each needs, the merged launch whose indirect
    role stages (the IndStash behind the staged scene) and the compacted fused kernels."""
    hk_options["lds_scene"] = 2
    hk_options.update(sl.LAUNCH_VARIANTS[variant])
    _rung_against_reference(name, bounces=2 if variant == "bounces_2" else 1, wavefront=variant == "wavefront")


_gbuffer_reference = {}


def _gbuffer_oracle(name, cam):
    """Planes 11..15 and the counters of one oracle G-buffer of the rung under `cam`, once per (rung, projection)."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    key = (name, cam.orthographic_height)
    if key not in _gbuffer_reference:
        scene, _, lights = sl.built(name)
        w, h = sl.SIZE
        o = Oracle(scene.desc, load_noise(), w, h, 1.0)
        o.render_gbuffer(frame_inputs(0, cam, lights, w, h))
        _gbuffer_reference[key] = ({oid: canon_plane(oid, o.output(oid)) for oid in range(11, 16)}, o.counters())
        o.close()
    return _gbuffer_reference[key]


GBUFFER_CASES = {"default": {}, "unstaged": {"gbuffer_lds_max_px": 0}, "stack_full": {"gbuffer_stack_full": 1},
                 "deep": {"gbuffer_deep": 1}, "orthographic": {}}


@pytest.mark.parametrize("case", list(GBUFFER_CASES))
@pytest.mark.parametrize("name", sl.GBUFFER_RUNGS)
def test_ladder_gbuffer_walks_bit_exact(name, case):
    """The primary-ray walk on the rungs at the G-buffer plan's limit, one chunk over it, and staged without room
    for its LDS stack (k_gbuffer<true, false, 0>): planes 11..15 and the primary counter, with the default small-frame
    staging, without it, with all 16 stack levels asked for, with the deep (scratch) stack, and under an
    orthographic view."""
    from hikari_amd import Camera, frame_inputs
    scene, cam, lights = sl.built(name)
    r = renderer(scene, sl.SIZE, options=GBUFFER_CASES[case])
    if case == "orthographic":
        cam = Camera.orthographic(cam.transform, 3.0)
    planes, counters = _gbuffer_oracle(name, cam)
    w, h = sl.SIZE
    fi = frame_inputs(0, cam, lights, w, h)
    assert (fi.view.projection[15] == 1.0) == (case == "orthographic")
    r.render_gbuffer(fi)
    errors = []
    compare_frame(r, (planes, ()), 0, errors, outputs=range(11, 16), rids=())
    assert not errors, "\n".join(errors)
    assert r.counters()["primary"] == counters["primary"] == w * h
    depth = planes[11].view(np.float32).reshape(h, w, 4)[..., 3]
    assert (depth > 0).mean() > 0.2  # the view sees the scene


@pytest.mark.parametrize("name", ["emitters_3", "one_triangle", "light_at_limit"])
def test_ladder_trace_matches_oracle(name):
    """hk_trace against hko_trace: 20 000 seeded rays through the rung's volume, 100 of them axis-parallel, with
    any-hit / closest-hit early distances and excluded instances (test_trace_matches_oracle on cornell)."""
    from hikari_amd import load_noise
    from oracle import Oracle
    scene, cam, lights = sl.built(name)
    r = renderer(scene, sl.SIZE)
    o = Oracle(scene.desc, load_noise(), 16, 16, 1.0)
    rng = np.random.default_rng(7)
    n = 20000
    org = rng.uniform([-1.3, -0.2, -1.3], [1.3, 2.2, 1.3], (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:100, 0] = 0.0  # axis-parallel rays: 1/0 = inf in the slab test
    rays = np.concatenate([org, d], axis=1).astype(np.float32)
    early = np.where(rng.random(n) < 0.5, 0.0, 65535.0).astype(np.float32)
    excl = rng.integers(0, len(scene.instances) + 1, n).astype(np.uint32)
    a = r.trace(rays, None, early, excl)
    b = o.trace(rays, None, early, excl)
    assert (a == b).all(), f"{int((a != b).any(axis=1).sum())} of {n} rays differ"
    hit = (a[:, 3] != 0xFFFFFFFF).mean()
    # a lone 0.4-square-unit triangle is hit by few random rays; the furnished rungs by a good part of them
    assert hit > (0.001 if name == "one_triangle" else 0.25), hit


@pytest.mark.parametrize("name", ["emitters_3", "no_emitters", "light_at_limit"])
def test_ladder_instance_update_matches_host_rebuild(name):
    """hk_update_instances on a rung (test_gpu_instance_update_matches_host_rebuild): the device's instance, alias,
    emissive, light-BVH and TLAS arrays against the host builder's for seeded transforms — a light BVH over three
    emitters, and the empty-emissive branch — then two frames against the oracle on the host-built scene."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs, load_noise
    from oracle import Oracle
    scene0, cam, lights = sl.built(name)
    r = renderer(scene0, sl.SIZE)
    scene1, _, _ = moved(sl.build(name), 7)
    d1 = scene1.build()
    r.update_instances(scene1.instance_models(), scene1.instance_local_aabbs())
    emitters = len(sl.RUNGS[name]["emitters"])
    assert len(host_scene_array(d1, 8, np.dtype((np.void, 64)))) == emitters
    assert len(host_scene_array(d1, 7, NODE_DT)) == (3 * emitters - 2 if emitters else 0)
    # an empty array of the scene: nothing to read back (the frames below cover the branch)
    assert_instance_update_matches_host(r, d1, skip_empty=True)
    # and the frames: the oracle sees the uploaded scene, then the moved one (motion vectors reproject from the
    # uploaded models); single-threaded with spatial reuse off, as the reprojection scatter is a write race
    w, hgt = sl.SIZE
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False)
    o = Oracle(scene0.desc, load_noise(), w, hgt, 1.0, threads=1)
    o.set_scene(d1)
    s = st.to_c()
    errors = []
    for f in range(2):
        fi = frame_inputs(f, cam, lights, w, hgt)
        for x in (r, o):
            passes(x, s, fi)
        compare_frame(r, o, f, errors, racy=RACY)
    assert not errors, "\n".join(errors[:10])
    assert r.counters() == o.counters()


def test_ladder_two_rounds_moving_camera():
    """The two-round rung under the examples' orbit camera (examples.orbit, 0.5 degrees per frame about the scene's
    centre), spatial reuse off and the oracle single-threaded: test_gpu_motion's comparison — everything outside
    the racy spatial-pair scatter targets bit-exact, those within its tolerance — and motion vectors present."""
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs
    w, h = sl.SIZE
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False, denoise=True)
    scene, cam, lights, r, o = pair(sl.built("two_rounds"), w, h, st, threads=1)
    s = st.to_c()
    target = (0.0, 1.0, 0.0)
    errors = []
    moved = 0
    for f in range(4):
        fi = frame_inputs(f, examples.orbit(cam, target, f), lights, w, h,
                          previous_camera=examples.orbit(cam, target, f - 1) if f else None)
        for x in (r, o):
            passes(x, s, fi)
        compare_frame(r, o, f, errors, racy=RACY)
        vel = r.output(15).view(np.float32).reshape(h, w, 4)[..., :2]
        moved += int((vel != 0).any(axis=-1).sum())
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert moved > w * h  # most covered pixels carry a motion vector in the three moving frames
    assert r.counters() == o.counters()
