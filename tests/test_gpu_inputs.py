"""GPU parity along the input axes the rest of the suite never feeds: fractional upscale ratios,
orthographic views and HikariSettings at their edges (tests/inputs_cases.py), each bit-exact against the CPU
oracle on every plane, reservoir buffer and counter.

Fractional ratios (Upscale::SmaaTu4x { ratio } in (1, 2)): the integrator grid s = ceil((1 / ratio) S) is no
divisor of S, jittered_deferred_uv (light.wgsl:1007-1017) adds a fractional (ratio - 1) jitter, deferred lookups
land on texels ratios 1 and 2 never produce (out-of-frame ones read 0), spatial reuse runs without its
workgroup window, the fused launch, background elision and the identity-reprojection shortcuts are off, and the
SMAA / TAA planes are ceil(S 2 / ratio).  Orthographic views (view.projection[3].w == 1): calculate_view's
orthographic vector in every light pass and the orthographic primary rays of the G-buffer.
tests/test_inputs_independent.py pins the oracle's side of all three to independent restatements.
"""
import copy

import numpy as np
import pytest

import inputs_cases as ic
from parity import RACY, compare_frame, orbit_camera, pair, passes, run_static

pytestmark = pytest.mark.gpu

WITH_POST = tuple(range(17)) + (18, 19)  # and OUT_UPSCALED, OUT_TAA (RGBA16F, as the tone-mapped plane)


def _check_sizes(r, o):
    """hk_output_info against the oracle's plane sizes, outputs 0..19 (17, the sub-frame accumulator, is the
    runtime's own: the oracle has none)."""
    for oid in range(20):
        try:
            h, w, b = o.output(oid).shape
        except KeyError:
            assert oid == 17
            continue
        assert r.output_info(oid) == (w, h, b), (oid, r.output_info(oid), (w, h, b))


FRACTIONAL = [(1.5, (63, 47), "cornell_textured", None),
              (1.3, (64, 48), "cornell", None),
              (1.7, (62, 41), "cornell", None),
              (1.5, (63, 47), "cornell_textured", {"merge": 1}),
              (1.5, (63, 47), "cornell_textured", {"merge": 0, "persistent_indirect": 1}),
              (1.5, (63, 47), "cornell_textured", {"pipeline_min_px": 0}),
              (1.5, (63, 47), "cornell_textured", {"lds_scene": 0}),
              (1.5, (63, 47), "cornell_textured", "wavefront")]


def _fractional_id(p):
    ratio, size, scene_fn, variant = p
    tag = "default" if variant is None else variant if isinstance(variant, str) else \
        "-".join(f"{k}={v}" for k, v in variant.items())
    return f"{ratio}-{size[0]}x{size[1]}-{scene_fn}-{tag}"


@pytest.mark.parametrize("case", FRACTIONAL, ids=_fractional_id)
def test_fractional_upscale_ratio_bit_exact(hk_options, case):
    """Ratios 1.5, 1.3 and 1.7 with TAA Jasmine, emissive and indirect spatial reuse, two bounces and the
    denoiser, frames 0..5 (direct and emissive validation frames, both jitter parities, temporal and spatial
    history), every pass incl. the post-process: plane sizes, all 17 planes, the upscaled and TAA outputs, all
    10 reservoir buffers (the indexed prefix) and the counters.  Ratio 1.5 also with the merged light launch,
    the persistent-wave indirect pass, forced frame pipelining, no LDS scene staging and the wavefront
    indirect pass."""
    from hikari_amd import HikariSettings, Taa, Upscale, frame_inputs
    ratio, (w, h), scene_fn, variant = case
    if isinstance(variant, dict):
        hk_options.update(variant)
    st = HikariSettings(upscale=Upscale.smaa_tu4x(ratio), taa=Taa.Jasmine, emissive_spatial_reuse=True,
                        indirect_bounces=2, denoise=True)
    scene, cam, lights, r, o = pair(scene_fn, w, h, st, threads=0, wavefront=variant == "wavefront")
    s = st.to_c()
    sw, sh, _ = r.output_info(4)
    assert (sw, sh) != (w, h) and (w % sw or h % sh)  # the integrator grid is smaller and no divisor of S
    errors = []
    for f in range(6):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi, post=True)
        _check_sizes(r, o)
        compare_frame(r, o, f, errors, outputs=WITH_POST)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()


def test_fractional_ratio_moving_camera():
    """Ratio 1.5 at 63x47 under test_gpu_motion's orbit at 2 degrees per frame, spatial reuse off, the oracle
    single-threaded (raster order): reprojection at previous uvs scaled by s while the velocity plane is read
    at S.  As test_moving_camera_bit_exact: everything outside the racy spatial-pair scatter targets bit-exact,
    those within its tolerance."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    w, h = 63, 47
    st = HikariSettings(upscale=Upscale.smaa_tu4x(1.5), indirect_spatial_reuse=False, denoise=True)
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=1)
    s = st.to_c()
    errors = []
    prev = None
    moved = 0
    for f in range(4):
        c = orbit_camera(cam, f, angle_step=ic.ORBIT_2_DEGREES)
        fi = frame_inputs(f, c, lights, w, h, previous_camera=prev)
        prev = copy.deepcopy(c)
        for x in (r, o):
            passes(x, s, fi)
        compare_frame(r, o, f, errors, racy=RACY)
        vel = r.output(15).view(np.float32).reshape(h, w, 4)[..., :2]
        moved += int((vel != 0).any(axis=-1).sum())
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert moved > w * h  # the camera moved: most covered pixels carry a motion vector
    assert r.counters() == o.counters()


EDGE_RUNS = [(case, None) for case in ic.EDGE_CASES] + \
            [(case, k) for case in ic.EDGE_LAUNCH_CASES for k in range(len(ic.EDGE_LAUNCH_OPTIONS))]


@pytest.mark.parametrize("scene_fn", ic.EDGE_SCENES)
@pytest.mark.parametrize("case,launch", EDGE_RUNS,
                         ids=[c if k is None else f"{c}-{'fused' if k == 0 else 'separate_w4'}" for c, k in EDGE_RUNS])
def test_edge_settings_bit_exact(hk_options, case, launch, scene_fn):
    """One HikariSettings field (or pair) at an edge value over emissive spatial reuse, three bounces and the
    denoiser (inputs_cases.EDGE_CASES; each shown to change the frames by
    test_inputs_independent.py::test_edge_settings_change_the_frames), frames 0..4 at ratio 1: all planes,
    reservoirs and counters.  The interval-0 and reuse-count-0 cases also with the fused and with the separate
    (4 waves per SIMD) direct / emissive launches forced, so the host's per-frame variant pick
    (validation_frame: interval 0 -> every frame validates) meets the kernels' `number % 0 == 0`."""
    if launch is not None:
        hk_options.update(ic.EDGE_LAUNCH_OPTIONS[launch])
    run_static(scene_fn, *ic.EDGE_SIZE, ic.edge_settings(case), ic.EDGE_FRAMES, threads=0)


@pytest.mark.parametrize("jitter", [0, 2], ids=["static", "taa_smaa_jitter"])
@pytest.mark.parametrize("scene_fn", ["cornell", "scene"])
def test_orthographic_view_bit_exact(scene_fn, jitter):
    """An orthographic camera framing the scene (view.projection[3].w == 1: orthographic primary rays, the
    orthographic view vector in albedo and every light pass), default settings with emissive spatial reuse at
    ratio 1, frames 0..4, all passes incl. the post-process (SMAA TU4x + TAA); with and without the TAA + SMAA
    Halton jitter (HK_JITTER_TAA_SMAA)."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    w, h = 64, 48
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, emissive_spatial_reuse=True, denoise=True)
    scene, cam, lights, r, o = pair(scene_fn, w, h, st, threads=0)
    cam = ic.orthographic_camera(scene_fn, cam)
    s = st.to_c()
    errors = []
    positions = []
    for f in range(5):
        fi = frame_inputs(f, cam, lights, w, h, jitter=jitter)
        assert fi.view.projection[15] == 1.0
        for x in (r, o):
            passes(x, s, fi, post=True)
        compare_frame(r, o, f, errors, outputs=WITH_POST)
        positions.append(r.output(11).tobytes())
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()
    depth = r.output(11).view(np.float32).reshape(h, w, 4)[..., 3]
    assert (depth > 0).mean() > 0.25  # the camera sees the scene
    assert (len(set(positions)) > 1) == (jitter != 0)  # the jitter moved the primary rays


def test_orthographic_view_bit_exact_orbiting():
    """The orthographic camera orbiting the Cornell box over 3 frames (spatial reuse off, the oracle
    single-threaded): the planes outside the racy scatter targets bit-exact, the velocity plane (through
    view_proj and the previous view_proj, both orthographic) included and non-zero."""
    from hikari_amd import Camera, HikariSettings, Upscale, frame_inputs
    w, h = 64, 48
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False, denoise=True)
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=1)
    s = st.to_c()
    errors = []
    prev = None
    moved = 0
    for f in range(3):
        c = Camera.orthographic(orbit_camera(cam, f, angle_step=ic.ORBIT_2_DEGREES).transform,
                                ic.ORTHO_HEIGHT["cornell"])
        fi = frame_inputs(f, c, lights, w, h, previous_camera=prev)
        prev = copy.deepcopy(c)
        for x in (r, o):
            passes(x, s, fi)
        compare_frame(r, o, f, errors, racy=RACY)
        vel = r.output(15).view(np.float32).reshape(h, w, 4)[..., :2]
        moved += int((vel != 0).any(axis=-1).sum())
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert moved > w * h // 2
    assert r.counters() == o.counters()
