"""FSR1 on the GPU, word for word against the CPU side.

The renderer and the oracle (tests/parity.py's pair) run G-buffer, light passes, denoiser, tone sum and the
post-process with `Upscale.fsr1`.  The oracle has no FSR1 pass and stops after the TAA; include/hk_fsr.h's bodies
(tests/fsr_cpu.c, built with the oracle's flags) are then applied to the oracle's TAA output (output 19), or to its
tone-mapped plane (output 10) when the TAA is off, and the GPU's outputs 21 (EASU) and 22 (RCAS) must hold the same
words, f16 NaNs canonicalised.  tests/test_fsr_independent.py pins the CPU side to a second reading of the shaders.
Unless a case says otherwise it runs with option fsr_tiled 1 (input footprint staged in LDS) and 0 (plain).
"""
import copy
import ctypes

import numpy as np
import pytest

from parity import canon_f16, compare_frame, hip_runtime, mismatch_report, orbit_camera, pair, passes
from test_fsr_independent import FsrCpu

pytestmark = pytest.mark.gpu

TILED = pytest.mark.parametrize("tiled", [1, 0], ids=["tiled", "plain"])


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return FsrCpu(tmp_path_factory.mktemp("fsr_cpu"))


def settings(ratio, sharpness=0.0, taa=True, **more):
    from hikari_amd import HikariSettings, Taa, Upscale
    return HikariSettings(upscale=Upscale.fsr1(ratio, sharpness), taa=Taa.Jasmine if taa else Taa.None_, **more)


def check_fsr(cpu, r, o, st, size, frame, errors):
    """GPU outputs 21 / 22 and their hk_output_info against the shared bodies on the oracle's EASU input."""
    w, h = size
    taa = st.taa.value == 0
    src = o.output(19 if taa else 10).view(np.uint16)
    got_in = r.output(19 if taa else 10).view(np.uint16)
    m = mismatch_report(canon_f16(got_in), canon_f16(src), f"frame {frame} EASU input")
    if m:
        errors.append(m)
    easu = cpu.easu(src, w, h)
    rcas = cpu.rcas(easu, cpu.rcas_constant(st.upscale.sharpness()))
    for oid, want in ((21, easu), (22, rcas)):
        assert r.output_info(oid) == (w, h, 8)
        m = mismatch_report(canon_f16(r.output(oid).view(np.uint16)), canon_f16(want), f"frame {frame} output {oid}")
        if m:
            errors.append(m)
    return easu, rcas


def run(cpu, scene, size, st, tiled, frames=4, threads=0):
    """Frames 0..frames-1 under the scene's static camera; returns (renderer, oracle, camera, lights, last planes)."""
    from hikari_amd import frame_inputs
    w, h = size
    scene, cam, lights, r, o = pair(scene, w, h, st, threads=threads, options={"fsr_tiled": tiled})
    r.set_fsr1_sharpness(st.upscale.sharpness())
    s = st.to_c()
    errors, planes = [], None
    for f in range(frames):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi, post=True)
        planes = check_fsr(cpu, r, o, st, size, f, errors)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    return r, o, cam, lights, planes


@TILED
def test_fsr1_ratio_2_then_smaa_on_the_same_context(cpu, tiled):
    """Case 1: cornell, ratio 2, S 64x48, TAA Jasmine, frames 0..3.  Then hk_post_process with upscale = 0 on the same
    context: outputs 18 and 19 equal the oracle's (the TAA planes are reallocated at SMAA's size)."""
    from hikari_amd import HikariSettings, Taa, Upscale, frame_inputs
    size = (64, 48)
    r, o, cam, lights, (easu, rcas) = run(cpu, "cornell", size, settings(2.0), tiled)
    assert r.output_info(19)[:2] == (32, 24)
    assert np.isfinite(easu.view(np.float16).astype(np.float32)).all() and not np.array_equal(easu, rcas)
    smaa = HikariSettings(upscale=Upscale.smaa_tu4x(2.0), taa=Taa.Jasmine).to_c()
    errors = []
    for f in (4, 5):
        fi = frame_inputs(f, cam, lights, *size)
        for x in (r, o):
            passes(x, smaa, fi, post=True)
        compare_frame(r, o, f, errors, outputs=(10, 18, 19), rids=())
    assert not errors, "\n".join(errors)
    assert r.output_info(19)[:2] == (64, 48) and r.output_info(22) == (64, 48, 8)


@TILED
def test_fsr1_fractional_ratio_odd_sizes(cpu, tiled):
    """Case 2: textured cornell, ratio 1.5, S 63x47 (s 42x32): odd sizes, partial 16x16 blocks."""
    r, *_ = run(cpu, "cornell_textured", (63, 47), settings(1.5), tiled)
    assert r.output_info(4)[:2] == (42, 32)


@TILED
@pytest.mark.parametrize("ratio,size", [(1.3, (64, 48)), (1.7, (62, 41))], ids=["1.3", "1.7"])
def test_fsr1_scene_with_directional_light(cpu, tiled, ratio, size):
    """Case 3: scene.rs (directional light, bright edges) at ratios 1.3 and 1.7."""
    run(cpu, "scene", size, settings(ratio), tiled)


@TILED
def test_fsr1_ratio_1(cpu, tiled):
    """Case 4: ratio 1, S 48x32: s = S."""
    r, *_ = run(cpu, "cornell", (48, 32), settings(1.0), tiled)
    assert r.output_info(19)[:2] == (48, 32)


@TILED
def test_fsr1_without_taa_reads_the_tone_mapped_plane(cpu, tiled):
    """Case 5: Taa.None_: EASU's input is the tone-mapped plane."""
    run(cpu, "cornell", (64, 48), settings(2.0, taa=False), tiled)


@TILED
def test_fsr1_black_clear_colour(cpu, tiled):
    """Case 6: clear colour black: large areas where RCAS's limiters are 0 * rcp(0) = NaN and max(NaN, x) = x decides."""
    r, o, cam, lights, (easu, rcas) = run(cpu, "cornell", (64, 48), settings(2.0, clear_color=(0.0, 0.0, 0.0, 1.0)), tiled)
    rgb = rcas.view(np.float16).astype(np.float32)[..., :3]
    assert np.isfinite(rgb).all() and (rgb == 0).all(axis=-1).mean() > 0.05


@TILED
@pytest.mark.parametrize("sharpness", [0.0, 0.2, 2.0])
def test_fsr1_sharpness_through_the_plugin(cpu, tiled, sharpness):
    """Case 7: sharpness set by HikariPlugin.resize from settings.upscale.sharpness(); the plugin's renderer then
    runs the frames, post-process included."""
    from hikari_amd import HikariPlugin, examples, frame_inputs, load_noise
    from oracle import Oracle
    w, h = 64, 48
    st = settings(2.0, sharpness)
    scene, cam, lights = examples.cornell()
    plugin = HikariPlugin(scene, st)
    plugin.renderer.set_option("fsr_tiled", tiled)
    plugin.resize(w, h)
    r = plugin.renderer
    o = Oracle(scene.desc if scene.desc is not None else scene.build(), load_noise(), w, h, 2.0)
    s = st.to_c()
    errors = []
    for f in range(4):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi, post=True)
        check_fsr(cpu, r, o, st, (w, h), f, errors)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])


@TILED
def test_fsr1_orbiting_camera(cpu, tiled):
    """Case 8: ratio 1.5, S 63x47, 3 frames of an orbiting camera.  FSR1 has no history, so it is bit-exact under
    motion whenever its input is: Taa.None_ and no spatial reuse."""
    from hikari_amd import frame_inputs
    w, h = 63, 47
    st = settings(1.5, taa=False, indirect_spatial_reuse=False)
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=1, options={"fsr_tiled": tiled})
    s = st.to_c()
    errors, prev = [], None
    for f in range(3):
        c = orbit_camera(cam, f)
        fi = frame_inputs(f, c, lights, w, h, previous_camera=prev)
        prev = copy.deepcopy(c)
        for x in (r, o):
            passes(x, s, fi, post=True)
        check_fsr(cpu, r, o, st, (w, h), f, errors)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])


def test_fsr1_on_caller_streams(cpu):
    """Case 9 (tiled only): every call of frames 0..3 on a stream of the caller's, queued without a readback, and
    each frame's displayed plane (output 22) copied on a second stream into one of two alternating device buffers.
    Every copy holds its own frame's plane, so the copy waited for RCAS and the next frame's RCAS waited for the
    copy (ext_wait on the plane); the last frame is then read back as usual (ev_post ordered the G-buffers)."""
    from hikari_amd import _abi, frame_inputs
    hip = hip_runtime()
    w, h = 64, 48
    st = settings(2.0, 0.2)
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=0, options={"fsr_tiled": 1})
    r.set_fsr1_sharpness(st.upscale.sharpness())
    s = st.to_c()
    frame_stream, copy_stream = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(frame_stream)) == 0 and hip.hipStreamCreate(ctypes.byref(copy_stream)) == 0
    nbytes = w * h * 8
    bufs = [ctypes.c_void_p(), ctypes.c_void_p()]
    for b in bufs:
        assert hip.hipMalloc(ctypes.byref(b), nbytes) == 0
    want = {}
    for f in range(4):
        fi = frame_inputs(f, cam, lights, w, h)
        r.render_gbuffer(fi, frame_stream.value)
        r.render_frame(s, fi, frame_stream.value)
        r.denoise(s, fi, frame_stream.value)
        r.tone_sum(s, frame_stream.value)
        r.post_process(s, fi, frame_stream.value)
        r.copy_output_rows(_abi.OUT_FSR_RCAS, 0, h, bufs[f & 1].value, False, copy_stream.value)
        passes(o, s, fi, post=True)
        easu = cpu.easu(o.output(19).view(np.uint16), w, h)
        want[f] = cpu.rcas(easu, cpu.rcas_constant(0.2))
    assert hip.hipStreamSynchronize(copy_stream) == 0 and hip.hipStreamSynchronize(frame_stream) == 0
    for f in (2, 3):
        out = np.empty((h, w, 4), np.uint16)
        assert hip.hipMemcpy(out.ctypes.data, bufs[f & 1], nbytes, 2) == 0
        m = mismatch_report(canon_f16(out), canon_f16(want[f]), f"frame {f} copied plane")
        assert not m, m
    errors = []
    check_fsr(cpu, r, o, st, (w, h), 3, errors)
    assert not errors, "\n".join(errors)
    for b in bufs:
        hip.hipFree(b)
    hip.hipStreamDestroy(copy_stream)
    hip.hipStreamDestroy(frame_stream)


def test_fsr1_outputs_absent_before_the_first_pass_and_sharpness_checked():
    from hikari_amd import HikariError, _abi, examples
    from parity import renderer
    scene, cam, lights = examples.cornell()
    r = renderer(scene, (32, 24), 2.0)
    for oid in (_abi.OUT_FSR_EASU, _abi.OUT_FSR_RCAS):
        assert r.output_device_ptr(oid) is None
        with pytest.raises(HikariError):
            r.output_info(oid)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(HikariError):
            r.set_fsr1_sharpness(bad)
    r.set_fsr1_sharpness(-1.0)  # not clamped
    assert r.get_option("fsr_tiled") in (0.0, 1.0)
