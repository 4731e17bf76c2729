"""The present pass on the GPU, byte for byte against the CPU side.

The renderer and the oracle (tests/parity.py's pair) run frames 0..3 with the post-process.  The oracle has no overlay;
include/hk_overlay.h's body (tests/overlay_cpu.c, built with the oracle's flags) is applied to the oracle's planes — the
input the settings display (for Fsr1: tests/fsr_cpu.c's RCAS of the oracle's TAA, as test_gpu_fsr.check_fsr builds it)
and the albedo (output 0) — and hk_present's target must hold the same bytes, f16 NaNs canonicalised.
tests/test_overlay_independent.py pins the CPU side to a second reading of the shader.  Every comparison runs under
option present_run 1 (16-byte row runs where the viewport's runs are aligned) and 0 (one thread per texel).
"""
import ctypes

import numpy as np
import pytest

from parity import canon_f16, compare_frame, hip_runtime, mismatch_report, pair, passes
from test_fsr_independent import FsrCpu
from test_overlay_independent import BPP, OverlayCpu, view

pytestmark = pytest.mark.gpu

RGBA8, BGRA8, RGBA16F = 0, 1, 2
FORMATS = (RGBA8, BGRA8, RGBA16F)
HK_ERR_INVALID, HK_ERR_STATE = -1, -3
FILL = 0xA5


@pytest.fixture(scope="module")
def ov(tmp_path_factory):
    return OverlayCpu(tmp_path_factory.mktemp("overlay_cpu"))


@pytest.fixture(scope="module")
def fsr(tmp_path_factory):
    return FsrCpu(tmp_path_factory.mktemp("fsr_cpu"))


def smaa(ratio, taa=True, **more):
    from hikari_amd import HikariSettings, Taa, Upscale
    return HikariSettings(upscale=Upscale.smaa_tu4x(ratio), taa=Taa.Jasmine if taa else Taa.None_, **more)


def oracle_planes(o, st, size, fsr=None):
    """(displayed plane, albedo) of the oracle as (h, w, 4) uint16: overlay.rs:227-231's choice."""
    albedo = o.output(0).view(np.uint16)
    if st.upscale.kind == "Fsr1":
        src = o.output(19 if st.taa.value == 0 else 10).view(np.uint16)
        easu = fsr.easu(src, *size)
        return fsr.rcas(easu, fsr.rcas_constant(st.upscale.sharpness())), albedo
    return o.output(19 if st.taa.value == 0 else 18).view(np.uint16), albedo


def canon(a, fmt):
    return canon_f16(a.view(np.uint16)) if fmt == RGBA16F else a


def check_own_plane(ov, r, s, src, alb, width, height, fmt, label, errors, input=-1):
    """hk_present into the context's own plane, in both present_run modes, against overlay_cpu."""
    want, _ = view(ov.present(src, alb, width, height, fmt), fmt, None, width, height)
    for run in (1, 0):
        r.set_option("present_run", run)
        got = r.present(s, width, height, fmt, input=input)
        assert got.shape == (height, width, 4) and got.dtype == (np.uint16 if fmt == RGBA16F else np.uint8)
        assert r.present_info() == (width, height, BPP[fmt], fmt)
        m = mismatch_report(canon(got, fmt), canon(want, fmt), f"{label} {width}x{height} format {fmt} run {run}")
        if m:
            errors.append(m)
    return want


def run_frames(ov, scene, size, st, targets, fsr=None, frames=4, formats=FORMATS):
    """Frames 0..frames-1 under the scene's static camera, each presented at every (width, height) of `targets` in
    every format; returns (renderer, oracle, camera, lights, (src, alb) of the last frame)."""
    from hikari_amd import frame_inputs
    w, h = size
    scene, cam, lights, r, o = pair(scene, w, h, st, threads=0)
    if st.upscale.kind == "Fsr1":
        r.set_fsr1_sharpness(st.upscale.sharpness())
    s = st.to_c()
    errors, planes = [], None
    for f in range(frames):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi, post=True)
        planes = oracle_planes(o, st, size, fsr)
        for (tw, th) in targets:
            for fmt in formats:
                check_own_plane(ov, r, s, *planes, tw, th, fmt, f"frame {f}", errors)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    return r, o, cam, lights, planes


def test_present_default_path(ov):
    """Case 1: cornell, S 64x48, ratio 2, SMAA TU4x + Jasmine: the input is the TAA plane (64x48).  Presented at the
    identity size, larger and smaller (odd: no aligned runs), all three formats, the context's own plane."""
    r, *_ = run_frames(ov, "cornell", (64, 48), smaa(2.0), [(64, 48), (128, 96), (37, 29)])
    assert r.output_info(19)[:2] == (64, 48)
    assert "present_run" in r.options()


def test_present_upscaled_plane_without_taa(ov):
    """Case 2a: textured cornell, ratio 1.5, S 63x47, Taa::None: the input is HK_OUT_UPSCALED."""
    r, o, *_ = run_frames(ov, "cornell_textured", (63, 47), smaa(1.5, taa=False), [(63, 47), (100, 61)])
    assert r.output_info(18)[:2] == o.output(18).shape[1::-1]


def test_present_fsr1_plane(ov, fsr):
    """Case 2b: scene.rs, Fsr1 ratio 1.3, 64x48: the input is output 22."""
    from hikari_amd import HikariSettings, Taa, Upscale
    st = HikariSettings(upscale=Upscale.fsr1(1.3, 0.2), taa=Taa.Jasmine)
    run_frames(ov, "scene", (64, 48), st, [(64, 48), (90, 70)], fsr=fsr)


def test_present_ratio_1_input_twice_the_albedo(ov):
    """Case 2c: cornell, ratio 1, 48x32: SMAA TU4x doubles, so the input is 2S (96x64) and the albedo S."""
    r, *_ = run_frames(ov, "cornell", (48, 32), smaa(1.0), [(48, 32), (96, 64)])
    assert r.output_info(19)[:2] == (96, 64) and r.output_info(0)[:2] == (48, 32)


def device_target(hip, nbytes):
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), nbytes) == 0
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    assert hip.hipMemset(p, FILL, nbytes) == 0 and hip.hipDeviceSynchronize() == 0
    return p


def read_back(hip, r, p, nbytes):
    r.sync()
    assert hip.hipDeviceSynchronize() == 0
    out = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, p, nbytes, 2) == 0
    return out


def test_present_caller_owned_target(ov):
    """Case 3: a 100x80 target of the caller's, prefilled with 0xA5, pitch 100 * bpp + 12 (RGBA16F: + 24, the nearest
    multiple of its 8-byte texel; + 12 itself is refused) — rows fall off the 16-byte grid: the per-texel kernel
    whatever the origin — and 100 * bpp + 16 (rows stay on it: the odd origin (5, 7) takes the per-texel kernel, the
    aligned one (4, 8) the run kernel); then `data` one texel past a 16-byte boundary.  Every byte outside the
    viewport is still 0xA5."""
    r, o, cam, lights, (src, alb) = run_frames(ov, "cornell", (64, 48), smaa(2.0), [], frames=2)
    s = smaa(2.0).to_c()
    hip = hip_runtime()
    errors = []
    W, H = 100, 80
    for fmt in FORMATS:
        b = BPP[fmt]
        if fmt == RGBA16F:  # 100 * 8 + 12 is no multiple of the 8-byte texel: refused, as the ABI states
            expect(r, HK_ERR_INVALID, s, W, H, fmt, dst_ptr=16, pitch=W * b + 12)
        for extra in (12 if b == 4 else 24, 16):
            pitch = W * b + extra
            for vp in ((5, 7, 64, 48), (4, 8, 64, 48)):
                want = ov.present(src, alb, W, H, fmt, vp, pitch, fill=FILL)
                for run in (1, 0):
                    r.set_option("present_run", run)
                    p = device_target(hip, pitch * H)
                    assert r.present(s, W, H, fmt, viewport=vp, dst_ptr=p.value, pitch=pitch) is None
                    got = read_back(hip, r, p, pitch * H).reshape(H, pitch)
                    hip.hipFree(p)
                    gv, g_out = view(got, fmt, vp, W, H)
                    wv, _ = view(want, fmt, vp, W, H)
                    m = mismatch_report(canon(gv, fmt), canon(wv, fmt), f"format {fmt} pitch +{extra} viewport {vp} run {run}")
                    if m:
                        errors.append(m)
                    assert (g_out == FILL).all(), f"format {fmt} pitch +{extra} viewport {vp} run {run}: wrote outside"
        # data one texel past a 16-byte boundary: a 99-texel-wide target inside the allocation
        pitch = W * b
        want = ov.present(src, alb, W - 1, H, fmt, None, pitch, fill=FILL)
        for run in (1, 0):
            r.set_option("present_run", run)
            p = device_target(hip, pitch * H + 16)
            assert p.value % 16 == 0
            r.present(s, W - 1, H, fmt, dst_ptr=p.value + b, pitch=pitch)
            got = read_back(hip, r, p, pitch * H + 16)
            hip.hipFree(p)
            assert (got[:b] == FILL).all() and (got[b + pitch * H:] == FILL).all()
            gv, g_out = view(got[b:b + pitch * H].reshape(H, pitch), fmt, None, W - 1, H)
            wv, _ = view(want, fmt, None, W - 1, H)
            m = mismatch_report(canon(gv, fmt), canon(wv, fmt), f"format {fmt} offset data run {run}")
            if m:
                errors.append(m)
            assert (g_out == FILL).all()
    assert not errors, "\n".join(errors[:20])


def test_present_nan_fallback_on_the_device(ov):
    """Case 4: f16 NaN / inf words copied into the input plane on the device (a full texel, an alpha-only NaN, a
    plane corner, an inf) and into the CPU side's copy: the targets match, the affected texels equal the albedo's
    sample and the others do not."""
    r, o, cam, lights, (src, alb) = run_frames(ov, "cornell", (64, 48), smaa(2.0), [], frames=4)
    s = smaa(2.0).to_c()
    hip = hip_runtime()
    w, h = r.output_info(19)[:2]
    src = src.copy()
    r.output(19)  # a blocking readback: the frame is complete
    r.sync()
    base = r.output_device_ptr(19)
    NAN, INF = 0x7E00, 0x7C00
    edits = [((20, 30), [NAN] * 4), ((10, 12), [None, None, None, NAN]), ((0, 0), [NAN, None, None, None]),
             ((h - 1, w - 1), [None, NAN, None, None]), ((33, 40), [INF, None, None, None])]
    clean_src = src.copy()
    nan_src = src.copy()  # the NaN words alone: what falls back because of them
    for (y, x), words in edits:
        for k, word in enumerate(words):
            if word is None:
                continue
            v = np.array([word], np.uint16)
            assert hip.hipMemcpy(base + ((y * w + x) * 4 + k) * 2, v.ctypes.data, 2, 1) == 0
            src[y, x, k] = word
            if word == NAN:
                nan_src[y, x, k] = word
    assert hip.hipDeviceSynchronize() == 0
    got_in = r.output(19).view(np.uint16)
    assert np.array_equal(got_in, src)
    errors = []
    for (tw, th) in ((64, 48), (128, 96), (37, 29)):
        for fmt in FORMATS:
            check_own_plane(ov, r, s, src, alb, tw, th, fmt, "NaN", errors)
            shown = [view(ov.present(p, alb, tw, th, fmt), fmt, None, tw, th)[0] for p in (nan_src, clean_src, alb)]
            with_nan, clean, albedo_only = [canon(p, fmt) for p in shown]
            affected = (with_nan != clean).any(axis=-1)
            assert affected.sum() >= 4, (tw, th, fmt)
            # every texel the NaNs changed holds the albedo's sample (the albedo presented as the input, same uv);
            # the others hold what they held, which over most of the frame is not the albedo
            assert (with_nan[affected] == albedo_only[affected]).all(), (tw, th, fmt)
            assert (with_nan[~affected] != albedo_only[~affected]).any(axis=-1).mean() > 0.3, (tw, th, fmt)
    assert not errors, "\n".join(errors[:20])


def test_present_hdr_black_clear_colour(ov):
    """Case 5: clear colour black, RGBA16F: the background's luminance is 0, so the inverse Reinhard stores NaN there
    (0 * inf), bit for bit as the CPU side; covered texels are finite and brighter than their input."""
    st = smaa(2.0, clear_color=(0.0, 0.0, 0.0, 1.0))
    r, o, cam, lights, (src, alb) = run_frames(ov, "cornell", (64, 48), st, [(64, 48), (128, 96)], formats=(RGBA16F,))
    out = r.present(st.to_c(), 64, 48, RGBA16F).view(np.float16).astype(np.float32)
    inp = src.view(np.float16).astype(np.float32)

    def lum(c):
        return c[..., 0] * 0.2126 + c[..., 1] * 0.7152 + c[..., 2] * 0.0722
    black = lum(inp) == 0
    assert 0.02 < black.mean() < 0.98
    # a texel whose whole footprint is black is NaN; one with luminance well inside the clamp grows
    inner = np.zeros_like(black)
    inner[1:-1, 1:-1] = black[1:-1, 1:-1] & black[:-2, 1:-1] & black[2:, 1:-1] & black[1:-1, :-2] & black[1:-1, 2:]
    assert inner.any() and np.isnan(out[inner][:, :3]).all()
    lit = (lum(inp) > 0.01) & (lum(inp) < 0.9)
    lit[0, :] = lit[-1, :] = lit[:, 0] = lit[:, -1] = False
    near = lit.copy()
    near[1:-1, 1:-1] &= lit[:-2, 1:-1] & lit[2:, 1:-1] & lit[1:-1, :-2] & lit[1:-1, 2:]
    assert near.sum() > 100 and np.isfinite(out[near]).all() and (lum(out[near]) > lum(inp[near])).all()


def expect(r, code, s, *args, **kw):
    from hikari_amd import HikariError
    with pytest.raises(HikariError) as e:
        r.present(s, *args, **kw)
    assert f"({code})" in str(e.value) and str(e.value).split(":", 1)[1].strip(), str(e.value)


def test_present_errors_and_state(ov):
    """Case 6: HK_ERR_STATE before the first hk_post_process and before the first own-plane present; each invalid
    descriptor HK_ERR_INVALID with a message and no launch; hk_present_info follows a format change; the frame after
    a present is still bit-exact against the oracle."""
    from hikari_amd import HikariError, _abi, frame_inputs
    st = smaa(2.0)
    s = st.to_c()
    w, h = 64, 48
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=0)
    expect(r, HK_ERR_STATE, s, w, h)  # no TAA plane yet
    with pytest.raises(HikariError):
        r.present_info()
    with pytest.raises(HikariError):
        r.get_present()
    for f in range(2):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi, post=True)
    with pytest.raises(HikariError):
        r.present_info()  # still no own-plane present
    hip = hip_runtime()
    p = device_target(hip, 100 * 80 * 8 + 16)
    r.enable_kernel_timing(True)  # clears the sums
    t = _abi.hk_present_target(None, w, h, 0, 3, 0, 0, 0, 0, -1)                 # unknown format (past the mirror's enum)
    assert _abi.lib().hk_present(r.ctx, ctypes.byref(s), ctypes.byref(t), None) == HK_ERR_INVALID
    assert b"format" in _abi.lib().hk_last_error(r.ctx)
    expect(r, HK_ERR_INVALID, s, w, h, input=11)                             # an f32 plane
    expect(r, HK_ERR_INVALID, s, w, h, input=23)                             # no such plane
    expect(r, HK_ERR_INVALID, s, w, h, viewport=(1, 0, w, h))                # viewport outside the target
    expect(r, HK_ERR_INVALID, s, w, h, viewport=(0, 0, w, h + 1))
    expect(r, HK_ERR_INVALID, s, 0, h)                                       # zero dimensions
    expect(r, HK_ERR_INVALID, s, w, 0)
    expect(r, HK_ERR_INVALID, s, w, h, viewport=(0, 0, 8, 0))
    expect(r, HK_ERR_INVALID, s, 100, 80, dst_ptr=p.value, pitch=100 * 4 - 4)       # pitch below a row
    expect(r, HK_ERR_INVALID, s, 100, 80, dst_ptr=p.value, pitch=100 * 4 + 2)       # not a multiple of the texel
    expect(r, HK_ERR_INVALID, s, 100, 80, RGBA16F, dst_ptr=p.value, pitch=100 * 8 + 4)
    expect(r, HK_ERR_INVALID, s, 100, 80, dst_ptr=p.value + 2)                      # data off the texel size
    expect(r, HK_ERR_INVALID, s, 100, 80, RGBA16F, dst_ptr=p.value + 4)
    expect(r, HK_ERR_INVALID, s, w, h, pitch=w * 4 + 16)                            # the own plane is packed
    expect(r, HK_ERR_STATE, s, w, h, input=22)                                      # no FSR1 plane on this context
    assert "present" not in r.kernel_timing()  # none of them launched anything
    assert (read_back(hip, r, p, 100 * 80 * 8 + 16) == FILL).all()
    hip.hipFree(p)
    src, alb = oracle_planes(o, st, (w, h))
    errors = []
    check_own_plane(ov, r, s, src, alb, w, h, RGBA8, "first", errors)
    assert "present" in r.kernel_timing()
    check_own_plane(ov, r, s, src, alb, w, h, RGBA16F, "format change", errors)
    assert r.present_info() == (w, h, 8, RGBA16F)
    check_own_plane(ov, r, s, src, alb, 40, 30, BGRA8, "size change", errors)
    assert r.present_info() == (40, 30, 4, BGRA8)
    # a debug view: the tone-mapped plane (32x24 at ratio 2) and the albedo itself, settings not needed
    check_own_plane(ov, r, None, o.output(10).view(np.uint16), alb, w, h, RGBA8, "tone-mapped", errors, input=10)
    check_own_plane(ov, r, None, alb, alb, w, h, RGBA8, "albedo", errors, input=0)
    r.enable_kernel_timing(False)
    # the joins did not disturb the pipeline: the next frames, with a present after each, still match the oracle
    for f in (2, 3):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi, post=True)
        r.present(s, w, h)
        compare_frame(r, o, f, errors, outputs=(0, 10, 19), rids=())
    assert not errors, "\n".join(errors[:20])
    r.resize(w, h, 2.0)
    with pytest.raises(HikariError):
        r.present_info()  # released with the other targets


def test_present_between_pipelined_frames(ov):
    """Frames 0..5 queued without a readback on a context that pipelines at this size (G-buffer and tail on their own
    streams), each presented into one of two alternating targets of the caller's: every target holds its own frame,
    so the present waited for the frame's tail and the later G-buffers, which rewrite the albedo slot it reads,
    waited for it; the last frame still matches the oracle."""
    from hikari_amd import frame_inputs
    w, h = 64, 48
    st = smaa(2.0)
    s = st.to_c()
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=0, options={"pipeline_min_px": 0})
    hip = hip_runtime()
    nbytes = w * h * 4
    bufs = [device_target(hip, nbytes) for _ in range(2)]
    want = {}
    for f in range(6):
        fi = frame_inputs(f, cam, lights, w, h)
        passes(r, s, fi, post=True)
        r.present(s, w, h, RGBA8, dst_ptr=bufs[f & 1].value)
        passes(o, s, fi, post=True)
        want[f] = ov.present(*oracle_planes(o, st, (w, h)), w, h, RGBA8)
    errors = []
    for f in (4, 5):
        got = read_back(hip, r, bufs[f & 1], nbytes).reshape(h, w * 4)
        m = mismatch_report(got, want[f], f"frame {f} target")
        if m:
            errors.append(m)
    compare_frame(r, o, 5, errors, outputs=(0, 10, 19), rids=())
    assert not errors, "\n".join(errors)
    for b in bufs:
        hip.hipFree(b)


def test_present_through_the_plugin(ov):
    """Case 7: HikariPlugin.present() returns the renderer call's bytes with the plugin's settings: the physical size
    by default, RGBA16F under hdr, a viewport."""
    from hikari_amd import HikariPlugin, examples, frame_inputs, load_noise
    from oracle import Oracle
    w, h = 64, 48
    st = smaa(2.0)
    scene, cam, lights = examples.cornell()
    plugin = HikariPlugin(scene, st)
    plugin.resize(w, h)
    r = plugin.renderer
    o = Oracle(scene.desc if scene.desc is not None else scene.build(), load_noise(), w, h, 2.0)
    s = st.to_c()
    for f in range(4):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi, post=True)
    src, alb = oracle_planes(o, st, (w, h))
    for run in (1, 0):
        r.set_option("present_run", run)
        got = plugin.present()
        assert got.shape == (h, w, 4) and got.dtype == np.uint8
        assert np.array_equal(got, r.present(s, w, h, "rgba8_srgb"))
        want, _ = view(ov.present(src, alb, w, h, RGBA8), RGBA8, None, w, h)
        assert np.array_equal(got, want)
        hdr = plugin.present(hdr=True)
        assert hdr.dtype == np.uint16 and np.array_equal(canon_f16(hdr), canon_f16(r.present(s, w, h, RGBA16F)))
        part = plugin.present(80, 60, viewport=(8, 6, 64, 48))
        want = ov.present(src, alb, 80, 60, RGBA8, (8, 6, 64, 48), fill=0)
        wv, _ = view(want, RGBA8, (8, 6, 64, 48), 80, 60)
        assert np.array_equal(part[6:54, 8:72], wv)
