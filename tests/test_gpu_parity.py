"""GPU parity: the HIP path (libhikari_amd.so, via the C ABI) against the CPU oracle,
bit-exact on every output plane and reservoir buffer (NaN payloads canonicalised).

Scenes: cornell (examples/cornell.rs) at small sizes; frames 0..N so that validation frames
(number % 3 == 0 and % 5 == 0), temporal reuse and the spatial pass are all exercised.
"""
import numpy as np
import pytest

from parity import (RACY, assert_instance_update_matches_host, canon_plane, compare_frame, core_agreement, decomposed,
                    hip_runtime, mismatch_report, moved, pair, passes, renderer, run_frames, run_static, summed_counters)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["1", "0", "2"], ids=["lds_default", "lds_off", "lds_all"])
def lds_mode(request, hk_options):
    """Option lds_scene: scene arrays staged in LDS by the default kernels / none / every traversal kernel."""
    hk_options["lds_scene"] = int(request.param)
    return request.param


@pytest.mark.parametrize("size", [(64, 64), (96, 72), (63, 47), (256, 256)])
def test_cornell_frames_bit_exact(size, lds_mode):
    """(256, 256): BASELINE configs[0] (examples/cornell.rs 256x256, all passes incl. spatial reuse
    and the denoiser).  (63, 47): odd sizes — partial 16x16 tiles on both edges, and the tone pass's
    tile kernel (k_tone; even widths take the 2-pixel-run kernel)."""
    from hikari_amd import HikariSettings, Upscale
    run_static("cornell", size[0], size[1], HikariSettings(upscale=Upscale.SMAA_TU_1_0), 7)


# uneven 8-band split of city 3840x2160 (cost-balanced bands as bench.py's calibration produces them:
# narrow bands over the houses and the sphere in the lower half)
CITY_UNEVEN = [0, 464, 848, 1104, 1296, 1488, 1688, 1904, 2160]


@pytest.mark.parametrize("config,frames,uneven", [("cornell-1080p-nee", 4, False), ("scene-1080p-full", 2, False),
                                                  ("city-4k", 2, False), ("city-4k", 2, True), ("city-4k", 2, "tiles")],
                         ids=["cornell-1080p-nee-4", "scene-1080p-full-2", "city-4k-2", "city-4k-uneven-2",
                              "city-4k-tiles-2"])
def test_full_size_bench_workloads_bit_exact(config, frames, uneven):
    """The bench workloads themselves (BASELINE configs 2-4 at 1920x1080 and 3840x2160): every output plane
    of every frame, all reservoir buffers of the last frame and the ray counters bit-exact; for city 4K
    the 8-band decomposition of configs[3] too (each band's core rows of the tone-mapped frame), with
    equal bands and with uneven (cost-balanced) ones, and the 8-tile one (4 row bands x 2 column bands of
    1920 x 540, hk_resize_tile: each tile's core rectangle, and the tiles' ray counts summing to the frame's)."""
    import bench
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    from hikari_amd.bands import halo_rows
    cfg = bench.CONFIGS[config]
    w, h = cfg["width"], cfg["height"]
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=cfg["spatial"], denoise=cfg["denoise"])
    scene, cam, lights, r, o = pair(cfg["scene"], w, h, st)
    s = st.to_c()
    # city 4K: also BASELINE configs[3]'s own decomposition, 8 row bands of 270 rows + halo (one context
    # per band, as the 8 ranks of bench.py --gpus 8 hold them), core rows against the whole-frame oracle
    bands = []
    if config == "city-4k":
        bands = decomposed(scene, 8, w, h, "tiles" if uneven == "tiles" else "bands",
                           halo_rows(cfg["spatial"], cfg["denoise"]), CITY_UNEVEN if uneven is True else None)
    errors = []
    for f in range(frames):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in [r, o] + [rb for _, rb in bands]:
            passes(x, s, fi)
        whole = canon_plane(10, o.output(10))
        for b, rb in bands:
            row0, rows, core0, core_rows = rb.band_info()
            assert row0 + core0 == b.y0 and core_rows == b.rows == (b.rows if uneven else h // 8)
            if uneven == "tiles":
                assert rb.tile_info() == (b.x0, b.cols)
                x0, x1 = b.x0, b.x0 + b.cols
                mine = canon_plane(10, np.ascontiguousarray(rb.output(10)[core0: core0 + core_rows, x0:x1]))
                ref = canon_plane(10, np.ascontiguousarray(o.output(10)[b.y0: b.y0 + b.rows, x0:x1]))
            else:
                mine = canon_plane(10, rb.output(10)[core0: core0 + core_rows])
                ref = whole[b.y0: b.y0 + b.rows]
            m = mismatch_report(mine, ref, f"frame {f} band {b.y0}+{b.rows} output 10")
            if m:
                errors.append(m)
        compare_frame(r, o, f, errors, rids=())
        if errors:
            break
    compare_frame(r, o, "last", errors, outputs=())  # the reservoir buffers after the last frame only
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()
    if uneven == "tiles":  # the tiles count their own pixels' rays: together the frames' rays, once each
        assert summed_counters(bands) == o.counters()


@pytest.mark.parametrize("denoise,mode", [(True, "forced"), (False, "forced"), (True, "serial")],
                         ids=["denoise", "tone_only", "denoise_serial"])
def test_frame_pipelining_bit_exact(hk_options, denoise, mode):
    """Frame pipelining forced on a small frame (option pipeline_min_px=0): the G-buffer of frame f on
    its own stream next to frame f-1's light passes, frame f's tail (denoise, tone-sum) next to
    frame f+1's; every plane, reservoir and counter of every frame as the oracle's serial run,
    with readbacks after each frame and without (outputs compared after the last frame only).
    (Frames with spatial reuse pipeline at every size by default, pipeline_heavy_min_px = 0; "serial" keeps
    them in series: pipeline_heavy_min_px above the frame.)"""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    if mode == "forced":
        hk_options["pipeline_min_px"] = 0
    else:
        hk_options["pipeline_heavy_min_px"] = 1e12
    w, h = 96, 72
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=True, denoise=denoise)
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    s = st.to_c()
    errors = []
    frames = 9
    for f in range(frames):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi)
        if f < 3 or f == frames - 1:  # frames 3..7 run back to back, no readback in between
            compare_frame(r, o, f, errors)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()


def test_heavy_frame_schedule_switches_bit_exact(hk_options):
    """The schedule follows the settings (pipeline_size: a frame with spatial reuse or after a denoised frame
    pipelines at any size, a frame of traversal + NEE alone below pipeline_min_px does not): a sequence that
    turns spatial reuse and the denoiser off and on again switches between the pipelined and the serial
    schedule (and the merged light launch) from frame to frame, and every frame equals the oracle's."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    w, h = 96, 72
    heavy = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=True, denoise=True)
    light = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False, denoise=False)
    scene, cam, lights, r, o = pair("cornell", w, h, heavy)
    errors = []
    for f, st in enumerate([heavy, heavy, light, light, heavy, light, heavy, heavy]):
        s = st.to_c()
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi)
        if f % 2 == 1 or f == 7:
            compare_frame(r, o, f, errors)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()


def test_device_pointer_after_sync_is_current(hk_options):
    """The zero-copy route of INTEGRATION.md §3: with frame pipelining forced on, a reader that takes
    hk_output_device_ptr and makes its own stream wait with hk_sync reads the frame's finished
    planes (tone-mapped, denoised, G-buffer) — copied with hipMemcpyAsync on that stream, bit-equal
    to the oracle's — without any other readback in between."""
    import ctypes

    from hikari_amd import HikariSettings, Upscale, frame_inputs
    hk_options["pipeline_min_px"] = 0
    hip = hip_runtime()
    w, h = 96, 72
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=True, denoise=True)
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    s = st.to_c()
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0  # the reader's own stream
    for f in range(6):
        fi = frame_inputs(f, cam, lights, w, h)
        for x in (r, o):
            passes(x, s, fi)
        r.sync(stream)
        for oid in (10, 7, 8, 9, 11, 15):  # tone-mapped, denoised x3, G-buffer position, velocity
            cw, ch, b = r.output_info(oid)
            dst = np.empty((ch, cw, b), np.uint8)
            ptr = r.output_device_ptr(oid)
            assert ptr
            assert hip.hipMemcpyAsync(dst.ctypes.data, ptr, dst.nbytes, 2, stream) == 0
            assert hip.hipStreamSynchronize(stream) == 0
            m = mismatch_report(canon_plane(oid, dst), canon_plane(oid, o.output(oid)), f"frame {f} output {oid}")
            assert not m, m
    hip.hipStreamDestroy(stream)


def test_fallback_paths_bit_exact(hk_options):
    """The paths the defaults switch off stay exact: one stream (no channel fork), walk nodes
    without leaf collapse, the G-buffer stack with its scratch overflow levels."""
    from hikari_amd import HikariSettings, Upscale
    hk_options.update(channel_streams=0, leaf_collapse=0, gbuffer_deep=1)
    run_static("cornell", 64, 48, HikariSettings(upscale=Upscale.SMAA_TU_1_0), 4)


def test_trace_matches_oracle():
    from hikari_amd import HikariSettings, Upscale
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0)
    scene, cam, lights, r, o = pair("cornell", 16, 16, st)
    rng = np.random.default_rng(7)
    n = 20000
    org = rng.uniform([-1.2, -0.2, -1.2], [1.2, 2.2, 1.2], (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:100, 0] = 0.0  # axis-parallel rays: 1/0 = inf in the slab test
    rays = np.concatenate([org, d], axis=1).astype(np.float32)
    early = np.where(rng.random(n) < 0.5, 0.0, 65535.0).astype(np.float32)
    excl = rng.integers(0, 9, n).astype(np.uint32)
    a = r.trace(rays, None, early, excl)
    b = o.trace(rays, None, early, excl)
    assert (a == b).all(), f"{int((a != b).any(axis=1).sum())} of {n} rays differ"
    assert (a[:, 3] != 0xFFFFFFFF).mean() > 0.5


@pytest.mark.parametrize("spatial,denoise,world,H", [(True, True, 2, 96), (False, False, 2, 96), (True, True, 4, 192),
                                                     (True, False, 3, 192), (False, True, 3, 192),
                                                     ("indirect", True, 3, 192)])
def test_gpu_row_bands_match_whole_frame(spatial, denoise, world, H):
    """Band contexts (the multi-GPU decomposition, run on one GPU) reproduce the whole-frame
    oracle render bit-exactly on their own rows, and count only their own rays.  At H = 192 the
    bands' halos and the per-pass row windows (hk_runtime.hip pass_window: G-buffer and temporal
    passes on core +-36, spatial reuse +-16, demodulation +-15, the a-trous levels +-7/3/1/0) are
    strict parts of the frame, over 5 frames of reservoir history.  spatial = "indirect": indirect
    spatial reuse alone (the bench configs), where the direct / emissive launch runs on core +-16 only."""
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs, load_noise
    from hikari_amd.bands import halo_rows
    from oracle import Oracle
    W = 64
    scene, cam, lights = examples.cornell()
    desc = scene.build()
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=bool(spatial),
                        emissive_spatial_reuse=spatial is True, denoise=denoise)
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, 1.0)
    ranks = decomposed(scene, world, W, H, "bands", halo_rows(bool(spatial), denoise))
    for f in range(5):
        fi = frame_inputs(f, cam, lights, W, H)
        for x in [o] + [r for _, r in ranks]:
            passes(x, s, fi)
    whole = o.output(10)
    for b, r in ranks:
        row0, rows, core0, core_rows = r.band_info()
        assert row0 + core0 == b.y0 and core_rows == b.rows
        mine = r.output(10)[core0: core0 + core_rows]
        assert np.array_equal(canon_plane(10, mine), canon_plane(10, whole[b.y0: b.y0 + b.rows])), b
    assert summed_counters(ranks) == o.counters()


@pytest.mark.parametrize("refill", [True, False], ids=["refill", "zero_fill"])
def test_gpu_row_bands_settings_toggle(refill):
    """A band's light-pass windows depend on the settings (hk_runtime.hip pass_window: each channel's temporal pass on
    core +-(OUT + its spatial range)); turning the denoiser on at frame 4 widens every window, emissive spatial reuse
    at frame 6 the direct / emissive one.  The rows a window takes in hold no history of this band; their owner bands
    hold it exactly, and bands.refill_windows_local copies it over (hk_band_window_grow + hk_reservoir_rows) before the
    frame: every band's core rows equal the whole-frame render bit for bit on every frame.
    Without the refill (zero_fill) hk_render_frame zero-fills the new rows (hk_resize's state): exact before the first
    widening; afterwards the new rows' ReSTIR chains restart and the denoiser spreads the difference over the core rows
    (measured 47-78 % of pixels exact, mean relative difference <= 5.5e-3: profiles/r06/c2), held to <= 1e-2."""
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs, load_noise
    from hikari_amd.bands import halo_rows, refill_windows_local
    from oracle import Oracle
    W, H, world = 64, 192, 3
    scene, cam, lights = examples.cornell()
    desc = scene.build()

    def settings(emissive, denoise):
        return HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=True,
                              emissive_spatial_reuse=emissive, denoise=denoise).to_c()
    # (emissive spatial reuse, denoise) per frame: denoise on at 4, emissive spatial reuse on at 6, off at 8, on at 9
    plan = [(False, False)] * 4 + [(False, True)] * 2 + [(True, True)] * 2 + [(False, True), (True, True), (True, True)]
    o = Oracle(desc, load_noise(), W, H, 1.0)
    ranks = decomposed(scene, world, W, H, "bands", halo_rows(True, True))
    errors, worst, moved = [], [], []
    previous = None
    for f, (emissive, denoise) in enumerate(plan):
        s = settings(emissive, denoise)
        fi = frame_inputs(f, cam, lights, W, H)
        passes(o, s, fi)
        for _, r in ranks:
            r.render_gbuffer(fi)
        if refill and (emissive, denoise) != previous:
            moved.append((f, refill_windows_local(ranks, s)))
        previous = (emissive, denoise)
        for _, r in ranks:
            r.render_frame(s, fi)
            r.denoise(s, fi)
            r.tone_sum(s)
        whole = canon_plane(10, o.output(10)).reshape(H, W, 4)
        for b, r in ranks:
            exact, rel = core_agreement(r, b, whole)
            worst.append((f, b.y0, round(exact, 4), round(rel, 5)))
            if (refill or f < 4) and exact < 1.0:
                errors.append(f"frame {f} band {b.y0}: {exact:.4f} of pixels exact")
            if not rel <= 0.01:  # (inf or NaN for a value that is not finite)
                errors.append(f"frame {f} band {b.y0}: {exact:.4f} of pixels exact, mean relative difference {rel:.4f}")
    assert not errors, "\n".join(errors) + f"\n{worst}"
    if refill:
        # the widening frames moved rows (both inner bands on both sides, the outer bands on one side)
        grown = dict(moved)
        assert grown[0] == 0 and grown[4] > 0 and grown[6] > 0 and grown[8] == 0 and grown[9] == 0, moved


@pytest.mark.parametrize("world,spatial,denoise", [(4, True, True), (8, True, True), (4, "indirect", True),
                                                   (8, False, False)])
def test_gpu_tiles_match_whole_frame(world, spatial, denoise):
    """2-D tile contexts (hk_resize_tile: 2x2 at world 4, 4x2 at world 8 on a 128 x 192 frame, halo 40) reproduce the
    whole-frame oracle render bit-exactly on their own rectangles over 5 frames, and their ray counters add up to the
    whole frame's (each pixel counted by the tile that owns it).  The tiles' rows + halo and columns + halo are strict
    parts of the frame, so every pass runs on a proper row and column window (pass_window)."""
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs, load_noise
    from hikari_amd.bands import halo_rows
    from oracle import Oracle
    W, H = 128, 192
    scene, cam, lights = examples.cornell()
    desc = scene.build()
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=bool(spatial),
                        emissive_spatial_reuse=spatial is True, denoise=denoise)
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, 1.0)
    ranks = decomposed(scene, world, W, H, "tiles", halo_rows(True, True))
    errors = []
    for f in range(5):
        fi = frame_inputs(f, cam, lights, W, H)
        passes(o, s, fi)
        whole = o.output(10)
        for t, r in ranks:
            passes(r, s, fi)
            row0, rows, core0, core_rows = r.band_info()
            assert row0 + core0 == t.y0 and core_rows == t.rows
            mine = np.ascontiguousarray(r.output(10)[core0: core0 + core_rows, t.x0: t.x0 + t.cols])
            ref = np.ascontiguousarray(whole[t.y0: t.y0 + t.rows, t.x0: t.x0 + t.cols])
            if not np.array_equal(canon_plane(10, mine), canon_plane(10, ref)):
                errors.append(f"frame {f} tile {t}")
    assert not errors, "\n".join(errors)
    assert summed_counters(ranks) == o.counters()


def test_gpu_tile_rect_copy():
    """hk_copy_output_rect: a tile's core rectangle of the tone-mapped plane copied packed and into a pitched
    whole-frame buffer equals those pixels of hk_get_output."""
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs
    W, H = 128, 96
    scene, cam, lights = examples.cornell()
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0).to_c()
    r = renderer(scene)
    r.set_band_halo(16)
    r.resize_tile(W, H, 64, 64, 48, 48)
    fi = frame_inputs(0, cam, lights, W, H)
    r.render_gbuffer(fi)
    r.render_frame(st, fi)
    r.tone_sum(st)
    full = r.output(10)
    row0, rows, core0, core_rows = r.band_info()
    packed = np.zeros((core_rows, 64, 8), np.uint8)
    r.copy_output_rect(10, core0, core_rows, 64, 64, packed.ctypes.data, 0, True)
    assert np.array_equal(packed, full[core0: core0 + core_rows, 64:128])
    frame = np.zeros((H, W, 8), np.uint8)
    dst = frame[48:96, 64:128]
    r.copy_output_rect(10, core0, core_rows, 64, 64, dst.ctypes.data, W * 8, True)
    assert np.array_equal(frame[48:96, 64:128], full[core0: core0 + core_rows, 64:128])
    assert not frame[:48].any() and not frame[:, :64].any()


def test_gpu_row_bands_moving_camera_within_tolerance():
    """Band contexts under camera motion (the examples' orbit, examples.orbit at 2 deg/frame): every pass
    then runs on the whole band (pass_window keeps row windows for static frames only), and temporal
    reprojection reads previous reservoirs that the band computed itself.  The reference's own scatter
    race (light.wgsl:1092-1095) and rows reprojected from beyond a band's halo make this inexact by
    nature, so the tone-mapped core rows must match the whole-frame oracle on >= 95 % of
    pixels with a mean relative difference <= 2 %, over 5 frames with spatial reuse and the denoiser."""
    import math
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs, load_noise
    from hikari_amd.bands import halo_rows
    from oracle import Oracle
    W, H, world = 64, 192, 3
    scene, cam, lights = examples.cornell()
    desc = scene.build()
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=True, denoise=True)
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, 1.0, threads=1)
    ranks = decomposed(scene, world, W, H, "bands", halo_rows(True, True))
    target = examples.ORBIT_TARGETS["cornell"]
    yaw = math.radians(2.0)
    errors = []
    for f in range(5):
        fi = frame_inputs(f, examples.orbit(cam, target, f, yaw), lights, W, H,
                          previous_camera=examples.orbit(cam, target, f - 1, yaw) if f else None)
        for x in [o] + [r for _, r in ranks]:
            passes(x, s, fi)
        whole = canon_plane(10, o.output(10)).reshape(H, W, 4)
        for b, r in ranks:
            exact, rel = core_agreement(r, b, whole)
            if exact < 0.95 or rel > 0.02:
                errors.append(f"frame {f} band {b.y0}: {exact:.4f} of pixels exact, mean relative difference {rel:.4f}")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("world", [2, 3])
def test_gpu_interleaved_stripes_match_whole_frame(world):
    """Interleaved 8-row stripe contexts (bench.py's decomposition for frames without neighbour
    reads, run on one GPU) reassemble the whole-frame oracle render bit-exactly, count exactly
    the whole frame's rays, and refuse the passes that read neighbours."""
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs, load_noise
    from hikari_amd._abi import HikariError
    from hikari_amd.bands import stripe_gather_rows
    from oracle import Oracle
    W, H = 64, 100  # 13 stripes, the last one 4 rows
    scene, cam, lights = examples.cornell()
    desc = scene.build()
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False, denoise=False)
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, 1.0)
    ranks = decomposed(scene, world, W, H, "stripes")
    for f in range(5):
        fi = frame_inputs(f, cam, lights, W, H)
        o.render_gbuffer(fi)
        o.render_frame(s, fi)
        o.tone_sum(s)
        for _, r in ranks:
            passes(r, s, fi)  # denoise off: a no-op, allowed
    pad, index = stripe_gather_rows(world, H)
    gathered = np.zeros((world * pad, W, 8), np.uint8)
    for k, r in ranks:
        row0, rows, core0, core_rows = r.band_info()
        assert row0 == 0 and core0 == 0 and rows == core_rows
        gathered[k * pad: k * pad + rows] = r.output(10)
    assert np.array_equal(canon_plane(10, gathered[index]), canon_plane(10, o.output(10)))
    assert summed_counters(ranks) == o.counters()
    spatial = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=True, denoise=True).to_c()
    with pytest.raises(HikariError):
        ranks[0][1].render_frame(spatial, frame_inputs(5, cam, lights, W, H))
    with pytest.raises(HikariError):
        ranks[0][1].denoise(spatial, frame_inputs(5, cam, lights, W, H))


@pytest.mark.parametrize("variant", ["default_ratio1", "emissive_spatial_multibounce", "no_temporal_no_spatial",
                                     "no_indirect", "validate_every_frame"])
def test_gpu_matches_golden_digests(variant):
    """GPU renders of the committed golden variants (tests/golden/) reproduce every digest."""
    import json
    from pathlib import Path

    import make_golden_path  # noqa: F401
    from make_golden import FRAMES, H, W, render
    gold = json.loads((Path(__file__).parent / "golden" / "cornell_golden.json").read_text())
    frames, _ = render(lambda scene, desc: renderer(scene, (W, H)), variant)
    for f, (a, b) in enumerate(zip(frames, gold["variants"][variant]["digests"])):
        bad = [k for k in b if a[k] != b[k]]
        assert not bad, f"{variant} frame {f}: {bad}"


@pytest.mark.parametrize("ratio_setting", ["SMAA_TU_1_0", "SMAA_TU_2_0"])
def test_textured_materials_bit_exact(ratio_setting):
    """Textured pipeline (light.wgsl:748-794): sRGB / linear textures, all address modes and
    filters, on base colour, emissive, metallic-roughness and occlusion slots."""
    from hikari_amd import HikariSettings, Upscale
    run_static("cornell_textured", 64, 48, HikariSettings(upscale=getattr(Upscale, ratio_setting),
                                                          emissive_spatial_reuse=True, indirect_bounces=2), 5)


def test_upscale_ratio_two_half_resolution_integrator():
    """SMAA_TU_2_0 (the default): integrator at s = ceil(S/2), jittered deferred lookups."""
    from hikari_amd import HikariSettings, Upscale
    run_static("cornell", 64, 48, HikariSettings(upscale=Upscale.SMAA_TU_2_0), 5)


@pytest.mark.parametrize("scene_fn,size", [("scene", (64, 40)), ("city", (48, 32))])
def test_proxy_scenes_with_directional_light(scene_fn, size):
    """City-proxy scenes: 140K-triangle BLASes, a directional light (cone sampling, any-hit
    shadow rays) and an emissive sphere."""
    from hikari_amd import HikariSettings, Upscale
    run_static(scene_fn, size[0], size[1], HikariSettings(upscale=Upscale.SMAA_TU_1_0), 4)


def test_hardware_f16_conversion_matches_software_rne():
    """The kernels convert to f16 with v_cvt_f16_f32; the oracle restates IEEE round-to-nearest-
    even in software (hk_f32_to_f16). Check them equal on every f32 bit pattern of a 2^24 stride
    sweep plus 2^22 patterns near f16 boundaries (halfway cases, subnormals, overflow, inf/NaN)."""
    from hikari_amd import HikariRenderer
    import oracle as orc
    r = HikariRenderer(0)
    L = orc.lib()
    hi = np.arange(1 << 19, dtype=np.uint32) << 13  # every sign/exponent/upper-mantissa combination
    bits = np.concatenate([np.arange(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32)]
                          + [hi | np.uint32(k) for k in (0x0FFF, 0x1000, 0x1001, 0x0001, 0x1FFF)]
                          # dense over f16-subnormal / overflow results (f32 exponents 102..113, 142..143)
                          + [np.arange(0x33000000, 0x38800000, 7, dtype=np.uint32),
                             np.arange(0x477FE000, 0x47800000 + 64, dtype=np.uint32)])
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    vals = bits.view(np.float32)
    got = r.selftest_f16(vals)
    want = np.empty(len(vals), np.uint16)
    L.hko_f32_to_f16_array(vals.ctypes.data, len(vals), want.ctypes.data)
    nan = np.isnan(vals)
    assert np.array_equal(got[~nan], want[~nan]), int((got[~nan] != want[~nan]).sum())
    # NaN stays NaN (quiet; payloads are canonicalised everywhere they are compared)
    g = got[nan]
    assert ((g & 0x7C00) == 0x7C00).all() and ((g & 0x03FF) != 0).all()


@pytest.mark.parametrize("scene_fn,size", [("scene", (480, 270)), ("city", (480, 270)), ("cornell", (256, 256))])
def test_gbuffer_ordered_traversal_matches_oracle(scene_fn, size):
    """The primary-ray G-buffer (ordered closest-hit traversal over the wide BVH layout) against
    the oracle's restatement of the same rule, on every G-buffer plane."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    w, h = size
    scene, cam, lights, r, o = pair(scene_fn, w, h, HikariSettings(upscale=Upscale.SMAA_TU_1_0))
    fi = frame_inputs(0, cam, lights, w, h)
    r.render_gbuffer(fi)
    o.render_gbuffer(fi)
    errors = []
    compare_frame(r, o, 0, errors, outputs=range(11, 16), rids=())
    assert not errors, "\n".join(errors)
    assert r.counters()["primary"] == o.counters()["primary"] == w * h


def test_subframe_accumulation_matches_numpy():
    """hk_accumulate / hk_resolve_accumulation (config 5): f32 running sum of the tone-mapped
    RGBA16F sub-frames, divided by the count and rounded to f16 (numpy restatement, bit-exact)."""
    from hikari_amd import HikariSettings, Upscale, _abi, frame_inputs
    w, h = 48, 32
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0)
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    s = st.to_c()
    acc = np.zeros((h, w, 4), np.float32)
    for f in range(5):
        passes(r, s, frame_inputs(f, cam, lights, w, h))
        r.accumulate(reset=(f == 0))
        t = r.output(_abi.OUT_TONE_MAPPED).view(np.float16).reshape(h, w, 4).astype(np.float32)
        acc = (acc + t).astype(np.float32)
    r.resolve_accumulation()
    got = r.output(_abi.OUT_ACCUMULATED).view(np.uint16).reshape(h, w, 4)
    want = (acc / np.float32(5.0)).astype(np.float32).astype(np.float16).view(np.uint16)
    assert np.array_equal(got, want)


def test_fast_division_by_frame_size_is_exact():
    """div_by (hk_device.h), the kernels' division by an image dimension, returns the IEEE
    quotient's bits for every x with |x| in [2^-100, 2^100) (both signs), for every divisor
    1..4352 (all widths/heights up to 4K plus margin) and the 8K sizes."""
    from hikari_amd import HikariRenderer
    r = HikariRenderer(0)
    lo, hi = 0x0D800000, 0x71800000
    bad = {d: r.selftest_div(float(d), lo, hi) for d in list(range(1, 4353)) + [7680, 4320, 8192]}
    assert not any(bad.values()), {d: n for d, n in bad.items() if n}


def test_fast_reciprocal_is_exact():
    """rcp_exact (hk_device.h) returns the IEEE quotient 1 / x bit for bit for every f32 x
    (all 2^32 patterns: zeros, denormals, infinities and NaNs included)."""
    from hikari_amd import HikariRenderer
    r = HikariRenderer(0)
    assert r.selftest_rcp(0, 0x80000000) == 0


@pytest.mark.parametrize("scene_fn", ["cornell", "city"])
def test_gpu_instance_update_matches_host_rebuild(scene_fn):
    """hk_update_instances (GPU re-run of prepare_instances: instance records, TLAS build,
    emissive records + alias tables, light BVH) equals the host builder's buffers for the same
    transforms, and the next frame renders bit-exactly like the oracle on the host-built scene."""
    from hikari_amd import HikariSettings, Upscale, examples, frame_inputs, load_noise
    from oracle import Oracle
    scene0, cam, lights = examples.SCENES[scene_fn]()
    d0 = scene0.build()
    r = renderer(scene0)
    scene1, _, _ = moved(examples.SCENES[scene_fn](), 7)
    d1 = scene1.build()
    r.update_instances(scene1.instance_models(), scene1.instance_local_aabbs())
    assert_instance_update_matches_host(r, d1)
    # and the frame
    w, hgt = 48, 32
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False)
    r.resize(w, hgt, 1.0)
    # the oracle sees the same history: the uploaded scene, then the moved one (the first frame's
    # motion vectors reproject from the uploaded models, GlobalTransformQueue); single-threaded and
    # with spatial reuse off, as the reprojection scatter into the spatial pair is a write race
    # (test_gpu_motion.py)
    o = Oracle(d0, load_noise(), w, hgt, 1.0, threads=1)
    o.set_scene(d1)
    s = st.to_c()
    errors = []
    for f in range(2):
        fi = frame_inputs(f, cam, lights, w, hgt)
        for x in (r, o):
            passes(x, s, fi)
        compare_frame(r, o, f, errors, racy=RACY)
    assert not errors, "\n".join(errors[:10])


@pytest.mark.parametrize("ratio_setting,taa,pipelined", [("SMAA_TU_2_0", "Jasmine", False), ("SMAA_TU_1_0", "Jasmine", False),
                                                         ("SMAA_TU_2_0", "None_", False), ("SMAA_TU_1_0", "Jasmine", True)])
def test_post_process_smaa_taa_bit_exact(ratio_setting, taa, pipelined, hk_options):
    """SMAA TU4x + TAA Jasmine (hk_post_process) on the GPU vs the oracle, bit for bit, over
    frames with both jitter parities (the reference default pipeline is SMAA_TU_2_0 + Jasmine).
    `pipelined`: frame pipelining forced on (the post-process reads the previous G-buffer slot,
    which the next frame's G-buffer overwrites)."""
    from hikari_amd import HikariSettings, Taa, Upscale, _abi, frame_inputs
    if pipelined:
        hk_options["pipeline_min_px"] = 0
    w, h = 62, 41
    st = HikariSettings(upscale=getattr(Upscale, ratio_setting), taa=getattr(Taa, taa))
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    outs = [_abi.OUT_TONE_MAPPED, _abi.OUT_UPSCALED] + ([_abi.OUT_TAA] if taa == "Jasmine" else [])
    run_frames(r, o, st.to_c(), (frame_inputs(f, cam, lights, w, h) for f in range(4)), post=True, counters=False,
               outputs=outs, rids=())


@pytest.mark.parametrize("mode", ["no_view", "no_temporal_reuse"])
def test_spatial_reuse_without_view_planes_bit_exact(hk_options, mode):
    """Spatial reuse gathering the neighbours' own reservoir planes instead of the spatial view planes
    (hk_device.h store_res_view): forced with spatial_view_planes=0, and taken by the runtime when the temporal
    pass does not store its records (temporal_reuse = false: the records in `cur` are older than any view
    plane).  Every plane and reservoir bit-exact against the oracle over 6 frames."""
    from hikari_amd import HikariSettings, Upscale
    if mode == "no_view":
        hk_options["spatial_view_planes"] = 0
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, temporal_reuse=mode != "no_temporal_reuse")
    run_static("cornell", 64, 64, st, 6, counters=False)
