"""GPU parity for the tone pass over the kept rectangle (option bg_tile_skip): hk_tone_sum launches its kernel over the
pixels that can hold anything but the clear colour's texel.  Frames of 96x64 to 176x112 with the camera pulled back, so that the scene's
bound covers a few tiles in the middle; every frame's tone plane and its previous slot, every other output plane, every
reservoir buffer and the counters bit for bit against the CPU oracle, and hk_tone_skip_info / hk_tile_skip_info showing
where the skip was on (with the rectangle the test works out from the bound itself) and where it had to be off, so that
no case passes by never skipping."""
import numpy as np
import pytest

from parity import canon_plane, compare_frame, decomposed, pair, passes
from tile_skip_cases import pan_camera

pytestmark = pytest.mark.gpu

RUN = 2  # the tone kernel's pixel run (TONE_RUN): the launched columns are outward to it
# the default 1080p frame's schedule (pipelined: two render slots, the tone-sum on the tail stream) and the small
# frame's own default (one render slot, k_light_merged); k_gbuffer launched every frame, as in the benchmark
PIPELINED = {"gbuffer_reuse": 0, "pipeline_min_px": 0, "fuse_min_px": 0, "merge": 0}
SMALL = {"gbuffer_reuse": 0}


def _settings(**kw):
    from hikari_amd import HikariSettings, Upscale
    kw.setdefault("indirect_spatial_reuse", False)
    kw.setdefault("denoise", False)
    kw.setdefault("upscale", Upscale.SMAA_TU_1_0)
    return HikariSettings(**kw)


def _far(cam, dx=0.0, back=2.0):
    """The scene's camera `back` times as far away and moved sideways by dx with its target: the bound is a few tiles
    in the middle of the frame, left or right of it."""
    from hikari_amd import Camera, Transform
    t = np.asarray(cam.transform.translation, np.float64)
    return Camera(Transform.from_xyz(t[0] + dx, t[1], t[2] * back).looking_at((dx, 1.0, 0.0)))


def _frame(r, o, st, fi, f):
    """One frame on both, compared; returns (hk_tone_skip_info, hk_tile_skip_info) of the renderer."""
    errors = []
    s = st.to_c()
    for x in (r, o):
        passes(x, s, fi)
    compare_frame(r, o, f, errors)
    assert not errors, "\n".join(errors[:20])
    return r.tone_skip_info(), r.tile_skip_info()


def _aligned(rect, window):
    """`rect` = (x0, y0, x1, y1) within `window`, columns outward to RUN; None when empty."""
    x0, y0, x1, y1 = max(rect[0], window[0]), max(rect[1], window[1]), min(rect[2], window[2]), min(rect[3], window[3])
    if x1 <= x0 or y1 <= y0:
        return None
    return (x0 // RUN * RUN, y0, -(-x1 // RUN) * RUN, y1)


def _join(a, b):
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))


def _expect(tone, rect, window):
    """The tone launch ran over `rect` (aligned, within the window) and left the window's other pixels out."""
    want = _aligned(rect, window) if rect else None
    area = (want[2] - want[0]) * (want[3] - want[1]) if want else 0
    px = (window[2] - window[0]) * (window[3] - window[1])
    assert tone == {"skipped": px - area, "rect": want}, (tone, want, window)
    return px - area


def _full(tone, w, h):
    assert tone == {"skipped": 0, "rect": (0, 0, w, h)}, tone


@pytest.mark.parametrize("size", [(96, 64), (176, 112)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("path", ["pipelined", "small"])
def test_still_camera(hk_options, path, size):
    """Case 1.  Frames 0 and 1 write each tone slot whole; from frame 2 the launch is the bound's rectangle."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED if path == "pipelined" else SMALL)
    w, h = size
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cam = _far(cam)
    for f in range(6):
        tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
        if f < 2:
            _full(tone, w, h)
        else:
            assert tiles["bound"] is not None and tiles["gbuffer"] > 0
            assert _expect(tone, tiles["bound"], (0, 0, w, h)) > w * h // 2, (f, tone)
    assert r.counters() == o.counters()


def test_camera_jump(hk_options):
    """Case 2.  The bound moves off tiles it covered: the first launch on each slot after the jump runs over the join
    of the old and the new bound (the old one's texels get the clear colour again), the next over the new bound."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED)
    w, h = 176, 112
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cams = [_far(cam, 1.5)] * 4 + [_far(cam, -1.5)] * 4  # the scene left of the middle, then right of it
    bounds = []
    for f, c in enumerate(cams):
        tone, tiles = _frame(r, o, st, frame_inputs(f, c, lights, w, h), f)
        bounds.append(tiles["bound"])
        if f in (2, 3, 6, 7):
            _expect(tone, bounds[f], (0, 0, w, h))
        elif f in (4, 5):
            assert bounds[f][0] >= bounds[3][2], "the jump must leave the old bound"
            _expect(tone, _join(bounds[3], bounds[f]), (0, 0, w, h))
    # the old bound's pixels are background again
    x0, y0, x1, y1 = bounds[3]
    plane = canon_plane(10, r.output(10)).reshape(h, w, 4)
    assert (plane[y0:y1, x0:x1] == plane[0, 0]).all()
    assert r.counters() == o.counters()


def test_clear_colour_change(hk_options):
    """Case 3.  Another clear colour: the next launch on each slot is whole, then the skip resumes."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED)
    w, h = 128, 80
    scene, cam, lights, r, o = pair("cornell", w, h, _settings())
    cam = _far(cam)
    for f in range(8):
        st = _settings(clear_color=(0.4, 0.4, 0.4, 1.0) if f < 4 else (0.1, 0.6, 0.2, 0.5))
        tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
        if f in (0, 1, 4, 5):
            _full(tone, w, h)
        else:
            _expect(tone, tiles["bound"], (0, 0, w, h))


def test_indirect_bounces_off_and_on(hk_options):
    """Case 4.  indirect_bounces 1 -> 0 -> 1: without bounces the pass reads the direct and emissive planes alone (and
    the frame is not pipelined); exact on every frame, and each stage ends skipping."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED)
    w, h = 128, 80
    scene, cam, lights, r, o = pair("cornell", w, h, _settings())
    cam = _far(cam)
    f = 0
    for bounces in (1, 0, 1):
        st = _settings(indirect_bounces=bounces)
        for _ in range(4):
            tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
            f += 1
        _expect(tone, tiles["bound"], (0, 0, w, h))
    assert r.counters() == o.counters()


def test_denoiser_switched_on(hk_options):
    """Case 5.  From the frame the denoiser is on, the pass reads the denoised planes, for which no constant
    background texel is shown: no skip from then on (the launch is whole), and the plane is exact."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED)
    w, h = 128, 80
    scene, cam, lights, r, o = pair("cornell", w, h, _settings())
    cam = _far(cam)
    for f in range(6):
        tone, tiles = _frame(r, o, _settings(denoise=f >= 3), frame_inputs(f, cam, lights, w, h), f)
        if f == 2:
            _expect(tone, tiles["bound"], (0, 0, w, h))
        else:
            _full(tone, w, h)


@pytest.mark.parametrize("w", [161, 160])
def test_odd_and_even_width(hk_options, w):
    """Case 6.  Width 161 takes the per-texel kernel, which keeps the whole launch; 160 skips, its bound's odd right
    edge outward to the run."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED)
    h = 96
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cam = _far(cam)
    for f in range(4):
        tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
        if w % 2 or f < 2:
            _full(tone, w, h)
        else:
            assert tiles["bound"][2] % 2 == 1
            _expect(tone, tiles["bound"], (0, 0, w, h))
    assert r.counters() == o.counters()


def test_camera_sees_nothing(hk_options):
    """Case 7.  The scene is off screen: once both slots hold the clear colour nothing is launched, the plane is all
    clear colour, every workgroup of the frame kernels is skipped and the primary rays are still counted."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED)
    w, h = 96, 64
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cam = pan_camera(cam, 40.0)
    tiles_all = ((w + 15) // 16) * ((h + 15) // 16)
    for f in range(5):
        tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
        assert tiles["bound"] == (0, 0, 0, 0)
        if f >= 2:
            assert tone == {"skipped": w * h, "rect": None}, tone
            assert all(tiles[k] == tiles_all for k in ("gbuffer", "direct", "indirect")), tiles
    plane = canon_plane(10, r.output(10)).reshape(-1, 4)
    assert (plane == plane[0]).all()
    assert r.counters() == o.counters() and r.counters()["primary"] == 5 * w * h


def test_camera_inside_the_box(hk_options):
    """Case 8.  No bound: nothing is skipped."""
    from hikari_amd import Camera, Transform, frame_inputs
    hk_options.update(PIPELINED)
    w, h = 96, 64
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cam = Camera(Transform.from_xyz(0.0, 1.0, 0.5).looking_at((0.0, 1.0, -1.0)))
    for f in range(4):
        tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
        assert tiles["bound"] is None
        _full(tone, w, h)


@pytest.mark.parametrize("option", ["bg_tile_skip", "bg_elision"])
def test_options_off(hk_options, option):
    """Case 9.  Either option off: the whole launch on every frame, the same planes; back on, the skip resumes."""
    from hikari_amd import frame_inputs
    hk_options.update(PIPELINED)
    hk_options[option] = 0
    w, h = 128, 80
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cam = _far(cam)
    for f in range(8):
        if f == 4:
            r.set_option(option, 1)
        tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
        if f < 6:
            _full(tone, w, h)
            assert f >= 4 or tiles["gbuffer"] == tiles["direct"] == tiles["indirect"] == 0
        else:
            _expect(tone, tiles["bound"], (0, 0, w, h))


def test_resize_in_mid_run(hk_options):
    """Case 10.  hk_resize drops the slots' histories with the buffers: two whole launches, then the skip again."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    hk_options.update(PIPELINED)
    w, h = 128, 80
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cam = _far(cam)
    for stage in range(2):
        for f in range(3):
            tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
            if f < 2:
                _full(tone, w, h)
            else:
                _expect(tone, tiles["bound"], (0, 0, w, h))
        if stage == 0:
            r.resize(w, h, 1.0)
            o = Oracle(scene.desc, load_noise(), w, h, 1.0)


@pytest.mark.parametrize("kind", ["bands", "tiles"])
def test_band_and_tile_contexts(hk_options, kind):
    """Case 11.  Two row bands (hk_resize with y0, rows) and a left and a right half (hk_resize_tile): each part's own
    pixels are the whole-frame oracle's, and each part launches the bound's rectangle within its own rows and columns
    (nothing where the bound misses the part: the lower band)."""
    from types import SimpleNamespace

    from hikari_amd import Camera, Transform, examples, frame_inputs, load_noise
    from oracle import Oracle
    from parity import renderer
    hk_options["gbuffer_reuse"] = 0
    W, H = 160, 96
    scene, cam, lights = examples.cornell()
    desc = scene.build()
    if kind == "bands":  # the bound inside the upper band's rows
        cam = Camera(Transform.from_xyz(0.0, -2.2, 12.0).looking_at((0.0, -2.2, 0.0)))
        ranks = decomposed(scene, 2, W, H, kind, halo=0)
    else:  # the bound across both halves
        cam = _far(cam)
        ranks = []
        for x0 in (0, W // 2):
            r = renderer(scene)
            r.set_band_halo(0)
            r.resize_tile(W, H, x0, W // 2, 0, H)
            ranks.append((SimpleNamespace(x0=x0, cols=W // 2, y0=0, rows=H), r))
    st = _settings()
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, 1.0)
    launched = []
    for f in range(5):
        fi = frame_inputs(f, cam, lights, W, H)
        for x in [o] + [r for _, r in ranks]:
            passes(x, s, fi)
        whole = canon_plane(10, o.output(10)).reshape(H, W, 4)
        for k, (rect, r) in enumerate(ranks):
            row0, rows, core0, core_rows = r.band_info()
            mine = canon_plane(10, r.output(10)).reshape(rows, W, 4)[core0: core0 + core_rows]
            x0, x1 = (rect.x0, rect.x0 + rect.cols) if kind == "tiles" else (0, W)
            assert np.array_equal(mine[:, x0:x1], whole[rect.y0: rect.y0 + rect.rows, x0:x1]), (f, k)
            tone, tiles = r.tone_skip_info(), r.tile_skip_info()
            window = (x0, rect.y0, x1, rect.y0 + rect.rows)
            if f < 2:
                assert tone == {"skipped": 0, "rect": window}, (f, k, tone)
            else:
                _expect(tone, tiles["bound"], window)
                if f == 4:
                    launched.append(tone["rect"])
    if kind == "bands":
        assert launched[0] is not None and launched[1] is None, launched
    else:
        assert None not in launched, launched


def _kept_tiles(bound, w, h):
    x0, y0, x1, y1 = bound
    return ((x1 + 15) // 16 - x0 // 16) * ((y1 + 15) // 16 - y0 // 16)


@pytest.mark.parametrize("case", ["merged", "spatial"])
def test_kept_grid_launches(hk_options, case):
    """Case 12.  The kept tiles of k_light_merged (per role) and next to spatial reuse (those channels' launches still
    store their background pixels' spatial pair, so they keep every tile): skipped[] is what the test works out from
    the bound, and the tone pass skips in both.  (A grid of the kept tiles alone was measured and not kept; these
    numbers are the same for either.)"""
    from hikari_amd import frame_inputs
    hk_options.update({"gbuffer_reuse": 0, "merge": 1} if case == "merged" else PIPELINED)
    w, h = 176, 112
    spatial = case == "spatial"
    st = _settings(indirect_spatial_reuse=spatial, emissive_spatial_reuse=spatial)
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    cam = _far(cam)
    tiles_all = ((w + 15) // 16) * ((h + 15) // 16)
    for f in range(5):
        tone, tiles = _frame(r, o, st, frame_inputs(f, cam, lights, w, h), f)
        want = tiles_all - _kept_tiles(tiles["bound"], w, h) if f >= 2 else 0
        assert want > 0 or f < 2
        assert tiles["gbuffer"] == want, (f, tiles)
        assert tiles["direct"] == tiles["indirect"] == (0 if spatial else want), (f, tiles)
        if f >= 2:
            _expect(tone, tiles["bound"], (0, 0, w, h))
    assert r.counters() == o.counters()
