"""GPU parity for the background tile skip (option bg_tile_skip): workgroups of k_gbuffer and of the light passes whose
tile lies outside the scene's screen bound, and whose targets already hold a background pixel's constants, return at
their first instruction.  Frames a few tiles wide (cornell at 384x128 and 256x64: whole tile columns are skipped), every
plane, reservoir buffer and counter bit for bit against the CPU oracle on every frame, and hk_tile_skip_info showing
where the skip was off (no history yet, a pass whose background still stores, an unknown bound) and where it was on, so
that no case passes by never skipping."""
import copy

import numpy as np
import pytest

from parity import RACY, canon_plane, compare_frame, decomposed, orbit_camera, pair, passes, summed_counters
from tile_skip_cases import pan_camera

pytestmark = pytest.mark.gpu

SIZES = [(384, 128), (256, 64)]
# the kernels a frame takes at a test's size: the default 1080p frame's (pipelined, k_direct_fused_w4 next to k_indirect),
# the small frame's default (k_light_merged), and the separate direct launches (k_direct_lit_w4, k_direct)
# (gbuffer_reuse off, as in the benchmark's 1-spp frames: a still camera's k_gbuffer is launched every frame)
PATHS = {
    "default_frame": {"gbuffer_reuse": 0, "pipeline_min_px": 0, "fuse_min_px": 0, "merge": 0},
    "merged": {"gbuffer_reuse": 0},
    "separate": {"gbuffer_reuse": 0, "merge": 0, "fuse": 0, "direct_w4_min_px": 0},
    "separate_small": {"gbuffer_reuse": 0, "merge": 0, "fuse": 0},
}
KEYS = ("gbuffer", "direct", "indirect")


def _settings(**kw):
    from hikari_amd import HikariSettings, Upscale
    kw.setdefault("indirect_spatial_reuse", False)
    kw.setdefault("upscale", Upscale.SMAA_TU_1_0)
    return HikariSettings(**kw)


def _frame(r, o, s, fi, f, racy=(), gbuffer=True):
    """One frame on both, compared; returns the renderer's hk_tile_skip_info."""
    errors = []
    for x in (r, o):
        if gbuffer:
            passes(x, s, fi)
        else:
            x.render_frame(s, fi)
            x.denoise(s, fi)
            x.tone_sum(s)
    compare_frame(r, o, f, errors, racy=racy)
    assert not errors, "\n".join(errors[:20])
    return r.tile_skip_info()


def _all(info, keys=KEYS):
    return all(info[k] > 0 for k in keys)


def _none(info, keys=KEYS):
    return all(info[k] == 0 for k in keys)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("path", list(PATHS))
def test_still_camera(hk_options, path, size):
    """Frames 0 to 7: nothing is skipped until each mask's history holds (two frames: both G-buffer slots, both
    reservoir parities and render slots), then every launch skips, and the counters are the oracle's."""
    from hikari_amd import frame_inputs
    hk_options.update(PATHS[path])
    w, h = size
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    for f in range(8):
        info = _frame(r, o, st.to_c(), frame_inputs(f, cam, lights, w, h), f)
        assert (_none(info) if f < 2 else _all(info)), (f, info)
        if f >= 2:
            x0, y0, x1, y1 = info["bound"]
            kept = ((x1 + 15) // 16 - x0 // 16) * ((y1 + 15) // 16 - y0 // 16)
            assert all(info[k] == tiles - kept for k in KEYS), (f, info, tiles, kept)
    assert r.counters() == o.counters()


@pytest.mark.parametrize("motion", [True, False], ids=["orbit", "orbit_teleport"])
def test_orbiting_camera(hk_options, motion):
    """The bound moves every frame.  With the previous view given the frame has motion vectors: the direct pair's
    background still stores (no skip there), the G-buffer and the indirect pass skip; without it every reprojection
    is the identity and all three skip, each only outside every bound its mask's bits have seen."""
    from hikari_amd import frame_inputs
    hk_options.update(PATHS["default_frame"])
    w, h = 256, 64
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=1)
    prev = None
    for f in range(7):
        c = orbit_camera(cam, f)
        fi = frame_inputs(f, c, lights, w, h, previous_camera=prev if motion else None)
        prev = copy.deepcopy(c)
        info = _frame(r, o, st.to_c(), fi, f, racy=RACY if motion and f >= 1 else ())
        if f >= 3:
            assert _all(info, ("gbuffer", "indirect")), (f, info)
            assert (info["direct"] == 0) if motion else (info["direct"] > 0), (f, info)
    assert r.counters() == o.counters()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pan_off_screen_and_back(hk_options, size):
    """The view slides until the scene is off screen (then every tile is skipped) and back (then none wrongly)."""
    from hikari_amd import frame_inputs
    hk_options.update(PATHS["default_frame"])
    w, h = size
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    shifts = [0, 0, 0, 3, 40, 40, 40, 40, 3, 0, 0, 0]
    off = 0
    for f, dx in enumerate(shifts):
        info = _frame(r, o, st.to_c(), frame_inputs(f, pan_camera(cam, float(dx)), lights, w, h), f)
        if dx == 40:
            assert info["bound"] == (0, 0, 0, 0) and not (r.output(11).view(np.float32).reshape(-1, 4)[:, 3] > 0).any()
            if shifts[f - 2: f + 1] == [40, 40, 40]:
                assert all(info[k] == tiles for k in KEYS), (f, info)
                off += 1
        elif f >= 10:
            assert _all(info) and info["gbuffer"] < tiles, (f, info)
    assert off == 2
    assert r.counters() == o.counters()


@pytest.mark.parametrize("moving", [False, True], ids=["still", "orbit"])
def test_orthographic(hk_options, moving):
    from hikari_amd import Camera, frame_inputs
    hk_options.update(PATHS["default_frame"])
    w, h = 256, 64
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", w, h, st, threads=1)
    prev = None
    for f in range(6):
        c = Camera.orthographic((orbit_camera(cam, f) if moving else cam).transform, 2.6)
        fi = frame_inputs(f, c, lights, w, h, previous_camera=prev if moving else None)
        prev = copy.deepcopy(c)
        info = _frame(r, o, st.to_c(), fi, f, racy=RACY if moving and f >= 1 else ())
        if f >= 3:
            assert _all(info, ("gbuffer", "indirect")), (f, info)
    assert r.counters() == o.counters()


def test_ratio_with_taa_jitter(hk_options):
    """Ratio 1.5 under the TAA jitter: the light passes do not elide at a ratio other than 1, k_gbuffer skips on the
    deferred grid, and the bound holds the jittered rays."""
    from hikari_amd import Upscale, frame_inputs
    hk_options.update(PATHS["default_frame"])
    w, h = 384, 128
    st = _settings(upscale=Upscale.smaa_tu4x(1.5))
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    for f in range(6):
        info = _frame(r, o, st.to_c(), frame_inputs(f, cam, lights, w, h, jitter=1), f)
        assert info["direct"] == 0 and info["indirect"] == 0
        assert (info["gbuffer"] > 0) == (f >= 2), (f, info)
    assert r.counters() == o.counters()


def test_settings_and_options_during_a_run(hk_options):
    """Spatial reuse on and off, the denoiser on, bg_elision and bg_tile_skip off and on: exact on every frame, the
    getter showing where each launch stopped skipping and where it resumed."""
    from hikari_amd import frame_inputs
    hk_options.update(PATHS["default_frame"])
    w, h = 256, 64
    base = dict(denoise=False)
    plan = [  # (frames, settings, options, launches that must skip on the stage's last frame, ... that must not at all)
        (3, {}, {}, KEYS, ()),
        (2, {"indirect_spatial_reuse": True}, {}, ("gbuffer", "direct"), ("indirect",)),
        (2, {"emissive_spatial_reuse": True}, {}, ("gbuffer", "indirect"), ("direct",)),
        (3, {}, {}, KEYS, ()),
        (3, {"denoise": True}, {}, KEYS, ()),
        (2, {}, {"bg_elision": 0}, (), KEYS),
        (3, {}, {"bg_elision": 1}, KEYS, ()),
        (2, {}, {"bg_tile_skip": 0}, (), KEYS),
        (1, {}, {"bg_tile_skip": 1}, KEYS, ()),
    ]
    scene, cam, lights, r, o = pair("cornell", w, h, _settings(**base))
    f = 0
    for frames, kw, opts, on, off in plan:
        st = _settings(**{**base, **kw})
        for k, v in opts.items():
            r.set_option(k, v)
        for n in range(frames):
            info = _frame(r, o, st.to_c(), frame_inputs(f, cam, lights, w, h), f)
            assert _none(info, off), (f, kw, opts, info)
            f += 1
        assert _all(info, on), (f, kw, opts, info)
    assert r.counters() == o.counters()


def test_buffers_during_a_run(hk_options):
    """hk_resize, hk_load_reservoirs and host-supplied G-buffer planes in the middle of a run: each drops what it
    invalidates (everything; the light masks; the G-buffer's mask and the bound), and the skip resumes after two frames."""
    from hikari_amd import frame_inputs, load_noise
    from hikari_amd.plugin import RESERVOIR_DTYPE
    from oracle import Oracle
    hk_options.update(PATHS["default_frame"])
    w, h = 256, 64
    st = _settings(denoise=False)
    s = st.to_c()
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    f = 0

    def run(n, **kw):
        nonlocal f
        out = []
        for _ in range(n):
            out.append(_frame(r, o, s, frame_inputs(f, cam, lights, w, h), f, **kw))
            f += 1
        return out

    assert _all(run(3)[-1])
    # hk_resize: zero-filled buffers, the oracle anew, frame numbers from 0
    r.resize(w, h, 1.0)
    counted = r.counters()
    o = Oracle(scene.desc, load_noise(), w, h, 1.0)
    f = 0
    infos = run(3)
    assert _none(infos[0]) and _none(infos[1]) and _all(infos[2]), infos
    primary = r.counters()["primary"] - counted["primary"]
    assert primary == o.counters()["primary"] == 3 * w * h
    # hk_load_reservoirs over a spatial pair's buffers, the same records in both
    rng = np.random.default_rng(9)
    for rid in (4, 8):
        rec = np.frombuffer(rng.bytes(w * h * RESERVOIR_DTYPE.itemsize), RESERVOIR_DTYPE)
        r.load_reservoirs(rid, rec)
        o.load_reservoirs(rid, rec)
    infos = run(3)
    assert all(i["gbuffer"] > 0 for i in infos)
    assert _none(infos[0], ("direct", "indirect")) and _none(infos[1], ("direct", "indirect")) and _all(infos[2]), infos
    # host planes (the oracle's own G-buffer): no bound, nothing skipped; then k_gbuffer again
    for _ in range(2):
        fi = frame_inputs(f, cam, lights, w, h)
        o.render_gbuffer(fi)
        for plane, oid in enumerate((11, 12, 13, 14, 15)):
            r.set_gbuffer_plane(plane, o.output(oid))
        errors = []
        for x in (r, o):
            x.render_frame(s, fi)
            x.tone_sum(s)
        compare_frame(r, o, f, errors)
        assert not errors, "\n".join(errors[:20])
        info = r.tile_skip_info()
        assert _none(info) and info["bound"] is None, info
        f += 1
    infos = run(4)
    assert _none(infos[0]) and _all(infos[-1]), infos


def _cornell_plus(dx):
    """Cornell and the same scene with one more instance of the tall box's mesh, dx to the side: outside the box's bound."""
    from hikari_amd import examples
    scene, cam, lights = examples.cornell()
    more = copy.copy(scene)
    more._h, more.desc = None, None
    mesh, mat, m = scene.instances[1]  # the tall box
    t = np.eye(4)
    t[0, 3] = dx
    more.instances = list(scene.instances) + [(mesh, mat, t @ np.asarray(m, np.float64))]
    return scene, more, cam, lights


def test_scene_changes_during_a_run(hk_options):
    """hk_update_instances moving an instance outside the old bound, hk_set_instances spawning one there, and
    hk_update_meshes (after which the host no longer knows the box: no bound, nothing skipped)."""
    from hikari_amd import frame_inputs
    hk_options.update(PATHS["default_frame"])
    w, h = 384, 128
    st = _settings(denoise=False)
    s = st.to_c()
    scene, more, cam, lights = _cornell_plus(2.5)
    triple = (scene, cam, lights)
    _, _, _, r, o = pair(triple, w, h, st, threads=1)
    f = 0

    def run(n):
        nonlocal f
        out = []
        for _ in range(n):
            out.append(_frame(r, o, s, frame_inputs(f, cam, lights, w, h), f, racy=RACY))
            f += 1
        return out

    first = run(3)[-1]
    assert _all(first)
    # an instance moved out of the box, to where every launch skipped
    moved = copy.copy(scene)
    moved._h, moved.desc = None, None
    mesh, mat, m = scene.instances[1]
    t = np.eye(4)
    t[0, 3] = -2.5
    moved.instances = [scene.instances[0], (mesh, mat, t @ np.asarray(m, np.float64))] + list(scene.instances[2:])
    r.update_instances(moved.instance_models(), moved.instance_local_aabbs())
    o.set_scene(moved.build())
    infos = run(4)
    assert infos[0]["bound"][0] < first["bound"][0] and infos[0]["direct"] == 0, (first, infos[0])  # (a motion frame)
    assert _all(infos[-1]) and infos[-1]["gbuffer"] < first["gbuffer"]
    assert (r.output(11).view(np.float32).reshape(h, w, 4)[:, : first["bound"][0], 3] > 0).any()
    # back, then one spawned on the other side
    r.update_instances(scene.instance_models(), scene.instance_local_aabbs())
    o.set_scene(scene.build())
    assert _all(run(4)[-1])
    r.set_instances(more, previous=list(range(len(scene.instances))) + [None], local_aabbs=more.instance_local_aabbs())
    o.set_scene(more.build())
    infos = run(4)
    assert infos[0]["bound"][2] > first["bound"][2]
    assert _all(infos[-1])
    assert (r.output(11).view(np.float32).reshape(h, w, 4)[:, first["bound"][2]:, 3] > 0).any()
    # a deformed mesh: the box is unknown from here on
    deformed = copy.copy(more)
    deformed._h, deformed.desc = None, None
    deformed.meshes = list(more.meshes)
    dm = copy.copy(more.meshes[mesh])
    dm.positions = (np.asarray(dm.positions) * np.float32(1.1)).astype(np.float32)
    deformed.meshes[mesh] = dm
    r.update_meshes(deformed, [mesh], local_aabbs=deformed.instance_local_aabbs())
    o.set_scene(deformed.build())
    for info in run(3):
        assert _none(info) and info["bound"] is None, info
    assert r.counters() == o.counters()


@pytest.mark.parametrize("kind", ["bands", "stripes", "tiles"])
def test_decompositions(hk_options, kind):
    """Two row bands, two interleaved stripes and a 2x1 tile split in one process: each part's own pixels of the
    tone-mapped frame and the summed counters are the whole-frame oracle's.  Bands and tiles skip on their own launch
    grids; stripes' rows are not contiguous in the frame, so they keep every tile."""
    from hikari_amd import examples, frame_inputs, load_noise
    from oracle import Oracle
    hk_options["gbuffer_reuse"] = 0
    W, H = (256, 64) if kind == "tiles" else (192, 128)
    scene, cam, lights = examples.cornell()
    desc = scene.build()
    st = _settings(denoise=False)
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, 1.0)
    ranks = decomposed(scene, 2, W, H, kind, halo=0)
    for f in range(6):
        fi = frame_inputs(f, cam, lights, W, H)
        for x in [o] + [r for _, r in ranks]:
            passes(x, s, fi)
        whole = canon_plane(10, o.output(10)).reshape(H, W, 4)
        for rect, r in ranks:
            row0, rows, core0, core_rows = r.band_info()
            mine = canon_plane(10, r.output(10)).reshape(rows, W, 4)[core0: core0 + core_rows]
            if kind == "stripes":
                ys = np.array([y for y in range(H) if (y // 8) % 2 == rect])
                assert np.array_equal(mine[: len(ys)], whole[ys]), (f, rect)
            elif kind == "tiles":
                assert np.array_equal(mine[:, rect.x0: rect.x0 + rect.cols],
                                      whole[rect.y0: rect.y0 + rect.rows, rect.x0: rect.x0 + rect.cols]), (f, rect)
            else:
                assert np.array_equal(mine, whole[rect.y0: rect.y0 + rect.rows]), (f, rect)
            info = r.tile_skip_info()
            assert (_none(info) if f < 2 or kind == "stripes" else _all(info)), (f, rect, info)
    assert summed_counters(ranks) == o.counters()
