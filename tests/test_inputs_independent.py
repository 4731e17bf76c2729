"""The oracle along the input axes of tests/test_gpu_inputs.py, pinned without a GPU (CPU).

The GPU tests show kernels == oracle at fractional upscale ratios, under orthographic views and with settings at
their edges; both were written by the same hands, so here the oracle itself is held against independent
statements of the same inputs:

* the pure-Python restatements of light.wgsl / denoise.wgsl (tests/direct_python.py, indirect_python.py,
  denoise_python.py) at ratio 1.5, where the integrator size s and the G-buffer size S differ: s carries the
  reservoir index, the pixel's uv and the previous-uv coordinates, S the jitter texel size, the deferred
  coordinates and the plane loads (out-of-frame ones return 0); light.wgsl:1007-1017, denoise.wgsl:37-41;
* the same restatements with calculate_view's orthographic branch (light.wgsl:714-727);
* every settings case of test_edge_settings_bit_exact changes the oracle's frames (none is vacuous);
* the orthographic primary rays against a ray set built in float64 from the camera's Transform and extents,
  not from its matrices.

Tolerance of the restatement tests: none (bit-exact), as tests/test_indirect_independent.py.
"""
import functools

import numpy as np
import pytest

import denoise_python as dnp
import direct_python as dp
import indirect_python as ip
import inputs_cases as ic
from parity import canon_plane, canon_reservoirs
from test_indirect_independent import _bits, _frame_dict, _gbuffer

U32_MAX = 0xFFFFFFFF


def _check_channel(o, ch, bufs, size, buffer_ids, tag):
    w, h = size
    got_r = o.output(4 + ch).view(np.uint16).reshape(h, w, 4)
    want_r = bufs["render"].astype(np.float16).view(np.uint16)
    bad = np.argwhere((got_r != want_r).any(-1))
    assert len(bad) == 0, (tag, "render", bad[:5].tolist())
    got_v = _bits(o.output(1 + ch).view(np.float32).reshape(h, w))
    bad = np.argwhere(got_v != _bits(bufs["variance"]))
    assert len(bad) == 0, (tag, "variance", bad[:5].tolist())
    for name, k in buffer_ids:
        got = o.reservoirs(k).view(np.uint32).reshape(-1, 16)[: w * h]
        bad = np.argwhere((got != bufs[name]).any(1)).ravel()
        assert len(bad) == 0, (tag, name, k, bad[:5].tolist(), got[bad[0]].tolist(), bufs[name][bad[0]].tolist())


def _multi_loop(S, ratio, frames, camera_of=None):
    """test_indirect_independent's "multi" variant (MULTIPLE_BOUNCES with 3 bounces, emissive and indirect spatial
    reuse, max_reservoir_lifetime 3, the denoiser) on cornell with a G-buffer of size S at `ratio`: per frame the
    restatements run on the oracle's G-buffer and on the reservoir buffers as they were before the frame, and every
    render, variance and reservoir word and every denoised texel must equal the oracle's.  Returns every deferred
    lookup the light-pass restatements made as (uv, coords)."""
    import oracle as orc
    from hikari_amd import HikariSettings, Taa, Upscale, examples, frame_inputs, load_noise
    from oracle import Oracle
    W, H = S
    scene, cam, lights = examples.cornell()
    if camera_of is not None:
        cam = camera_of(cam)
    desc = scene.build()
    L = orc.lib()
    sc = dp.Scene(scene.arrays(), L)
    noise = load_noise().reshape(16, 64, 64, 4)
    st = HikariSettings(upscale=Upscale.smaa_tu4x(ratio), taa=Taa.None_, indirect_spatial_reuse=True, denoise=True,
                        indirect_bounces=3, emissive_spatial_reuse=True, max_reservoir_lifetime=3.0)
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, ratio, threads=1)
    sh, sw = o.output(4).shape[:2]  # the integrator grid s = ceil((1 / ratio) S)
    n = sw * sh
    lookups = []
    counts = {"top": 0, "emitter": 0, "deferred_lookups": lookups}
    stats = {}
    for f in range(frames):
        before = [o.reservoirs(k).view(np.uint32).reshape(-1, 16)[:n].copy() for k in range(10)]
        fi = frame_inputs(f, cam, lights, W, H)
        o.render_gbuffer(fi)
        o.render_frame(s, fi)
        o.denoise(s, fi)
        gb = _gbuffer(o, W, H)
        fr = _frame_dict(f, s, fi, L)
        fr.update(size=(sw, sh), deferred_size=(W, H), ratio=np.float32(ratio))
        if fi.view.projection[15] == 1.0:
            fr["orthographic_view"] = tuple(np.float32(fi.view.view_proj[4 * k + 2]) for k in range(3))
        fm = ip.Frame(fr, gb, noise)
        fm.lookups = lookups
        current, previous = f % 2, 1 - f % 2
        pixels = [(x, y) for y in range(sh) for x in range(sw)]

        # direct + emissive temporal, then EMISSIVE_LIT spatial reuse over the pair they share
        pair = {"prev_spatial": before[current + 4].copy(), "spatial": before[previous + 4].copy()}
        for ch, emissive_lit in ((0, False), (1, True)):
            bufs = dict(pair, prev=before[current + 2 * ch], cur=before[previous + 2 * ch].copy(),
                        variance=np.zeros((sh, sw), np.float32), render=np.zeros((sh, sw, 4), np.float32))
            for x, y in pixels:
                dp.direct_lit(sc, fr, gb, noise, bufs, x, y, emissive_lit, counts)
            if ch == 0:
                _check_channel(o, 0, bufs, (sw, sh), (("cur", previous),), (f, "direct"))
        for x, y in pixels:
            ip.spatial_reuse(sc, fm, bufs, x, y, True)
        _check_channel(o, 1, bufs, (sw, sh), (("cur", previous + 2), ("prev_spatial", current + 4),
                                              ("spatial", previous + 4)), (f, "emissive"))

        bufs = {"prev": before[current + 6], "cur": before[previous + 6].copy(),
                "prev_spatial": before[current + 8].copy(), "spatial": before[previous + 8].copy(),
                "variance": np.zeros((sh, sw), np.float32), "render": np.zeros((sh, sw, 4), np.float32)}
        for x, y in pixels:
            ip.indirect_lit_ambient(sc, fm, bufs, x, y, counts)
        for x, y in pixels:
            ip.spatial_reuse(sc, fm, bufs, x, y, False)
        _check_channel(o, 2, bufs, (sw, sh), (("cur", previous + 6), ("prev_spatial", current + 8),
                                              ("spatial", previous + 8)), (f, "indirect"))

        albedo = o.output(0).view(np.float16).reshape(H, W, 4).astype(np.float32)
        pl = dnp.Planes(gb, albedo)
        for ch in range(3):
            render = o.output(4 + ch).view(np.float16).reshape(sh, sw, 4).astype(np.float32)
            variance = o.output(1 + ch).view(np.float32).reshape(sh, sw)
            out, _ = dnp.denoise_channel(L, pl, render, variance, ch >= 1, f, ratio=ratio, stats=stats)
            got = o.output(7 + ch).view(np.uint16).reshape(sh, sw, 4)
            bad = np.argwhere((got != out.astype(np.float16).view(np.uint16)).any(-1))
            assert len(bad) == 0, (f, "denoised", ch, bad[:5].tolist())
    assert counts["top"] > 0
    return (sw, sh), lookups


def test_restatements_at_fractional_ratio():
    """cornell, S = 24x20 at ratio 1.5 (s = 16x14), frames 0..3: direct_lit, EMISSIVE_LIT and indirect
    spatial_reuse, indirect_lit_ambient and the denoiser restated with s and S kept apart, bit-exact against the
    oracle.  The case says something ratio 1 does not only if the jitter moved a lookup: at least one deferred
    lookup fell outside the frame or on a texel other than floor(uv S)."""
    S = (24, 20)
    s, lookups = _multi_loop(S, 1.5, 4)
    assert s == (16, 14)
    F = np.float32
    outside = sum(not (0 <= c[0] < S[0] and 0 <= c[1] < S[1]) for _, c in lookups)
    moved = sum(c != (int(np.floor(uv[0] * F(S[0]))), int(np.floor(uv[1] * F(S[1])))) for uv, c in lookups)
    assert lookups and (outside > 0 or moved > 0), (len(lookups), outside, moved)


def test_restatements_orthographic_view():
    """The same loop at ratio 1 under the orthographic camera (cornell 24x20, frames 0..2): calculate_view's
    orthographic vector in direct_lit, indirect_lit_ambient and both spatial passes, bit-exact."""
    _multi_loop((24, 20), 1.0, 3, camera_of=lambda cam: ic.orthographic_camera("cornell", cam))


# ------------------------------------------------------------------ settings cases are not vacuous
@functools.lru_cache(maxsize=None)
def _edge_last_frame(scene_fn, case):
    from hikari_amd import examples, frame_inputs, load_noise
    from oracle import Oracle
    w, h = ic.EDGE_SIZE
    scene, cam, lights = examples.SCENES[scene_fn]()
    st = ic.edge_settings(case)
    s = st.to_c()
    o = Oracle(scene.build(), load_noise(), w, h, 1.0, threads=1, textures=scene.textures)
    for f in range(ic.EDGE_FRAMES):
        fi = frame_inputs(f, cam, lights, w, h)
        o.render_gbuffer(fi)
        o.render_frame(s, fi)
        o.denoise(s, fi)
        o.tone_sum(s)
    return ([canon_plane(k, o.output(k)) for k in range(17)], [canon_reservoirs(o.reservoirs(k)) for k in range(10)])


def _edge_differs(scene_fn, case):
    base, got = _edge_last_frame(scene_fn, None), _edge_last_frame(scene_fn, case)
    return any(not np.array_equal(a, b) for a, b in zip(base[0] + base[1], got[0] + got[1]))


@pytest.mark.parametrize("case", list(ic.EDGE_CASES))
def test_edge_settings_change_the_frames(case):
    """Every case of test_edge_settings_bit_exact changes at least one plane or reservoir buffer of the oracle's
    last frame against the base settings on at least one of its two scenes, so that GPU == oracle on it says
    something the base settings do not."""
    assert any(_edge_differs(scene_fn, case) for scene_fn in ic.EDGE_SCENES)


def test_reservoir_lifetime_zero_is_the_base():
    """Why max_reservoir_lifetime = 0.0 is not an edge case (inputs_cases.EDGE_CASES): reservoir_lifetime
    (light.wgsl:913-915) turns a limit <= 1 into F32_MAX, so it renders the base settings' frames word for
    word, where 2.0 (a case) does not."""
    ic.EDGE_CASES["_lifetime_0"] = dict(max_reservoir_lifetime=0.0)
    try:
        assert not any(_edge_differs(scene_fn, "_lifetime_0") for scene_fn in ic.EDGE_SCENES)
    finally:
        del ic.EDGE_CASES["_lifetime_0"]


# ------------------------------------------------------------------ orthographic primary rays
def _reprojection_error(view_proj, position, covered):
    """Largest distance (pixels, either axis) between a covered pixel's centre and where view_proj maps its
    stored position (float64 arithmetic on the float32 matrix and positions)."""
    h, w = covered.shape
    m = np.asarray(view_proj, np.float64).reshape(4, 4).T  # column-major -> row-major
    p = np.concatenate([position[..., :3].astype(np.float64), np.ones((h, w, 1))], -1)
    clip = p @ m.T
    u = (clip[..., 0] / clip[..., 3] + 1.0) * 0.5 * w
    v = (1.0 - (clip[..., 1] / clip[..., 3] + 1.0) * 0.5) * h
    ys, xs = np.mgrid[0:h, 0:w]
    err = np.maximum(np.abs(u - (xs + 0.5)), np.abs(v - (ys + 0.5)))
    return float(err[covered].max())


def _gbuffer_of(o, cam, lights, w, h):
    from hikari_amd import frame_inputs
    fi = frame_inputs(0, cam, lights, w, h)
    o.render_gbuffer(fi)
    position = o.output(11).view(np.float32).reshape(h, w, 4)
    instance = o.output(14).view(np.float32).reshape(h, w, 2)[..., 0]
    return fi, position, instance


def test_orthographic_primary_rays_match_independent_rays():
    """The G-buffer of the orthographic camera on cornell 64x48 against pixel-centre rays built in float64 from the
    camera's Transform and its extents (origin = translation + right x + up y - back near, direction = -back;
    cast to f32) and traced as closest-hit queries:
    (a) hit / miss and the instance id agree on >= 99 % of pixels (the rest: silhouette pixels where the two ray
        sets straddle an edge);
    (b) view_proj maps every covered pixel's stored position back to that pixel's centre, within 16x the same
        error of the example's perspective camera (existing behaviour; measured 5.01e-5 px there, and 2.25e-6 px
        for the orthographic camera).
    With primary rays that start at view.world_position whatever the projection (the rule before orthographic
    support) this fails: every ray heads for a point of the camera's own plane (near = 0), the G-buffer is
    empty, (a) 0.4792 of the pixels agree (the background ones) and (b) has no covered pixel to measure."""
    from hikari_amd import examples, load_noise
    from hikari_amd.scene import quat_to_mat3
    from oracle import Oracle
    w, h = 64, 48
    scene, cam, lights = examples.cornell()
    o = Oracle(scene.build(), load_noise(), w, h, 1.0)
    fi, position, _ = _gbuffer_of(o, cam, lights, w, h)
    reference = _reprojection_error(fi.view.view_proj, position, position[..., 3] > 0)
    assert 0 < reference < 1e-3  # a perspective hit lies on its pixel's ray up to float32 rounding

    oc = ic.orthographic_camera("cornell", cam)
    fi, position, instance = _gbuffer_of(o, oc, lights, w, h)
    covered = position[..., 3] > 0
    rot = quat_to_mat3(np.asarray(oc.transform.rotation, np.float64))
    right, up, back = rot[:, 0], rot[:, 1], rot[:, 2]
    half_h = 0.5 * oc.orthographic_height
    half_w = half_h * (w / h)
    ys, xs = np.mgrid[0:h, 0:w]
    px = ((xs + 0.5) / w * 2.0 - 1.0) * half_w
    py = (1.0 - (ys + 0.5) / h * 2.0) * half_h
    origin = np.asarray(oc.transform.translation, np.float64) + px[..., None] * right + py[..., None] * up \
        - back * oc.near
    rays = np.concatenate([origin, np.broadcast_to(-back, origin.shape)], -1).reshape(-1, 6).astype(np.float32)
    hits = o.trace(rays).reshape(h, w, 5)
    hit = hits[..., 3] != U32_MAX
    same = (hit == covered) & (~hit | (hits[..., 3] == np.floor(instance).astype(np.int64)))
    agree = float(same.mean())
    print(f"orthographic primary rays: covered {covered.mean():.4f}, independent rays hit {hit.mean():.4f}, agree {agree:.4f}")
    assert 0.25 < hit.mean() < 0.9  # the extents frame the box with background around it
    assert agree >= 0.99, agree
    error = _reprojection_error(fi.view.view_proj, position, covered)
    print(f"reprojection error {error:.3g} px (perspective camera {reference:.3g} px)")
    assert error <= 16.0 * reference, (error, reference)
