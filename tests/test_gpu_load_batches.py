"""GPU parity for the light kernels' batched loads: an indirect pixel's normal, instance / material, velocity / uv and
blue-noise texels behind one frame test and one index (load_texels_at), and the background-mask byte requested with
the position texel (bg_mask).  Only the place of a load and of its wait moved, so every case is bit for bit against the
CPU oracle on planes 0 to 16, all ten reservoir buffers and both ray counters, at the smallest shapes where a moved
load can go wrong: partial tiles, texels outside the frame, pixels that change between background and covered,
validation frames, a mask reset, and the stripe and row-band index maps.  The direct launches are covered on the same
cases: moving their mask byte and previous records was measured too and not kept.
"""
import copy

import numpy as np
import pytest

from parity import (RACY, canon_plane, canon_reservoirs, compare_frame, decomposed, mismatch_report, orbit_camera, pair,
                    passes, run_static, summed_counters)

pytestmark = pytest.mark.gpu


def _settings(ratio=1.0, **kw):
    from hikari_amd import HikariSettings, Upscale
    return HikariSettings(upscale=Upscale.smaa_tu4x(ratio), **kw)


# the kernels a frame takes, forced by options: name -> (hk_set_option values, wavefront, indirect bounces)
PATHS = {
    "defaults": ({}, False, 1),                # staged k_indirect, direct_lit and the emissive pass as two launches
    "fused": ({"fuse_min_px": 0}, False, 1),   # k_direct_fused_w4
    "merged": ({"merge": 1}, False, 1),        # k_light_merged: both roles
    "lds_off": ({"lds_scene": 0}, False, 1),   # the unstaged kernels (texels preloaded)
    "lds_all": ({"lds_scene": 2}, False, 1),
    "wavefront": ({}, True, 1),                # k_wf_gen / _trace / _shade
    "two_bounces": ({}, False, 2),             # the multi-bounce k_indirect
}


@pytest.mark.parametrize("size", [(63, 47), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("path", list(PATHS))
def test_partial_tiles_bit_exact(hk_options, path, size):
    """Cornell, frames 0-5, once per kernel path: an odd width and a partial last tile row (63 x 47) and whole tiles
    (64 x 64); frames 0 and 1 run before any mask bit is set, the later ones with the background stores elided."""
    options, wavefront, bounces = PATHS[path]
    hk_options.update(options)
    run_static("cornell", *size, _settings(indirect_bounces=bounces), 6, wavefront=wavefront)


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
@pytest.mark.parametrize("ratio", [1.5, 2.0])
def test_out_of_frame_texels_bit_exact(hk_options, ratio, fused):
    """63 x 47 at upscale ratios 1.5 and 2: the integrator plane is smaller than the G-buffer, and the jittered
    G-buffer coordinates of edge pixels fall outside the frame, where the batch's single frame test must give the
    zero texels each load_* helper gave."""
    if fused:
        hk_options["fuse_min_px"] = 0
    run_static("cornell", 63, 47, _settings(ratio), 4)


def test_background_and_covered_pixels_change_bit_exact(hk_options):
    """64 x 64 with the fused launch asked for: the camera orbits for six frames (pixels change between background and
    covered, mask bits clear and set, the reprojection is no identity so the separate launches run), then stands for
    three (the fused launch comes back).  Under motion the scatter into the previous spatial buffers is racy
    (parity.RACY, at RACY_MIN_EXACT); with spatial reuse off nothing reads those records."""
    from hikari_amd import frame_inputs
    hk_options["fuse_min_px"] = 0
    w = h = 64
    st = _settings(indirect_spatial_reuse=False)
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    inputs, prev = [], None
    for f in range(9):
        c = orbit_camera(cam, min(f, 5))
        inputs.append(frame_inputs(f, c, lights, w, h, previous_camera=prev))
        prev = copy.deepcopy(c)
    errors = []
    for f, fi in enumerate(inputs):
        for x in (r, o):
            passes(x, st.to_c(), fi)
        compare_frame(r, o, f, errors, racy=RACY if f >= 1 else ())
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()


@pytest.mark.parametrize("lds", [0, 1], ids=["lds_off", "lds_default"])
def test_validation_frames_fused_bit_exact(hk_options, lds):
    """The fused launch forced over frames 0-10: multiples of direct_validate_interval (3, 6, 9), of
    emissive_validate_interval (5, 10), of both (0) and of neither, so every k_direct_fused* instantiation runs."""
    hk_options["fuse_min_px"] = 0
    hk_options["lds_scene"] = lds
    st = _settings()
    assert (st.direct_validate_interval, st.emissive_validate_interval) == (3, 5)
    run_static("cornell", 64, 64, st, 11)


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_mask_reset_bit_exact(hk_options, fused):
    """Four static frames (elision on from the third), then garbage uploaded over the spatial pairs, which drops the
    masks, and three more frames at 64 x 64: every background record is stored again and everything the oracle
    writes stays bit-exact (the uploaded records of covered pixels are nobody's output with spatial reuse off)."""
    from hikari_amd import frame_inputs
    from hikari_amd.plugin import RESERVOIR_DTYPE
    if fused:
        hk_options["fuse_min_px"] = 0
    w = h = 64
    st = _settings(indirect_spatial_reuse=False)
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    s = st.to_c()
    errors = []
    for f in range(7):
        fi = frame_inputs(f, cam, lights, w, h)
        if f == 4:
            assert r.counters() == o.counters()
            rng = np.random.default_rng(8)
            for rid in RACY:
                r.load_reservoirs(rid, np.frombuffer(rng.bytes(w * h * RESERVOIR_DTYPE.itemsize), RESERVOIR_DTYPE))
        for x in (r, o):
            passes(x, s, fi)
        if f < 4:
            compare_frame(r, o, f, errors)
        else:
            compare_frame(r, o, f, errors, rids=[k for k in range(10) if k not in RACY])
            bg = r.output(11).view(np.float32).reshape(h * w, 4)[:, 3] < np.finfo(np.float32).eps
            assert bg.sum() > 0
            for rid in RACY:
                m = mismatch_report(canon_reservoirs(r.reservoirs(rid))[bg], canon_reservoirs(o.reservoirs(rid)[: w * h])[bg],
                                    f"frame {f} reservoir {rid} background records")
                if m:
                    errors.append(m)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()


def _compare_rows(errors, f, label, got_planes, got_res, o, rows):
    """Rows `rows` of the oracle's frame against a part's planes 0-16 and ten reservoir buffers, (len(rows), W, ..)."""
    for oid in range(17):
        want = canon_plane(oid, np.ascontiguousarray(o.output(oid)[rows]))
        m = mismatch_report(canon_plane(oid, np.ascontiguousarray(got_planes[oid])), want, f"frame {f} {label} output {oid}")
        if m:
            errors.append(m)
    W = o.output(10).shape[1]
    for rid in range(10):
        want = canon_reservoirs(o.reservoirs(rid)[: o.output(10).shape[0] * W]).reshape(-1, W, 16)[rows]
        m = mismatch_report(got_res[rid], want, f"frame {f} {label} reservoir {rid}")
        if m:
            errors.append(m)


@pytest.mark.parametrize("kind", ["stripes", "bands"])
def test_decompositions_bit_exact(kind):
    """64 x 64 as two interleaved stripe contexts and as two row bands with halo, frames 0-3, against the whole-frame
    oracle: the shared texel index goes through band_index's stripe map and its row clamp.  Each part's own rows of
    every plane and reservoir buffer, and the parts' counters added up."""
    from hikari_amd import examples, frame_inputs, load_noise
    from hikari_amd.bands import halo_rows
    from oracle import Oracle
    W = H = 64
    scene, cam, lights = examples.cornell()
    desc = scene.build()
    neighbours = kind == "bands"  # the stripes refuse the passes that read neighbours
    st = _settings(indirect_spatial_reuse=neighbours, denoise=neighbours)
    s = st.to_c()
    o = Oracle(desc, load_noise(), W, H, 1.0)
    ranks = decomposed(scene, 2, W, H, kind, halo_rows(neighbours, neighbours) if neighbours else 0)
    errors = []
    for f in range(4):
        fi = frame_inputs(f, cam, lights, W, H)
        for x in [o] + [r for _, r in ranks]:
            passes(x, s, fi)
        for k, (rect, r) in enumerate(ranks):
            row0, rows, core0, core_rows = r.band_info()
            if kind == "stripes":
                assert core0 == 0 and rows == core_rows
                local = np.arange(rows)
                frame_rows = ((local // 8) * 2 + k) * 8 + local % 8  # stripe k, k + 2, ...: 8 rows each
            else:
                assert row0 + core0 == rect.y0 and core_rows == rect.rows
                frame_rows = np.arange(rect.y0, rect.y0 + rect.rows)
            own = slice(core0, core0 + core_rows)
            planes = [r.output(oid)[own] for oid in range(17)]
            res = [canon_reservoirs(r.reservoirs(rid)).reshape(-1, W, 16)[own] for rid in range(10)]
            _compare_rows(errors, f, f"{kind} part {k}", planes, res, o, frame_rows)
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert summed_counters(ranks) == o.counters()
