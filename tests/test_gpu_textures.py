"""The textured material path on the device.

The sampler: hk_selftest_texture runs the kernels' own sample_material_texture over the bank of
tests/texture_numpy.py (every size class, every format / address pair / filter, uvs on the seams, the texel centres, the
int32 saturation boundaries and the non-finite values) and must give the words of the independent restatement and of
the CPU oracle, which share include/hk_texture.h with the kernels: hipcc's device code against gcc's host code.

The scenes: every case of tests/texture_cases.py (each proven to sit on its edge by tests/test_texture_cases.py) bit for
bit against the oracle, whose frames are computed once per case; wrap_all and emitters_textured also under the staging
settings, the ladder's launch variants, ratio 1.5, an orthographic view, a moving camera and two row bands; texture
uploads that change count and sizes under a running history; a material replacement that gives and takes a texture."""
import copy

import numpy as np
import pytest

import scene_ladder as sl
import texture_cases as tc
import texture_numpy as tn
from parity import (RACY, canon_frame, canon_plane, compare_frame, decomposed, orbit_camera, passes, renderer, run_frames,
                    summed_counters)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the sampler
@pytest.fixture(scope="module")
def sampler_pair():
    """(renderer, oracle) on the Cornell scene; the tests upload their own textures to both."""
    from hikari_amd import examples, load_noise
    from oracle import Oracle
    scene, _, _ = examples.cornell()
    scene.build()
    r = renderer(scene, (8, 8))
    o = Oracle(scene.desc, load_noise(), 8, 8, 1.0)
    yield r, o
    o.close()
    r.close()


def _upload(pair, textures):
    r, o = pair
    r.upload_textures(textures)
    o.set_textures(textures)


def _ramp_luts(pair):
    from hikari_amd import Texture
    t, uv = tn.ramp()
    _upload(pair, [Texture(t, srgb=True, filter=0), Texture(t, srgb=False, filter=0)])
    r, o = pair
    return [np.stack([x(0, uv), x(1, uv)]) for x in (r.selftest_texture, o.sample_texture)]


def test_device_decode_table_equals_the_oracles(sampler_pair):
    dev, cpu = _ramp_luts(sampler_pair)
    assert dev.shape == (2, 256, 4) and dev.tobytes() == cpu.tobytes()
    assert np.array_equal(dev[0, :, 3], dev[1, :, 0])  # alpha of the sRGB image through the unorm table
    assert np.array_equal(dev[1, :, 0], np.arange(256, dtype=np.float32) / np.float32(255.0))


def test_device_sampler_equals_restatement_and_oracle(sampler_pair):
    dev, _ = _ramp_luts(sampler_pair)
    lut = dev[:, :, 0]
    bank = tn.bank()
    _upload(sampler_pair, tn.bank_textures())
    r, o = sampler_pair
    words, bad = 0, []
    for tid, (texels, fmt, au, av, fl) in enumerate(bank):
        h, w = texels.shape[:2]
        uv = tn.uv_set(w, h)
        got = r.selftest_texture(tid, uv)
        if not tn.same_words(got, o.sample_texture(tid, uv)):
            bad.append(("oracle", (w, h), (fmt, au, av, fl)))
        if not tn.same_words(got, tn.sample(texels, fmt == tn.SRGB, au, av, fl, uv, lut)):
            bad.append(("restatement", (w, h), (fmt, au, av, fl)))
        words += got.size
    assert not bad, bad[:10]
    assert words > 9_000_000


def test_selftest_texture_refusals_leave_the_context_usable(sampler_pair):
    from hikari_amd import Texture, _abi
    r, o = sampler_pair
    t = [Texture(tn.random_texels(3, 5, 1), srgb=True), Texture(tn.random_texels(2, 2, 2), srgb=False)]
    _upload(sampler_pair, t)
    uv = np.array([[0.25, 0.75], [1.5, -0.5]], np.float32)
    out = np.full((2, 4), 7.0, np.float32)
    call = r._L.hk_selftest_texture
    for tid in (2, 9, 0xFFFFFFFF):
        assert call(r.ctx, tid, uv.ctypes.data, 2, out.ctypes.data) == _abi.HK_ERR_INVALID
    assert call(r.ctx, 0, None, 2, out.ctypes.data) == _abi.HK_ERR_INVALID
    assert call(r.ctx, 0, uv.ctypes.data, 2, None) == _abi.HK_ERR_INVALID
    assert call(None, 0, uv.ctypes.data, 2, out.ctypes.data) == _abi.HK_ERR_INVALID
    assert np.all(out == 7.0)
    assert call(r.ctx, 1, None, 0, None) == _abi.HK_OK and np.all(out == 7.0)  # n == 0: nothing to do
    assert r.selftest_texture(1, np.zeros((0, 2), np.float32)).shape == (0, 4)
    r.upload_textures([])
    assert call(r.ctx, 0, uv.ctypes.data, 2, out.ctypes.data) == _abi.HK_ERR_INVALID  # none uploaded
    r.upload_textures(t)
    for tid in (0, 1):
        assert tn.same_words(r.selftest_texture(tid, uv), o.sample_texture(tid, uv))


# ------------------------------------------------------------------ the scene cases
_reference = {}
_built = {}


def _triple(name):
    if name not in _built:
        scene, cam, lights = tc.CASES[name]()
        scene.build()
        _built[name] = (scene, cam, lights)
    return _built[name]


def _oracle_frames(key, triple, inputs, settings, size, ratio=1.0, threads=None):
    """The oracle's canonical frames and counters for these inputs, once per key."""
    from hikari_amd import load_noise
    from oracle import Oracle
    if key not in _reference:
        scene = triple[0]
        o = Oracle(scene.desc, load_noise(), *size, ratio, textures=scene.textures,
                   **({} if threads is None else {"threads": threads}))
        s = settings.to_c()
        out = []
        for fi in inputs:
            passes(o, s, fi)
            out.append(canon_frame(o))
        _reference[key] = (out, o.counters())
        o.close()
    return _reference[key]


def _static(name, bounces=2, wavefront=False, camera=None, tag=""):
    """The case over frames 0..5 at 64 x 48 with both spatial passes, `bounces` bounces and the denoiser: all outputs,
    all reservoir buffers, the counters."""
    from hikari_amd import frame_inputs
    triple = _triple(name)
    scene, cam, lights = triple
    cam = camera or cam
    w, h = tc.SIZE
    st = tc.settings(bounces)
    inputs = [frame_inputs(f, cam, lights, w, h) for f in range(tc.FRAMES)]
    ref = _oracle_frames((name, bounces, tag), triple, inputs, st, (w, h))
    r = renderer(scene, (w, h), wavefront=wavefront)
    run_frames(r, ref, st.to_c(), inputs, label=name + " ")
    r.close()


@pytest.mark.parametrize("name", list(tc.CASES))
def test_texture_case_bit_exact(name):
    _static(name)


VARIED = ["wrap_all", "emitters_textured"]


@pytest.mark.parametrize("lds", [0, 1, 2])
@pytest.mark.parametrize("name", VARIED)
def test_texture_case_under_scene_staging(hk_options, name, lds):
    hk_options["lds_scene"] = lds
    _static(name)


@pytest.mark.parametrize("variant", list(sl.LAUNCH_VARIANTS))
@pytest.mark.parametrize("name", VARIED)
def test_texture_case_under_launch_variants(hk_options, name, variant):
    """The ladder's launch variants (scene_ladder.LAUNCH_VARIANTS), the wavefront indirect pass included, as
    test_ladder_launch_variants_bit_exact runs them: lds_scene = 2 unless the variant sets it."""
    hk_options["lds_scene"] = 2
    hk_options.update(sl.LAUNCH_VARIANTS[variant])
    _static(name, bounces=2 if variant == "bounces_2" else 1, wavefront=variant == "wavefront")


@pytest.mark.parametrize("name", VARIED)
def test_texture_case_at_ratio_1_5(name):
    """63 x 47 at upscale ratio 1.5: the integrator grid is smaller than the G-buffer and no divisor of it, so the
    light passes read the uv plane at scaled pixel positions."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    triple = _triple(name)
    scene, cam, lights = triple
    w, h = 63, 47
    st = HikariSettings(upscale=Upscale.smaa_tu4x(1.5), emissive_spatial_reuse=True, indirect_bounces=2, denoise=True)
    inputs = [frame_inputs(f, cam, lights, w, h) for f in range(tc.FRAMES)]
    ref = _oracle_frames((name, "ratio"), triple, inputs, st, (w, h), 1.5)
    r = renderer(scene, (w, h), 1.5)
    sw, sh, _ = r.output_info(4)
    assert (sw, sh) != (w, h)
    run_frames(r, ref, st.to_c(), inputs, label=name + " ")
    r.close()


@pytest.mark.parametrize("name", VARIED)
def test_texture_case_orthographic(name):
    from hikari_amd import Camera
    cam = Camera.orthographic(_triple(name)[1].transform, 3.0)
    _static(name, camera=cam, tag="orthographic")


@pytest.mark.parametrize("name", VARIED)
def test_texture_case_moving_camera(name):
    """parity.orbit_camera, spatial reuse off and the oracle single-threaded (raster order), as the other moving-camera
    tests: everything outside the racy scatter targets bit-exact, those by RACY_MIN_EXACT."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    triple = _triple(name)
    scene, cam, lights = triple
    w, h = tc.SIZE
    st = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False, indirect_bounces=2, denoise=True)
    inputs, prev = [], None
    for f in range(tc.FRAMES):
        c = orbit_camera(cam, f)
        inputs.append(frame_inputs(f, c, lights, w, h, previous_camera=prev))
        prev = copy.deepcopy(c)
    ref = _oracle_frames((name, "orbit"), triple, inputs, st, (w, h), threads=1)
    r = renderer(scene, (w, h))
    run_frames(r, ref, st.to_c(), inputs, label=name + " ", racy=RACY)
    vel = r.output(15).view(np.float32).reshape(h, w, 4)[..., :2]
    assert (vel != 0).any(axis=-1).sum() > 0.2 * w * h
    r.close()


@pytest.mark.parametrize("name", VARIED)
def test_texture_case_as_two_row_bands(name):
    """Two band contexts (parity.decomposed) reproduce the whole-frame oracle on their own rows of planes 0..16 after
    frames 0..5, and their counters add up to the oracle's."""
    from hikari_amd import frame_inputs
    from hikari_amd.bands import halo_rows
    triple = _triple(name)
    scene, cam, lights = triple
    w, h = tc.SIZE
    st = tc.settings(2)
    inputs = [frame_inputs(f, cam, lights, w, h) for f in range(tc.FRAMES)]
    frames, counters = _oracle_frames((name, 2, ""), triple, inputs, st, (w, h))
    ranks = decomposed(scene, 2, w, h, "bands", halo_rows(True, True))
    s = st.to_c()
    for fi in inputs:
        for _, r in ranks:
            passes(r, s, fi)
    for b, r in ranks:
        row0, rows, core0, core_rows = r.band_info()
        assert row0 + core0 == b.y0 and core_rows == b.rows
        for oid in range(17):
            mine = canon_plane(oid, r.output(oid)[core0: core0 + core_rows])
            whole = frames[-1][0][oid].reshape(h, -1)[b.y0: b.y0 + b.rows]
            assert np.array_equal(mine.reshape(core_rows, -1), whole), (b, oid)
    assert summed_counters(ranks) == counters
    for _, r in ranks:
        r.close()


# ------------------------------------------------------------------ the runtime side
def test_texture_uploads_swap_under_a_running_history():
    """tc.swap_uploads: A, B (another count, other sizes), none, A — uploaded between frames to a renderer and set on the
    oracle, the reservoir history carried throughout; every frame bit-exact."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    (scene, cam, lights), uploads = tc.swap_uploads()
    scene.build()
    w, h = tc.SIZE
    st = tc.settings(2)
    s = st.to_c()
    r = renderer(scene, (w, h))
    o = Oracle(scene.desc, load_noise(), w, h, 1.0, textures=scene.textures)
    errors, f = [], 0
    for k, (textures, n) in enumerate(uploads):
        if k:
            r.upload_textures(textures)
            o.set_textures(textures)
        for _ in range(n):
            fi = frame_inputs(f, cam, lights, w, h)
            for x in (r, o):
                passes(x, s, fi)
            compare_frame(r, o, f, errors)
            f += 1
        assert not errors, f"upload {k}\n" + "\n".join(errors[:10])
    assert f == 8 and r.counters() == o.counters()
    o.close()
    r.close()


def test_a_material_gains_and_loses_a_texture_through_set_instances():
    """tc.gains_texture: two frames on the uploaded materials, hk_set_instances with the replaced material records,
    two more; the oracle takes the host-built scene of step 1."""
    import instance_set_cases as ic
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    case, cam, lights = tc.gains_texture()
    w, h = tc.SIZE
    st = tc.settings(2)
    s = st.to_c()
    r = renderer(case.scenes[0], (w, h))
    o = Oracle(case.scenes[0].desc, load_noise(), w, h, 1.0, textures=case.scenes[0].textures)
    errors, f = [], 0
    for k, scene in enumerate(case.scenes):
        if k:
            r.set_instances(scene, previous=case.previous[k], materials=True, local_aabbs=ic.local_aabbs(scene))
            o.set_scene(scene.build())
        for _ in range(2):
            fi = frame_inputs(f, cam, lights, w, h)
            for x in (r, o):
                passes(x, s, fi)
            compare_frame(r, o, f, errors)
            f += 1
        assert not errors, f"step {k}\n" + "\n".join(errors[:10])
    assert r.counters() == o.counters()
    o.close()
    r.close()
