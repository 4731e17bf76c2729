"""The oracle's texture sampler (include/hk_texture.h through hko_sample_texture) against the independent float32
restatement of tests/texture_numpy.py: every stored word, over every image size class, every (format, address_u,
address_v, filter) and a UV set that sits on the seams, the texel centres, the int32 saturation boundaries and the
non-finite values.  The decode table is checked on its own against the float64 formula; seven misreadings of the
definition, applied to the restatement, are each caught."""
import numpy as np
import pytest

import texture_numpy as tn


@pytest.fixture(scope="module")
def oracle():
    from hikari_amd import examples, load_noise
    from oracle import Oracle
    scene, _, _ = examples.cornell()
    o = Oracle(scene.build(), load_noise(), 8, 8, 1.0)
    o._scene = scene
    return o


@pytest.fixture(scope="module")
def oracle_lut(oracle):
    from hikari_amd import Texture
    t, uv = tn.ramp()
    oracle.set_textures([Texture(t, srgb=True, filter=0), Texture(t, srgb=False, filter=0)])
    s, l_ = oracle.sample_texture(0, uv), oracle.sample_texture(1, uv)
    # one table per format whatever the channel, alpha of an sRGB image through the unorm table
    assert np.array_equal(s[:, 0], s[:, 1]) and np.array_equal(s[:, 0], s[:, 2])
    assert np.array_equal(l_[:, 0], l_[:, 1]) and np.array_equal(l_[:, 0], l_[:, 2]) and np.array_equal(l_[:, 0], l_[:, 3])
    assert np.array_equal(s[:, 3], l_[:, 3])
    return np.stack([s[:, 0], l_[:, 0]])


@pytest.fixture(scope="module")
def bank_results(oracle, oracle_lut):
    """[(entry, uv, oracle words)] for the whole bank, uploaded as one set of 252 textures."""
    bank = tn.bank()
    oracle.set_textures(tn.bank_textures())
    out = []
    for tid, entry in enumerate(bank):
        h, w = entry[0].shape[:2]
        uv = tn.uv_set(w, h)
        got = oracle.sample_texture(tid, uv)
        got.setflags(write=False)
        out.append((entry, uv, got))
    return out


def test_decode_table(oracle_lut):
    b = np.arange(256)
    # unorm: byte / 255 in f32, exactly
    assert np.array_equal(oracle_lut[1], b.astype(np.float32) / np.float32(255.0))
    assert np.array_equal(oracle_lut[1], tn.decode_reference(b, False).astype(np.float32))
    srgb = oracle_lut[0]
    assert srgb[0] == 0.0 and srgb[255] == 1.0 and np.all(np.diff(srgb) > 0)
    # the linear branch takes exactly bytes 0..10 (10/255 = 0.0392 <= 0.04045 < 11/255 = 0.0431): there the table is
    # the f32 quotient itself
    c = b.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(srgb[:11], c[:11] / np.float32(12.92))
    assert not np.any(srgb[11:] == c[11:] / np.float32(12.92))
    assert int(np.sum(c <= np.float32(0.04045))) == 11
    want = tn.decode_reference(b, True)
    ulp = np.abs(srgb.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    print(f"sRGB decode table: worst distance from the float64 formula {ulp.max():.2f} ulp at byte {int(ulp.argmax())}")
    assert ulp.max() <= 8


def test_uv_set_sits_on_its_edges():
    """The UV set holds what it claims: seams with both neighbours, the saturation boundaries, the non-finite values."""
    uv = tn.uv_set(3, 5)
    u = uv[:, 0]
    third = np.float32(1.0 / 3.0)
    for x in (third, np.nextafter(third, np.float32(0)), np.nextafter(third, np.float32(1)), np.float32(-7.0 / 3.0),
              np.float32(10.0 / 3.0)):
        assert np.any(u == x)
    for x in (2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, np.inf, -np.inf):
        assert np.any(u == np.float32(x)) and np.any(uv[:, 1] == np.float32(x))
    assert np.isnan(uv).any() and np.any((u == 0) & np.signbit(u)) and np.any((u > 0) & (u < 1e-44))
    # 3 * 5 texel centres, and draws over [-2.5, 3.5]
    assert np.any((u == np.float32(0.5 / 3)) & (uv[:, 1] == np.float32(4.5 / 5)))
    fin = uv[np.isfinite(uv).all(axis=1)]
    assert np.sum((np.abs(fin) < 4).all(axis=1) & ((fin < 0) | (fin > 1)).any(axis=1)) > 3000
    # saturation is reached from both sides, and the coordinate just below it is not saturated
    with np.errstate(over="ignore"):
        i = tn.to_int(np.floor(u * np.float32(3)))
    assert np.any(i == tn.INT_MAX) and np.any(i == tn.INT_MIN)
    assert tn.to_int(np.float32(2147483520.0)) == 2147483520 and tn.to_int(np.float32(-2147483904.0)) == tn.INT_MIN


def test_oracle_sampler_equals_restatement_in_every_word(bank_results, oracle_lut):
    words = 0
    for (texels, fmt, au, av, fl), uv, got in bank_results:
        want = tn.sample(texels, fmt == tn.SRGB, au, av, fl, uv, oracle_lut)
        bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
        assert not bad.any(), (texels.shape[:2], (fmt, au, av, fl), int(bad.sum()), uv[bad.any(axis=1)][:4].tolist())
        words += got.size
    assert words > 9_000_000


def test_textures_of_one_upload_do_not_read_each_other(oracle, bank_results):
    """Each texture of the bank sits at its own texel offset behind images of other sizes.  Re-uploading a texture
    alone (offset 0) gives the words it gave inside the bank, and the bank's offsets are no multiple of anything."""
    textures = tn.bank_textures()
    sizes = [t.rgba8.shape[0] * t.rgba8.shape[1] for t in textures]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert np.any(offsets % 2 == 1) and np.any(offsets % 4 == 3) and len(set(sizes)) >= 6
    try:
        for tid in (37, 36 * 3 + 5, 36 * 4 + 35, 36 * 6 + 17, 251):
            assert offsets[tid] > 0
            oracle.set_textures([textures[tid]])
            _, uv, got = bank_results[tid]
            assert tn.same_words(oracle.sample_texture(0, uv), got), tid
    finally:
        oracle.set_textures(textures)


@pytest.mark.parametrize("misread", tn.MISREADINGS)
def test_misreadings_of_the_definition_are_caught(bank_results, oracle_lut, misread):
    differing = 0
    for (texels, fmt, au, av, fl), uv, got in bank_results:
        if texels.shape[:2] not in ((5, 3), (3, 257)):  # (H, W): the two non-square images with an interior
            continue
        wrong = tn.sample(texels, fmt == tn.SRGB, au, av, fl, uv, oracle_lut, misread=misread)
        differing += not tn.same_words(wrong, got)
    assert differing > 0, misread
