"""The present pass (overlay.wgsl / overlay.rs) pinned by an independent restatement, on the CPU.

include/hk_overlay.h holds the per-pixel body that the gfx950 kernels and the CPU side of the GPU parity test
(tests/overlay_cpu.c) both compile, so GPU == CPU alone cannot catch a misreading made in the header.  Here
tests/overlay_cpu.c, built with the oracle's flags, is compared with tests/overlay_numpy.py, a vectorised restatement
written from the shader: float32 sampling and HDR path, and the sRGB encode by the standard's formula in float64, not
by the header's threshold table.  Every stored byte or word must be equal (f16 NaNs canonicalised).  The table itself is
checked against tools/srgb_thresholds.py's exact rational arithmetic.
"""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import overlay_numpy as on
from parity import canon_f16

ROOT = Path(__file__).resolve().parent.parent
CFLAGS = ["-O3", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

FORMATS = [on.RGBA8_SRGB, on.BGRA8_SRGB, on.RGBA16F]
BPP = {on.RGBA8_SRGB: 4, on.BGRA8_SRGB: 4, on.RGBA16F: 8}
SIZES = [(1, 1), (2, 3), (5, 4), (21, 16), (32, 24)]  # input (w, h)
KINDS = ["constant", "black", "noise", "ramp", "out_of_range", "nan_texel", "nan_alpha", "nan_beside"]
MUTATIONS = ["y_not_flipped", "nan_rgb_only", "l_plus", "no_clamp", "srgb_alpha", "albedo_nearest"]
SENTINEL = 0xA5


class OverlayCpu:
    """tests/overlay_cpu.c compiled into `directory` and loaded with ctypes."""

    def __init__(self, directory):
        so = Path(directory) / "liboverlay_cpu.so"
        subprocess.run(["gcc", *CFLAGS, "-I", str(ROOT / "include"), "-shared", "-o", str(so),
                        str(ROOT / "tests" / "overlay_cpu.c"), "-lm"], check=True)
        L = C.CDLL(str(so))
        vp, u32 = C.c_void_p, C.c_uint32
        L.overlay_cpu.argtypes = [vp, u32, u32, vp, u32, u32, vp, u32, u32, u32, u32, u32, u32]
        L.overlay_cpu.restype = None
        L.overlay_cpu_table.restype = C.POINTER(C.c_float * 256)
        L.overlay_cpu_codes.argtypes = [vp, u32, vp]
        L.overlay_cpu_codes.restype = None
        self.L = L

    def present(self, input, albedo, width, height, fmt, viewport=None, pitch=0, fill=SENTINEL):
        """input, albedo: (h, w, 4) uint16 RGBA16F.  Returns the whole target as (height, pitch) bytes, prefilled with
        `fill`; pitch 0: packed rows."""
        src, alb = np.ascontiguousarray(input, np.uint16), np.ascontiguousarray(albedo, np.uint16)
        pitch = pitch or width * BPP[fmt]
        vx, vy, vw, vh = viewport or (0, 0, width, height)
        out = np.full((height, pitch), fill, np.uint8)
        self.L.overlay_cpu(src.ctypes.data, src.shape[1], src.shape[0], alb.ctypes.data, alb.shape[1], alb.shape[0],
                           out.ctypes.data, pitch, fmt, vx, vy, vw, vh)
        return out

    def table(self):
        return np.array(self.L.overlay_cpu_table().contents, np.float32)

    def codes(self, c):
        c = np.ascontiguousarray(c, np.float32)
        out = np.empty(len(c), np.uint8)
        self.L.overlay_cpu_codes(c.ctypes.data, len(c), out.ctypes.data)
        return out


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return OverlayCpu(tmp_path_factory.mktemp("overlay_cpu"))


def srgb_decode(e):
    return np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4)


def image(kind, w, h, seed=0):
    """A synthetic RGBA16F image (h, w, 4) as uint16 words."""
    rng = np.random.default_rng(0x0E71 + 97 * w + h + 1009 * seed)
    img = rng.uniform(0.0, 1.0, (h, w, 4))
    n = w * h
    if kind == "constant":
        img[:] = [0.5, 0.25, 0.75, 0.6]
    elif kind == "black":
        img[:] = [0.0, 0.0, 0.0, 1.0]
    elif kind == "ramp":
        # the centre of every sRGB code's bucket, a different order per channel, from the first texel on
        k = np.arange(n) % 256
        flat = img.reshape(n, 4)
        for ch, order in enumerate((k, 255 - k, (k * 7) % 256)):
            flat[:, ch] = srgb_decode(order / 255.0)
    elif kind == "out_of_range":
        img = img * 3.0 - 1.0
        for k in range(max(1, n // 20)):
            img[rng.integers(h), rng.integers(w), rng.integers(4)] = np.inf if k % 2 == 0 else -np.inf
    img = img.astype(np.float16)
    if kind == "nan_texel":
        img[h // 2, w // 2, :] = np.nan
    elif kind == "nan_alpha":
        img[h // 3, w // 3, 3] = np.nan
    elif kind == "nan_beside":
        img[h // 2, w // 2, 1] = np.nan
        img[0, w - 1, 0] = np.nan  # a plane corner
    return np.ascontiguousarray(img).view(np.uint16)


def decode(words):
    return words.view(np.float16).astype(np.float32)


def targets(w, h):
    """(width, height, viewport, pitch bytes beyond the row) for an input of w x h: the identity size, 1 x 1, larger
    and smaller targets, a viewport strictly inside a target at an odd origin, a pitch larger than the row."""
    return [(w, h, None, 0), (1, 1, None, 0), (50, 37, None, 0), (7, 5, None, 12), (2 * w, 2 * h, None, 0),
            (50, 37, (3, 5, 40, 29), 12), (w + 6, h + 4, (5, 1, w, h), 0)]


def view(out, fmt, viewport, width, height):
    """The viewport's texels of a target (height, pitch) as (vh, vw, 4) uint8 / uint16, and the bytes outside it."""
    b = BPP[fmt]
    vx, vy, vw, vh = viewport or (0, 0, width, height)
    inside = np.zeros(out.shape, bool)
    inside[vy:vy + vh, vx * b:(vx + vw) * b] = True
    tex = np.ascontiguousarray(out[vy:vy + vh, vx * b:(vx + vw) * b])
    tex = tex.view(np.uint16).reshape(vh, vw, 4) if fmt == on.RGBA16F else tex.reshape(vh, vw, 4)
    return tex, out[~inside]


def same(got, want, fmt):
    return np.array_equal(canon_f16(got), canon_f16(want)) if fmt == on.RGBA16F else np.array_equal(got, want)


def both(cpu, kind, w, h, fmt, target, mutate=None, albedo_kind="noise"):
    width, height, viewport, extra = target
    src = image(kind, w, h)
    alb = image(albedo_kind, w + 3, h + 2, seed=1) if (w + h) % 2 else image(albedo_kind, w, h, seed=1)
    out = cpu.present(src, alb, width, height, fmt, viewport, (width * BPP[fmt] + extra) if extra else 0)
    got, outside = view(out, fmt, viewport, width, height)
    vw, vh = (viewport or (0, 0, width, height))[2:]
    want = on.overlay(decode(src), decode(alb), vw, vh, fmt, mutate)
    return got, want, outside


def test_threshold_table_is_exact(cpu):
    """Every T[k] is the smallest f32 whose exact sRGB encode times 255 reaches k - 0.5 (tools/srgb_thresholds.py, in
    rational arithmetic), in the header's text and in the compiled table."""
    sys.path.insert(0, str(ROOT / "tools"))
    import srgb_thresholds as st
    exact = np.array(st.thresholds(), np.float64)
    assert len(exact) == 256 and exact[0] == 0.0 and (np.diff(exact) > 0).all()
    assert np.array_equal(np.array(st.header_values(), np.float64), exact)
    assert np.array_equal(cpu.table().astype(np.float64), exact)
    # the definition, spot-checked in float64 away from the rounding of either side: the f32 below T[k] encodes below
    # k - 0.5, T[k] itself at or above, within float64's error
    t = cpu.table()[1:]
    below = np.nextafter(t, np.float32(0))
    k = np.arange(1, 256)
    assert (255.0 * on.srgb_encode(t) >= k - 0.5 - 1e-9).all() and (255.0 * on.srgb_encode(below) <= k - 0.5 + 1e-9).all()


def test_srgb_code_is_the_count(cpu):
    """The body's code equals a searchsorted on T: at every T[k], just below it, at 0, 1, the knee 0.0031308 and its
    neighbours, and on 10^6 random f32 in [-0.5, 1.5] (NaN and the clamp included)."""
    t = cpu.table()
    knee = np.float32(0.0031308)
    special = np.array([0.0, 1.0, knee, np.nextafter(knee, np.float32(0)), np.nextafter(knee, np.float32(1)), -0.0,
                        np.nan, np.inf, -np.inf, 2.0, -1.0], np.float32)
    rnd = np.random.default_rng(7).uniform(-0.5, 1.5, 1_000_000).astype(np.float32)
    c = np.concatenate([t[1:], np.nextafter(t[1:], np.float32(0)), special, rnd])
    clamped = np.clip(np.where(np.isnan(c), np.float32(0), c), np.float32(0), np.float32(1))
    want = np.searchsorted(t[1:], clamped, side="right")  # #{k : T[k] <= c}
    got = cpu.codes(c)
    assert np.array_equal(got, want.astype(np.uint8))
    assert np.array_equal(cpu.codes(t[1:]), np.arange(1, 256)) and np.array_equal(
        cpu.codes(np.nextafter(t[1:], np.float32(0))), np.arange(0, 255))
    # and it is the nearest code of the float64 formula wherever that is not within 1e-6 of a tie
    e = 255.0 * on.srgb_encode(clamped)
    clear = np.abs(e - np.floor(e) - 0.5) > 1e-6
    assert np.array_equal(got[clear], np.floor(e[clear] + 0.5).astype(np.uint8))


@pytest.mark.parametrize("fmt", FORMATS, ids=["rgba8", "bgra8", "rgba16f"])
@pytest.mark.parametrize("kind", KINDS)
def test_matches_restatement(cpu, kind, fmt):
    for (w, h) in SIZES:
        for target in targets(w, h):
            got, want, outside = both(cpu, kind, w, h, fmt, target)
            assert same(got, want, fmt), f"{kind} {w}x{h} -> {target}: {int((got != want).sum())} words"
            assert (outside == SENTINEL).all(), f"{kind} {w}x{h} -> {target}: bytes outside the viewport written"


@pytest.mark.parametrize("fmt", [on.RGBA8_SRGB, on.BGRA8_SRGB], ids=["rgba8", "bgra8"])
def test_ramp_reaches_every_code(cpu, fmt):
    got, want, _ = both(cpu, "ramp", 32, 24, fmt, (32, 24, None, 0))
    for ch in range(3):
        assert len(np.unique(got[..., ch])) == 256


def test_bgra_swaps_red_and_blue(cpu):
    a, _, _ = both(cpu, "noise", 21, 16, on.RGBA8_SRGB, (50, 37, None, 0))
    b, _, _ = both(cpu, "noise", 21, 16, on.BGRA8_SRGB, (50, 37, None, 0))
    assert np.array_equal(a[..., [2, 1, 0, 3]], b) and not np.array_equal(a, b)


@pytest.mark.parametrize("fmt", FORMATS, ids=["rgba8", "bgra8", "rgba16f"])
def test_nan_turns_the_whole_footprint_to_albedo(cpu, fmt):
    """At the identity size the blend's weights are near 0 and 1 but the four texels are all read: every pixel whose
    footprint holds the NaN texel (0 * NaN) takes the albedo's sample, a 2 x 2 block or more; the rest do not."""
    w, h = 21, 16
    src, alb = image("nan_beside", w, h), image("noise", w + 3, h + 2, seed=1)
    clean = src.copy()
    nan = np.isnan(decode(src))
    clean[nan] = image("noise", w, h).copy()[nan]
    assert not np.isnan(decode(clean)).any()
    args = (w, h, fmt)
    with_nan, _ = view(cpu.present(src, alb, *args), fmt, None, w, h)
    without, _ = view(cpu.present(clean, alb, *args), fmt, None, w, h)
    # the albedo presented as the input, at the same uv: what a fallen-back pixel must hold
    alb_at_size, _ = view(cpu.present(alb, alb, *args), fmt, None, w, h)
    changed = (canon_f16(with_nan) != canon_f16(without)).any(axis=-1)
    ys, xs = np.nonzero(changed)
    assert changed.sum() >= 4 + 1  # the interior texel's 2 x 2 block or more, and the corner's pixel
    assert changed[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1].sum() + changed[h // 2:h // 2 + 2, w // 2:w // 2 + 2].sum() >= 4
    assert changed[0, w - 1]
    assert np.array_equal(canon_f16(with_nan[changed]), canon_f16(alb_at_size[changed]))
    assert len(ys) < w * h // 4


def test_hdr_black_is_nan_and_covered_pixels_brighten(cpu):
    """Inverse Reinhard: a black pixel is 0 * (l_new / 0) = NaN and stored as such; a pixel with luminance in
    (0.0005, 0.995) grows (l / (1 - l) > l)."""
    black, _, _ = both(cpu, "black", 5, 4, on.RGBA16F, (5, 4, None, 0))
    assert np.isnan(decode(black)[..., :3]).all() and (decode(black)[..., 3] == 1.0).all()
    got, _, _ = both(cpu, "constant", 5, 4, on.RGBA16F, (7, 5, None, 12))
    assert np.isfinite(decode(got)).all() and (decode(got)[..., :3] > np.float32([0.5, 0.25, 0.75])).all()
    assert (decode(got)[..., 3] == np.float32(np.float16(0.6))).all()


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_misreadings_are_caught(cpu, mutation):
    """Each misreading, applied to the restatement, changes the stored words of at least one case."""
    for kind in KINDS:
        for fmt in FORMATS:
            for (w, h) in SIZES[2:]:
                for target in targets(w, h)[:3]:
                    got, bad, _ = both(cpu, kind, w, h, fmt, target, mutate=mutation)
                    if not same(got, bad, fmt):
                        return
    pytest.fail(f"{mutation} changed no case")


def test_header_declares_present_and_keeps_the_abi():
    import hikari_amd
    A = hikari_amd._abi
    header = (ROOT / "include" / "hikari_amd.h").read_text()
    for name in ("hk_present", "hk_present_info", "hk_get_present"):
        assert f"int {name}(" in header and name in A.EXPORTED_SYMBOLS and hasattr(A.lib(), name)
    assert "HK_OUT_COUNT = 23" in header and "#define HK_ABI_VERSION 3" in header and A.lib().hk_abi_version() == 3
    assert "HK_PRESENT_RGBA8_SRGB = 0, HK_PRESENT_BGRA8_SRGB = 1, HK_PRESENT_RGBA16F = 2" in header
    doc = header[header.index("Runtime options"):header.index("int hk_set_option")]
    assert "present_run" in doc
    assert [int(f) for f in hikari_amd.PresentFormat] == [0, 1, 2]
    assert hikari_amd.PresentFormat.of("bgra8_srgb") is hikari_amd.PresentFormat.BGRA8_SRGB
    for cls, method in ((hikari_amd.HikariRenderer, "present"), (hikari_amd.HikariRenderer, "get_present"),
                        (hikari_amd.HikariRenderer, "present_info"), (hikari_amd.HikariPlugin, "present")):
        assert hasattr(cls, method)


def test_present_target_mirror_matches_header(tmp_path):
    """The ctypes hk_present_target has the C compiler's size and offsets."""
    import hikari_amd
    cls = hikari_amd._abi.hk_present_target
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hikari_amd.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(hk_present_target));']
    lines += [f'printf("{f} %zu\\n", offsetof(hk_present_target, {f}));' for f, _ in cls._fields_]
    lines.append("return 0;}")
    src, exe = tmp_path / "present.c", tmp_path / "present"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f
