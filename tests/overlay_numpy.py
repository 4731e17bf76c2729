"""The present pass restated from overlay.wgsl / overlay.rs in vectorised numpy: a second reading that does not include
include/hk_overlay.h.  Sampling and the HDR path are float32 in the shader's order (every numpy operation on float32
arrays is one exactly rounded f32 operation); the sRGB encode is the standard's formula in float64, rounded to nearest,
not the header's threshold table.  TEST INFRASTRUCTURE (tests/test_overlay_independent.py).

`mutate` applies one deliberate misreading, which the tests require to change the result:
    y_not_flipped   clip_to_uv without `uv.y = 1 - uv.y`
    nan_rgb_only    any_is_nan_vec3 in place of any_is_nan_vec4
    l_plus          l / (1 + l) in place of l / (1 - l)
    no_clamp        l_old not clamped to [0.0005, 0.995]
    srgb_alpha      the sRGB curve applied to alpha as well
    albedo_nearest  the albedo through the nearest sampler
"""
import numpy as np

F = np.float32
RGBA8_SRGB, BGRA8_SRGB, RGBA16F = 0, 1, 2


def _footprint(n, coord):
    x = coord * F(n) - F(0.5)
    x0 = np.floor(x)
    i0 = x0.astype(np.int64)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), x - x0


def linear(tex, u, v):
    """textureSample through the linear clamp-to-edge sampler: tex (h, w, 4) float32, u (vw,), v (vh,) -> (vh, vw, 4)."""
    h, w = tex.shape[:2]
    i0, i1, a = _footprint(w, u)
    j0, j1, b = _footprint(h, v)
    a, b = a[None, :, None], b[:, None, None]
    ia, ib = F(1) - a, F(1) - b
    t00, t10 = tex[j0][:, i0], tex[j0][:, i1]
    t01, t11 = tex[j1][:, i0], tex[j1][:, i1]
    with np.errstate(invalid="ignore", over="ignore"):
        return (t00 * ia + t10 * a) * ib + (t01 * ia + t11 * a) * b


def nearest(tex, u, v):
    h, w = tex.shape[:2]
    i = np.clip(np.floor(u * F(w)).astype(np.int64), 0, w - 1)
    j = np.clip(np.floor(v * F(h)).astype(np.int64), 0, h - 1)
    return tex[j][:, i]


def is_nan(v):
    """utils.wgsl:3-5"""
    with np.errstate(invalid="ignore"):
        return ~((v < 0) | (0 < v) | (v == 0))


def srgb_encode(c):
    """IEC 61966-2-1, float64"""
    c = c.astype(np.float64)
    return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 1e-300), 1.0 / 2.4) - 0.055)


def unorm(c):
    c = np.where(np.isnan(c), F(0), c)
    return np.clip(c, F(0), F(1))


def overlay(input, albedo, vw, vh, fmt, mutate=None):
    """The viewport's texels, (vh, vw, 4): uint8 for the 8-bit formats (in memory order: BGRA swapped), uint16 f16 bits
    for RGBA16F.  input, albedo: (h, w, 4) float32 (decoded RGBA16F)."""
    px = (np.arange(vw, dtype=F) + F(0.5)) / F(vw) * F(2) - F(1)           # position.x at the pixel centres
    py = F(1) - (np.arange(vh, dtype=F) + F(0.5)) / F(vh) * F(2)           # position.y: up
    u = (px + F(1)) * F(0.5)
    v = (py + F(1)) * F(0.5)
    if mutate != "y_not_flipped":
        v = F(1) - v
    alb = nearest(albedo, u, v) if mutate == "albedo_nearest" else linear(albedo, u, v)
    col = linear(input, u, v)
    bad = is_nan(col[..., :3] if mutate == "nan_rgb_only" else col).any(axis=-1)
    col = np.where(bad[..., None], alb, col).astype(F)
    if fmt == RGBA16F:
        with np.errstate(all="ignore"):
            rgb = col[..., :3]
            lum = (rgb[..., 0] * F(0.2126) + rgb[..., 1] * F(0.7152)) + rgb[..., 2] * F(0.0722)
            l_old = lum if mutate == "no_clamp" else np.fmin(np.fmax(lum, F(0.0005)), F(0.995))
            l_new = l_old / ((F(1) + l_old) if mutate == "l_plus" else (F(1) - l_old))
            rgb = rgb * (l_new / lum)[..., None]
            out = np.concatenate([rgb, col[..., 3:]], axis=-1).astype(F)
            return out.astype(np.float16).view(np.uint16)
    c = unorm(col)
    code = np.floor(255.0 * srgb_encode(c[..., :3]) + 0.5)
    alpha = np.floor(255.0 * srgb_encode(c[..., 3:]) + 0.5) if mutate == "srgb_alpha" else \
        np.floor(c[..., 3:] * F(255) + F(0.5))
    out = np.concatenate([code, alpha], axis=-1).astype(np.uint8)
    if fmt == BGRA8_SRGB:
        out = out[..., [2, 1, 0, 3]]
    return np.ascontiguousarray(out)
