"""Independent float32 restatement of the material texture sampler, in vectorised numpy.

Written from light.wgsl:748-794 (`textureSampleLevel(textures[id], samplers[id], uv, 0.0)`), the WebGPU
address modes (GPUAddressMode: clamp-to-edge, repeat, mirror-repeat) and the definition in the comment at
the head of include/hk_texture.h; it neither includes nor loads that header's code.

  nearest : i = floor(u*W), j = floor(v*H)
  linear  : x = u*W - 0.5, i0 = floor(x), a = x - floor(x) (same for y),
            result = (t00*(1-a) + t10*a)*(1-b) + (t01*(1-a) + t11*a)*b,
            every operation rounded to f32, in that order
  float -> int saturates to the int32 range, NaN -> 0; the second tap i0 + 1 does not wrap past INT_MAX
  address modes act on the integer texel coordinate
  a texel's four bytes decode through a 256-entry table per format; alpha uses the unorm table in sRGB images

The decode table is an argument (`lut[format][byte]`): the sRGB half is the build's own transcendental, so
the tests read it from the side under test through a 256x1 nearest ramp and check it separately
(`decode_reference`).  `misread` selects one deliberate misreading of the definition; the tests show that each
of them is caught.
"""
import numpy as np

SRGB, UNORM = 0, 1
CLAMP, REPEAT, MIRROR = 0, 1, 2
NEAREST, LINEAR = 0, 1
INT_MAX, INT_MIN = 2147483647, -2147483648

MISREADINGS = ("no_half", "round", "mirror_no_edge", "c_remainder", "swap_weights", "srgb_alpha", "transposed")

f32 = np.float32


def decode_reference(byte, srgb):
    """float64 statement of the texel decode: unorm byte/255, sRGB by the piecewise IEC 61966-2-1 curve."""
    c = np.asarray(byte, np.float64) / 255.0
    if not srgb:
        return c
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def reference_lut():
    """(2, 256) f32 table from decode_reference (the tests sample with the table of the side under test)."""
    b = np.arange(256)
    return np.stack([decode_reference(b, True), decode_reference(b, False)]).astype(f32)


def ulp_distance(a, b):
    """Distance in f32 units in the last place between two arrays of finite non-negative f32."""
    return np.abs(np.asarray(a, f32).view(np.int32).astype(np.int64) - np.asarray(b, f32).view(np.int32).astype(np.int64))


def to_int(x):
    """Saturating f32 -> int32 (held in int64), NaN -> 0."""
    x = np.asarray(x, f32)
    nan = np.isnan(x)
    hi = x >= f32(2147483648.0)
    lo = x <= f32(-2147483648.0)
    safe = np.where(nan | hi | lo, f32(0), x)
    i = np.trunc(safe).astype(np.int64)
    return np.where(hi, INT_MAX, np.where(lo, INT_MIN, i))


def address(i, n, mode, misread=None):
    """GPUAddressMode on integer texel coordinates i (int64) of an axis of n texels."""
    if mode == REPEAT:
        if misread == "c_remainder":  # C's %: the sign follows the dividend, so -1 -> texel 1 instead of n - 1
            return np.abs(np.fmod(i, n))
        return np.mod(i, n)
    if mode == MIRROR:
        if misread == "mirror_no_edge":  # ... 2 1 0 1 2 ... : period 2n - 2, the edge texel not repeated
            if n == 1:
                return np.zeros_like(i)
            r = np.mod(i, 2 * n - 2)
            return np.where(r < n, r, 2 * n - 2 - r)
        r = np.mod(i, 2 * n)  # 0 1 .. n-1 n-1 .. 1 0
        return np.where(r < n, r, 2 * n - 1 - r)
    return np.clip(i, 0, n - 1)


def fetch(texels, srgb, lut, x, y, misread=None):
    h, w = texels.shape[:2]
    flat = texels.reshape(-1, 4)
    t = flat[x * h + y] if misread == "transposed" else flat[y * w + x]
    colour = lut[SRGB if srgb else UNORM]
    alpha = colour if misread == "srgb_alpha" else lut[UNORM]
    return np.stack([colour[t[:, 0]], colour[t[:, 1]], colour[t[:, 2]], alpha[t[:, 3]]], axis=1)


def sample(texels, srgb, address_u, address_v, filt, uv, lut, misread=None):
    """textureSampleLevel(.., uv, 0) of an (H, W, 4) uint8 image at (n, 2) f32 uv -> (n, 4) f32."""
    assert misread is None or misread in MISREADINGS
    texels = np.ascontiguousarray(texels, np.uint8)
    lut = np.asarray(lut, f32).reshape(2, 256)
    h, w = texels.shape[:2]
    uv = np.asarray(uv, f32).reshape(-1, 2)
    u, v = uv[:, 0], uv[:, 1]
    floor = np.rint if misread == "round" else np.floor
    with np.errstate(all="ignore"):
        if filt == NEAREST:
            i = address(to_int(floor(u * f32(w))), w, address_u, misread)
            j = address(to_int(floor(v * f32(h))), h, address_v, misread)
            return fetch(texels, srgb, lut, i, j, misread)
        half = f32(0.0) if misread == "no_half" else f32(0.5)
        x, y = u * f32(w) - half, v * f32(h) - half
        x0, y0 = floor(x), floor(y)
        a, b = (x - x0)[:, None], (y - y0)[:, None]
        i0, j0 = to_int(x0), to_int(y0)
        i1, j1 = np.where(i0 == INT_MAX, i0, i0 + 1), np.where(j0 == INT_MAX, j0, j0 + 1)
        ia, ib = address(i0, w, address_u, misread), address(i1, w, address_u, misread)
        ja, jb = address(j0, h, address_v, misread), address(j1, h, address_v, misread)
        t00, t10 = fetch(texels, srgb, lut, ia, ja, misread), fetch(texels, srgb, lut, ib, ja, misread)
        t01, t11 = fetch(texels, srgb, lut, ia, jb, misread), fetch(texels, srgb, lut, ib, jb, misread)
        one = f32(1.0)
        ca, cb = one - a, one - b
        if misread == "swap_weights":
            a, ca = ca, a
        return ((t00 * ca + t10 * a) * cb + (t01 * ca + t11 * a) * b).astype(f32)


def same_words(a, b):
    """Every stored word equal, a NaN equal to a NaN."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------- the test inputs shared by the CPU and GPU comparison
SIZES = ((1, 1), (1, 7), (5, 1), (3, 5), (2, 2), (64, 64), (257, 3))  # (W, H)
COMBOS = tuple((fmt, au, av, fl) for fmt in (SRGB, UNORM) for au in range(3) for av in range(3) for fl in (NEAREST, LINEAR))

_DEN = np.float32(1e-45)  # the smallest denormal
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 0.5, _DEN, -_DEN, 1e6, -1e6, 3e9, -3e9, 2147483520.0, 2147483648.0,
                     -2147483648.0, -2147483904.0, 4e9, 1e30, -1e30, 3.4e38, np.inf, -np.inf, np.nan], np.float32)


def _with_neighbours(x):
    x = np.asarray(x, f32)
    return np.concatenate([np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))])


def seams(n):
    """k/n for k in [-2n-1, 3n+1], each with its two f32 neighbours."""
    k = np.arange(-2 * n - 1, 3 * n + 2)
    return _with_neighbours((k.astype(np.float64) / n).astype(f32))


def uv_set(w, h, seed=0):
    """The UV pairs of the sampler comparison for a W x H image."""
    su, sv = seams(w), seams(h)
    ku, kv = np.arange(len(su)), np.arange(len(sv))
    parts = [
        np.stack(np.meshgrid(SPECIALS, SPECIALS, indexing="ij"), axis=-1).reshape(-1, 2),
        # every u seam against a walk through the v seams, every v seam against a walk through the u seams, and every
        # seam against an interior coordinate of the other axis
        np.stack([su, sv[(ku * 7 + 3) % len(sv)]], axis=1),
        np.stack([su[(kv * 5 + 1) % len(su)], sv], axis=1),
        np.stack([su, np.full(len(su), 0.3, f32)], axis=1),
        np.stack([np.full(len(sv), -0.7, f32), sv], axis=1),
        # u*W and v*H exactly on the last f32 below 2^31 (converted, not saturated) and on -2^31, where W, H divide them
        np.array([[2147483520.0 / w, 0.3], [-0.7, 2147483520.0 / h], [-2147483648.0 / w, 0.3], [-0.7, -2147483648.0 / h],
                  [2147483520.0 / w, 2147483520.0 / h]], f32),
        # every texel centre
        np.stack(np.meshgrid(((np.arange(w) + 0.5) / w).astype(f32), ((np.arange(h) + 0.5) / h).astype(f32),
                             indexing="ij"), axis=-1).reshape(-1, 2),
        np.random.default_rng(seed).uniform(-2.5, 3.5, (6000, 2)).astype(f32),
    ]
    return np.ascontiguousarray(np.concatenate(parts).astype(f32))


def random_texels(w, h, seed):
    """(H, W, 4) uint8 with every channel varying, alpha included."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def ramp():
    """256x1 image whose texel k holds byte k in all four channels, and the uv of its texel centres."""
    t = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 4, axis=2)
    uv = np.stack([(np.arange(256) + 0.5) / 256, np.full(256, 0.5)], axis=1).astype(f32)
    return t, uv


def bank():
    """Every (size, combination) as one list of (texels, format, address_u, address_v, filter): uploaded together, so
    each texture sits at its own odd texel offset behind images of other sizes."""
    out = []
    for s, (w, h) in enumerate(SIZES):
        for c, (fmt, au, av, fl) in enumerate(COMBOS):
            out.append((random_texels(w, h, 1000 * s + c), fmt, au, av, fl))
    return out


def bank_textures():
    from hikari_amd import Texture
    return [Texture(t, srgb=fmt == SRGB, address_u=au, address_v=av, filter=fl) for t, fmt, au, av, fl in bank()]


def read_lut(sample_fn):
    """The (2, 256) decode table of a sampler, read through the nearest ramp; sample_fn(srgb, texels, uv) -> (n, 4).
    Alpha of the sRGB read must already be the unorm table (checked by the caller)."""
    t, uv = ramp()
    return np.stack([sample_fn(True, t, uv)[:, 0], sample_fn(False, t, uv)[:, 0]]).astype(f32)
