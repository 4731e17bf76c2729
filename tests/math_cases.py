"""The inputs of the scalar-function comparison, device against host (hk_selftest_math / hko_math_array), per function
id of enum hk_math_fn: deterministic, pure numpy, no GPU.  tests/test_math_cases.py shows that each set holds what
this text says; tests/test_gpu_math.py and tools/math_sweep.py run them.

Every set is the union of
  * the sweep: every 251st of the 2^32 bit patterns (about 2^24 words: both signs, every exponent, subnormals, NaN
    payloads, infinities); the second operand of a two-operand id is a sweep of another odd stride and offset that
    wraps many times, so the two operands' exponents and signs are unrelated;
  * a window of +-64 bit patterns (so nextafter on each side is in it) around every edge the function selects on, with
    both signs: 0, the smallest subnormal, 0x1p-126, FLT_MAX, inf, and the function's own edges (see `cases`);
  * the whole domain where it is small: all unorm16 / unorm8 codes, the 256 snorm8 codes in each byte lane, all f16
    codes in each half of a word whose other half is the bitwise complement (a decode of the wrong half differs).
Words are uint32: f32 bit patterns, or codes where the function takes one.
"""
from __future__ import annotations

import numpy as np

f32, u32 = np.float32, np.uint32

SWEEP_STRIDE = 251
SWEEP_STRIDE_B, SWEEP_OFFSET_B = 2654435761, 0x9E3779B9  # odd: coprime to 2^32 (and to 251)
WINDOW = 64
SIGN = 0x80000000
INV_LN2 = f32(1.4426950408889634)  # hk_exp's factor
DIV_BY_DIVISORS = (1, 3, 7, 47, 63, 1080, 1920, 2160, 3840, 4352)
QNAN, SNAN = 0x7FC00000, 0x7FA00000
MINMAX_SPECIALS = (QNAN, SNAN, 0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000)


def fb(x) -> np.ndarray:
    """f32 values -> their bit patterns."""
    return np.atleast_1d(np.asarray(x, f32)).view(u32)


def bf(u) -> np.ndarray:
    """bit patterns -> f32 values."""
    return np.ascontiguousarray(u, u32).view(f32)


def sweep() -> np.ndarray:
    return np.arange(0, 1 << 32, SWEEP_STRIDE, dtype=np.uint64).astype(u32)


def sweep_b(n: int) -> np.ndarray:
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(SWEEP_STRIDE_B) + np.uint64(SWEEP_OFFSET_B)) & np.uint64(0xFFFFFFFF)).astype(u32)


def window(centres, radius: int = WINDOW) -> np.ndarray:
    """The bit patterns c - radius .. c + radius of every centre c (wrapping at 2^32)."""
    c = np.atleast_1d(np.asarray(centres, u32)).astype(np.int64)
    w = (c[:, None] + np.arange(-radius, radius + 1, dtype=np.int64)[None, :]) & 0xFFFFFFFF
    return w.ravel().astype(u32)


def both(u) -> np.ndarray:
    u = np.atleast_1d(np.asarray(u, u32))
    return np.concatenate([u, u ^ u32(SIGN)])


def edge(values) -> np.ndarray:
    """Windows around f32 values and around their negations."""
    return window(both(fb(values)))


COMMON_EDGES = (0.0, 1e-45, 2.0 ** -126, 3.4028234663852886e38, np.inf)


def common() -> np.ndarray:
    return edge(COMMON_EDGES)


# ------------------------------------------------------------------ the functions' own edges
EXP2_EDGES = (-151.0, -150.0, -149.0, -126.0, -125.0, 127.0, 128.0)


def exp2_points() -> np.ndarray:
    """hk_exp2's selects and rounding ties as f32 values: the listed edges and n + 0.5 for n in -152..129."""
    ties = np.arange(-152, 130, dtype=np.float64) + 0.5
    return np.concatenate([np.array(EXP2_EDGES), ties]).astype(f32)


def exp2_subnormal_args() -> np.ndarray:
    """Arguments whose 2^x is subnormal (-151 .. -126), every 7th bit pattern."""
    lo, hi = int(fb(-126.0)[0]), int(fb(-151.0)[0])
    return np.arange(lo, hi + 1, 7, dtype=np.uint64).astype(u32)


def exp_subnormal_args() -> np.ndarray:
    """The same range divided by hk_exp's factor (f32 division), every 7th bit pattern."""
    lo, hi = int(fb(f32(-126.0) / INV_LN2)[0]), int(fb(f32(-151.0) / INV_LN2)[0])
    return np.arange(lo, hi + 1, 7, dtype=np.uint64).astype(u32)


def log2_big_switch() -> np.ndarray:
    """m = 1.41421356f (the `big` switch) in every 8th binade."""
    man = int(fb(1.41421356)[0]) & 0x007FFFFF
    return np.array([(e << 23) | man for e in range(1, 255, 8)], u32)


def sincos_quadrant_switches() -> np.ndarray:
    """Odd multiples of pi/4 up to 2^16: where rintf(x * 2/pi) changes."""
    k = np.arange(1, int(65536 / (np.pi / 4)) + 1, 2, dtype=np.float64)
    return (k * (np.pi / 4)).astype(f32)


SINCOS_Q_CLAMP = 2147483520.0  # hk_sincos clamps k here before the conversion
SINCOS_LARGE = (2147483520.0 * (np.pi / 2), 2147483648.0 * (np.pi / 2), 4294967296.0 * (np.pi / 2), 4e9, 1e10, 1e20,
                1e30)


def pow_int_thresholds() -> np.ndarray:
    """x at which x^2, x^4, x^5, x^8, x^16 (hk_pow2 / 5 / 16 and their intermediate products) reach FLT_MAX's binade
    end, the smallest normal, the smallest subnormal and half of it."""
    t = [2.0 ** (e / n) for n in (2, 4, 5, 8, 16) for e in (128.0, -126.0, -149.0, -150.0)]
    return np.array(t, np.float64).astype(f32)


def unorm16_ties() -> np.ndarray:
    """x with x * 65535 next to c + 0.5 for every code c."""
    return ((np.arange(65535, dtype=np.float64) + 0.5) / 65535.0).astype(f32)


def snorm8_ties() -> np.ndarray:
    return ((np.arange(-127, 127, dtype=np.float64) + 0.5) / 127.0).astype(f32)


CONVERSION_EDGES = (2147483648.0, 4294967296.0)  # each +-1 ulp and negated through the windows
ROUNDING_EDGES = (0.5, 1.0, 8388608.0, 16777216.0)  # floorf / clamp edges of fract, saturate, signf
RCP_EDGES = (2.0 ** -125, 2.0 ** 125, 2.0 ** -126, 2.0 ** 126, 2.0 ** 127)  # rcp_fast_ok's bounds; subnormal quotients


def snorm8_lanes():
    """(word, lane): the 256 codes in each byte lane, the other lanes holding the code's complement."""
    code = np.arange(256, dtype=u32)
    inv = (~code) & u32(0xFF)
    words, lanes = [], []
    for lane in range(4):
        fill = inv | (inv << u32(8)) | (inv << u32(16)) | (inv << u32(24))
        mask = u32(0xFF) << u32(8 * lane)
        words.append((fill & ~mask) | (code << u32(8 * lane)))
        lanes.append(np.full(256, lane, u32))
    return np.concatenate(words), np.concatenate(lanes)


def f16_words() -> np.ndarray:
    """Every f16 code in the low half with its complement in the high half, then the same in the high half."""
    code = np.arange(65536, dtype=u32)
    inv = (~code) & u32(0xFFFF)
    return np.concatenate([code | (inv << u32(16)), (code << u32(16)) | inv])


def product(a, b):
    a, b = np.atleast_1d(np.asarray(a, u32)), np.atleast_1d(np.asarray(b, u32))
    return np.repeat(a, len(b)), np.tile(b, len(a))


def cycle(values, n: int) -> np.ndarray:
    v = np.atleast_1d(np.asarray(values, u32))
    return v[np.arange(n) % len(v)]


PAIR_SPECIALS = both(fb([0.0, 1e-45, 2.0 ** -126, 2.0 ** -125, 0.5, 1.0, 2.0, 3.0, 5.0, 16.0, 2.0 ** 125,
                         3.4028234663852886e38, np.inf])).tolist() + [QNAN, SNAN]


def _pairs(name: str):
    """(a, b) chunks of a two-operand id besides the sweep."""
    sp = np.array(PAIR_SPECIALS, u32)
    chunks = [product(sp, sp)]
    w = common()
    if name in ("minf", "maxf"):
        chunks.append(product(MINMAX_SPECIALS, MINMAX_SPECIALS))
        chunks.append((w, cycle(sp, len(w))))
        chunks.append((cycle(sp, len(w)), w))
    elif name == "div":
        w = np.concatenate([w, edge(RCP_EDGES)])
        chunks.append((w, cycle(sp, len(w))))
        chunks.append((cycle(sp, len(w)), w))
        # subnormal quotients next to the smallest normal: a around 0x1p-125 and 0x1p-126 over small integers
        small = edge([2.0 ** -125, 2.0 ** -126, 2.0 ** -120])
        for d in (2.0, 3.0, 7.0, 1080.0):
            chunks.append((small, cycle(fb(d), len(small))))
    elif name == "pow":
        # the bases at which x^n leaves the normal range, with the kernels' literal exponents as y
        t = np.concatenate([w, edge(pow_int_thresholds()), edge([1.0, 2.0, 0.5])])
        chunks.append((t, cycle(fb([2.0, 5.0, 16.0, 0.5, -1.0, 1.0 / 2.2, 2.4]), len(t))))
        # y * log2(x) on hk_exp2's edges: base 2 and 0.5 with y on them
        y = np.concatenate([window(fb(exp2_points())), exp2_subnormal_args()])
        chunks.append((cycle(fb([2.0, 0.5]), len(y)), y))
    return chunks


def _div_by():
    s = sweep()
    mag = np.abs(bf(s))
    with np.errstate(invalid="ignore"):
        s = s[(mag >= f32(2.0 ** -100)) & (mag < f32(2.0 ** 100))]  # the domain the kernels claim
    x = np.concatenate([s, window(both(fb(0.0)))])
    d = fb(np.array(DIV_BY_DIVISORS, f32))
    return np.tile(x, len(d)), np.repeat(d, len(x))


def cases(name: str):
    """(a, b) for function `name` (hikari_amd._abi.MATH_FN_NAMES); b is None for the one-operand ids."""
    if name == "div_by":
        return _div_by()
    if name == "unpack_snorm8_fast":
        s = sweep()
        words, lanes = snorm8_lanes()
        return np.concatenate([s, words]), np.concatenate([sweep_b(len(s)), lanes])
    if name in ("pow", "minf", "maxf", "div"):
        s = sweep()
        a, b = [s], [sweep_b(len(s))]
        for ca, cb in _pairs(name):
            a.append(ca)
            b.append(cb)
        return np.concatenate(a), np.concatenate(b)
    parts = [sweep(), common()]
    if name == "exp2":
        parts += [window(fb(exp2_points())), exp2_subnormal_args()]
    elif name in ("exp", "exp_weight"):
        images = exp2_points() / INV_LN2
        parts += [window(fb(images)), exp_subnormal_args(), window(fb(f32(-160.0) / f32(1.4427)))]
    elif name == "log2":
        parts += [np.arange(1, 0x00800000, 7, dtype=u32), edge(bf(log2_big_switch())), edge(1.0)]
    elif name == "sincos":
        parts += [edge(sincos_quadrant_switches()), edge(np.array(SINCOS_LARGE).astype(f32)),
                  edge(bf(np.array([0x00000100, 0x00400000, 0x007FFFFF], u32)))]
    elif name in ("pow2", "pow5", "pow16"):
        parts += [edge(pow_int_thresholds()), edge(1.0)]
    elif name in ("f2u32", "f2i32"):
        parts += [edge(CONVERSION_EDGES), edge(ROUNDING_EDGES)]
    elif name == "unorm16":
        parts += [edge(unorm16_ties()), edge(ROUNDING_EDGES), edge(CONVERSION_EDGES)]
    elif name == "snorm8":
        parts += [edge(snorm8_ties()), edge(ROUNDING_EDGES), edge(CONVERSION_EDGES)]
    elif name == "unpack_unorm16_fast":
        parts += [np.arange(65536, dtype=u32)]
    elif name == "unorm8_fast":
        parts += [np.arange(256, dtype=u32)]
    elif name == "random_float":
        parts += [window(np.array([0xFFFFFFFF, 0x80000000], u32))]
    elif name in ("fract", "saturate", "signf"):
        parts += [edge(ROUNDING_EDGES)]
    elif name in ("sqrt", "rcp_exact", "rcp_fast"):
        parts += [edge(RCP_EDGES), edge(1.0)]
    elif name == "unpack_f16":
        parts += [f16_words()]
    else:
        raise KeyError(name)
    a = np.concatenate(parts)
    if name == "exp_weight":
        a = a[exp_weight_defined(a)]
    return a, None


def exp_weight_defined(a: np.ndarray) -> np.ndarray:
    """hk_exp_weight converts rintf(max(x * INV_LN2, -160)) to int32 without an upper clamp: its arguments are <= 0 or
    NaN (denoise.wgsl's -|a| / b).  From x * INV_LN2 >= 2^31 on the conversion is undefined in C (x86 gives INT_MIN,
    gfx950 saturates), so neither side is a reference there; those inputs, and only those, are left out (every
    argument of the function's domain, and the positive ones below that bound, stay)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return ~(bf(a) * INV_LN2 >= f32(2147483648.0))
