"""tests/math_cases.py holds what it says (no GPU): per function id, every special-case branch of the function is taken
by at least one input — found by classifying the inputs here in numpy, not by trusting the lists — NaN and non-NaN
results both occur where the function has them, subnormal results occur where the function can give them, and
hko_math_array agrees with the oracle's scalar entry points.  A later edit of the cases cannot hollow them out
unnoticed.

(sqrtf has no subnormal result: the root of the smallest subnormal is 2^-74.5.  Its set is held to subnormal inputs,
whose roots the hardware's sqrt sequence has to scale, and to the negative, zero and infinite ones.)"""
import re
from pathlib import Path

import numpy as np
import pytest

import math_cases as mc

f32, u32 = np.float32, np.uint32
ROOT = Path(__file__).resolve().parent.parent
INF, TINY = f32(np.inf), f32(2.0 ** -126)


def names():
    from hikari_amd import _abi
    return _abi.MATH_FN_NAMES


def pytest_generate_tests(metafunc):
    if "fn_name" in metafunc.fixturenames:
        metafunc.parametrize("fn_name", names())


def test_function_ids_are_the_headers_enum():
    from hikari_amd import _abi
    text = (ROOT / "include" / "hikari_amd.h").read_text()
    body = re.search(r"enum hk_math_fn \{(.*?)\};", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ids = re.findall(r"\bHK_MATH_(\w+)", body)
    assert ids[-1] == "COUNT" and "= 0" in body.split(",")[0] and body.count("=") == 1
    assert tuple(i.lower() for i in ids[:-1]) == _abi.MATH_FN_NAMES
    assert set(_abi.MATH_FN_TWO_OPERANDS) | set(_abi.MATH_FN_TWO_RESULTS) <= set(_abi.MATH_FN_NAMES)


def is_nan(x):
    return np.isnan(x)


def subnormal(x):
    return (np.abs(x) > 0) & (np.abs(x) < TINY)


def has_bits(a, *patterns):
    return all(np.any(a == u32(p)) for p in patterns)


def exp2_classes(y, exact=True):
    """hk_exp2's selects on its argument y.  hk_exp's argument is a rounded product, which steps over some floats: there
    (exact False) the two sides of a select are the floats within 4 ulp of it, not the neighbours themselves."""
    n = np.rint(y)

    def sides(edge):
        e = f32(edge)
        if exact:
            return y == e, y == np.nextafter(e, -INF)
        ulp = np.spacing(np.abs(e))
        return (y >= e) & (y <= e + 4 * ulp), (y < e) & (y >= e - 4 * ulp)

    at128, below128 = sides(128)
    at151, below151 = sides(-151)
    at126, below126 = sides(-126)
    return {
        "nan": is_nan(y), "overflow": y >= 128, "at 128": at128, "just below 128": below128,
        "zero": y < -151, "at -151": at151, "just below -151": below151, "at -126": at126, "just below -126": below126,
        "normal": (n >= -126) & (y < 128), "n = -126": n == -126, "n = -127": n == -127,
        "subnormal": (n < -126) & (y >= -151), "tie up": y - n == 0.5, "tie down": y - n == -0.5,
        "+inf": y == INF, "-inf": y == -INF,
    }


def classes(name, a, b):
    """{branch: mask over the inputs} for every branch and edge the function selects on."""
    x = mc.bf(a)
    y = None if b is None else mc.bf(b)
    with np.errstate(all="ignore"):
        if name == "exp2":
            return exp2_classes(x)
        if name == "exp":
            return exp2_classes(x * mc.INV_LN2, exact=False)
        if name == "exp_weight":
            t = x * mc.INV_LN2
            n = np.rint(np.where(is_nan(t) | (t < -160), f32(-160), t))
            return {"nan": is_nan(x), "clamped at -160": t < -160, "flushed": n <= -127, "n = -127": n == -127,
                    "n = -126": n == -126, "normal": n >= -126, "zero argument": x == 0, "positive": x > 0,
                    "the domain": x <= 0}
        if name == "log2":
            man = mc.bf((a & u32(0x007FFFFF)) | u32(0x3F800000))
            big = man > f32(1.41421356)
            pos = (x > 0) & (x < INF)
            return {"nan": is_nan(x), "negative": x < 0, "+0": a == 0, "-0": a == u32(mc.SIGN), "+inf": x == INF,
                    "subnormal": pos & (x < TINY), "smallest normal": x == TINY, "big": pos & big, "not big": pos & ~big,
                    "at the big switch": pos & (man == f32(1.41421356)),
                    "just above the big switch": pos & (man == np.nextafter(f32(1.41421356), f32(2))), "one": x == 1}
        if name == "sincos":
            k = np.rint(x * f32(0.63661977236758134))
            fin = np.isfinite(x)
            kc = np.clip(np.where(fin, k, 0), -mc.SINCOS_Q_CLAMP, mc.SINCOS_Q_CLAMP).astype(np.int64) & 3
            out = {"nan": is_nan(x), "+inf": x == INF, "-inf": x == -INF, "subnormal": subnormal(x),
                   "k clamped above": fin & (k > mc.SINCOS_Q_CLAMP), "k clamped below": fin & (k < -mc.SINCOS_Q_CLAMP),
                   "k at the clamp": fin & (np.abs(k) == mc.SINCOS_Q_CLAMP), "k = 0": fin & (k == 0),
                   "k beyond 2^16 / (pi/2)": fin & (np.abs(k) > 41721)}
            for q in range(4):
                out[f"quadrant {q}"] = fin & (kc == q)
                out[f"quadrant {q}, x < 0"] = fin & (kc == q) & (x < 0)
            return out
        if name in ("pow2", "pow5", "pow16"):
            p = {"pow2": 2, "pow5": 5, "pow16": 16}[name]
            r = x.astype(np.float64) ** p
            ok = x >= 0
            return {"nan": is_nan(x), "negative": x < 0, "-0": a == u32(mc.SIGN), "+0": a == 0, "+inf": x == INF,
                    "overflows": ok & (x < INF) & (r > 3.4028235677973366e38), "underflows to 0": (x > 0) & (r < 2.0 ** -150),
                    "subnormal result": (x > 0) & (r < 2.0 ** -126) & (r > 2.0 ** -149), "normal": ok & (r >= 2.0 ** -126) &
                    (r < 3.4e38), "subnormal input": subnormal(x) & ok}
        if name == "pow":
            return {"nan base": is_nan(x), "nan exponent": is_nan(y), "negative base": x < 0, "zero base": x == 0,
                    "-0 base": a == u32(mc.SIGN), "inf base": x == INF, "base one": x == 1, "subnormal base": subnormal(x) & (x > 0),
                    "exponent 2": y == 2, "exponent 5": y == 5, "exponent 16": y == 16, "zero exponent": y == 0,
                    "negative exponent": y < 0, "inf exponent": np.isinf(y), "base 2, subnormal result": (x == 2) & (y < -126) &
                    (y > -149), "base 2, exponent 128": (x == 2) & (y == 128)}
        if name in ("unorm16", "snorm8"):
            scale, lo = (f32(65535), f32(0)) if name == "unorm16" else (f32(127), f32(-1))
            t = np.clip(x, lo, f32(1)) * scale
            out = {"nan": is_nan(x), "clamped low": x < lo, "clamped high": x > 1, "at the low bound": x == lo, "one": x == 1,
                   "-0": a == u32(mc.SIGN), "inside": (x > lo) & (x < 1), "-inf": x == -INF, "+inf": x == INF,
                   "tie to even, up": (t - np.floor(t) == 0.5) & (np.floor(t) % 2 == 1),
                   "tie to even, down": (t - np.floor(t) == 0.5) & (np.floor(t) % 2 == 0)}
            return out
        if name == "unpack_unorm16_fast":
            return {"high half set": (a >> u32(16)) != 0, "code 0": (a & u32(0xFFFF)) == 0, "code 65535": (a & u32(0xFFFF)) == 0xFFFF}
        if name == "unpack_snorm8_fast":
            byte = (a >> (u32(8) * (b & u32(3)))) & u32(0xFF)
            out = {"-128 (clamped to -1)": byte == 0x80, "-127": byte == 0x81, "127": byte == 0x7F, "0": byte == 0,
                   "lane index above 3": b > 3}
            for lane in range(4):
                out[f"lane {lane}"] = (b & u32(3)) == lane
            return out
        if name == "unorm8_fast":
            return {"upper bytes set": (a >> u32(8)) != 0, "code 0": (a & u32(0xFF)) == 0, "code 255": (a & u32(0xFF)) == 0xFF}
        if name == "random_float":
            return {"0": a == 0, "all ones": a == 0xFFFFFFFF, "sign bit": a == u32(mc.SIGN)}
        if name == "fract":
            return {"nan": is_nan(x), "inf": np.isinf(x), "negative fraction": (x < 0) & (x != np.floor(x)), "-0": a == u32(mc.SIGN),
                    "tiny negative (result rounds to 1)": (x < 0) & (x > -f32(2.0 ** -25)), "integer": np.isfinite(x) & (x == np.floor(x)),
                    "beyond 2^23": np.isfinite(x) & (np.abs(x) >= 8388608), "positive fraction": (x > 0) & (x != np.floor(x))}
        if name in ("minf", "maxf"):
            qa, qb = is_nan(x) & ((a & u32(0x00400000)) != 0), is_nan(y) & ((b & u32(0x00400000)) != 0)
            return {"quiet nan, number": qa & ~is_nan(y), "number, quiet nan": ~is_nan(x) & qb,
                    "signalling nan, number": is_nan(x) & ~qa & ~is_nan(y), "number, signalling nan": ~is_nan(x) & is_nan(y) & ~qb,
                    "both nan": is_nan(x) & is_nan(y), "+0, -0": (a == 0) & (b == u32(mc.SIGN)), "-0, +0": (a == u32(mc.SIGN)) & (b == 0),
                    "a < b": x < y, "a > b": x > y, "equal": (x == y) & (a == b), "inf, -inf": (x == INF) & (y == -INF),
                    "subnormal operands": subnormal(x) & subnormal(y)}
        if name == "saturate":
            return {"quiet nan": is_nan(x) & ((a & u32(0x00400000)) != 0), "signalling nan": is_nan(x) & ((a & u32(0x00400000)) == 0),
                    "below 0": x < 0, "above 1": x > 1, "inside": (x > 0) & (x < 1), "-0": a == u32(mc.SIGN), "+0": a == 0,
                    "one": x == 1, "subnormal": subnormal(x), "inf": np.isinf(x)}
        if name == "signf":
            return {"nan": is_nan(x), "positive": x > 0, "negative": x < 0, "+0": a == 0, "-0": a == u32(mc.SIGN),
                    "subnormal": subnormal(x), "inf": np.isinf(x)}
        if name == "div":
            q = x.astype(np.float64) / y.astype(np.float64)
            return {"nan operand": is_nan(x) | is_nan(y), "0 / 0": (x == 0) & (y == 0), "inf / inf": np.isinf(x) & np.isinf(y),
                    "x / 0": (x != 0) & ~is_nan(x) & (y == 0), "x / inf": np.isfinite(x) & np.isinf(y),
                    "subnormal quotient": (np.abs(q) < 2.0 ** -126) & (np.abs(q) > 2.0 ** -149),
                    "quotient underflows": (q != 0) & (np.abs(q) < 2.0 ** -150), "quotient overflows": np.isfinite(q) & (np.abs(q) > 3.5e38),
                    "subnormal divisor": subnormal(y), "subnormal dividend": subnormal(x), "divisor beyond 2^126": np.isfinite(y) &
                    (np.abs(y) > f32(2.0 ** 126)), "negative quotient": q < 0}
        if name == "sqrt":
            return {"nan": is_nan(x), "negative": x < 0, "-0": a == u32(mc.SIGN), "+0": a == 0, "+inf": x == INF, "-inf": x == -INF,
                    "subnormal input": subnormal(x) & (x > 0), "smallest subnormal": a == 1, "FLT_MAX": a == 0x7F7FFFFF,
                    "normal": (x >= TINY) & (x < INF)}
        if name in ("rcp_exact", "rcp_fast"):
            m = np.abs(x)
            ok = (m >= f32(2.0 ** -125)) & (m <= f32(2.0 ** 125))
            return {"nan": is_nan(x), "fast path": ok, "divide path, small": ~is_nan(x) & (m < f32(2.0 ** -125)),
                    "divide path, large": (m > f32(2.0 ** 125)), "at 2^-125": m == f32(2.0 ** -125), "at 2^125": m == f32(2.0 ** 125),
                    "just below 2^-125": m == np.nextafter(f32(2.0 ** -125), f32(0)), "just above 2^125": m == np.nextafter(f32(2.0 ** 125), INF),
                    "+0": a == 0, "-0": a == u32(mc.SIGN), "inf": np.isinf(x), "subnormal quotient": np.isfinite(x) & (m > f32(2.0 ** 126)),
                    "subnormal input": subnormal(x), "negative": x < 0}
        if name == "div_by":
            out = {"+0": a == 0, "-0": a == u32(mc.SIGN), "subnormal": subnormal(x), "negative": x < 0,
                   "smallest of the domain": np.abs(x) < f32(2.0 ** -99.9), "largest of the domain": np.abs(x) > f32(2.0 ** 99.9)}
            for d in mc.DIV_BY_DIVISORS:
                out[f"divisor {d}"] = y == d
            return out
        if name == "f2u32":
            return {"nan": is_nan(x), "not above 0": x <= 0, "-0": a == u32(mc.SIGN), "saturates": x >= 4294967296.0,
                    "exactly 2^32": x == 4294967296.0, "just below 2^32": x == np.nextafter(f32(4294967296.0), f32(0)),
                    "exactly 2^31": x == 2147483648.0, "inside": (x > 0) & (x < 4294967296.0), "fraction truncated": (x > 0) & (x < 8388608) &
                    (x != np.floor(x)), "below 1": (x > 0) & (x < 1), "+inf": x == INF, "-inf": x == -INF}
        if name == "f2i32":
            return {"nan": is_nan(x), "saturates high": x >= 2147483648.0, "saturates low": x <= -2147483648.0,
                    "exactly 2^31": x == 2147483648.0, "just below 2^31": x == np.nextafter(f32(2147483648.0), f32(0)),
                    "exactly -2^31": x == -2147483648.0, "just below -2^31": x == np.nextafter(f32(-2147483648.0), -INF),
                    "just above -2^31": x == np.nextafter(f32(-2147483648.0), f32(0)), "-0": a == u32(mc.SIGN),
                    "negative fraction truncated": (x < 0) & (x > -8388608) & (x != np.floor(x)), "positive fraction truncated":
                    (x > 0) & (x < 8388608) & (x != np.floor(x)), "+inf": x == INF, "-inf": x == -INF}
        if name == "unpack_f16":
            lo, hi = a & u32(0xFFFF), a >> u32(16)
            out = {}
            for half, h in (("low", lo), ("high", hi)):
                ex, man = (h >> u32(10)) & u32(0x1F), h & u32(0x3FF)
                out.update({f"{half}: subnormal": (ex == 0) & (man != 0), f"{half}: zero": (h & u32(0x7FFF)) == 0, f"{half}: inf": (ex == 31) &
                            (man == 0), f"{half}: quiet nan": (ex == 31) & (man >= 0x200), f"{half}: signalling nan": (ex == 31) & (man != 0) &
                            (man < 0x200), f"{half}: normal": (ex > 0) & (ex < 31), f"{half}: negative": (h & u32(0x8000)) != 0})
            out["halves are complements"] = (lo ^ hi) == 0xFFFF
            return out
    raise KeyError(name)


# ids whose results include NaNs, and those that give subnormal results (sqrtf: see the module text)
NAN_RESULTS = ("exp2", "exp", "log2", "pow", "pow2", "pow5", "pow16", "sincos", "fract", "minf", "maxf", "div", "sqrt",
               "rcp_exact", "rcp_fast", "unpack_f16")
SUBNORMAL_RESULTS = ("exp2", "exp", "div", "rcp_exact", "rcp_fast", "pow", "pow2", "pow5", "pow16", "div_by")


def test_every_branch_of_the_function_is_taken(fn_name):
    import oracle
    a, b = mc.cases(fn_name)
    assert a.dtype == u32 and (b is None or (b.dtype == u32 and b.shape == a.shape))
    from hikari_amd import _abi
    assert (b is not None) == (fn_name in _abi.MATH_FN_TWO_OPERANDS)
    empty = [k for k, m in classes(fn_name, a, b).items() if not np.any(m)]
    assert not empty, f"{fn_name}: no input for {empty}"
    # the sweep is whole: every exponent with both signs (and so NaN payloads, infinities and subnormals)
    s = mc.sweep()
    assert len(s) == -(-(1 << 32) // mc.SWEEP_STRIDE) and len(np.unique(s >> u32(23))) == 512
    if fn_name != "div_by" and fn_name != "exp_weight":
        assert np.array_equal(a[:len(s)], s)
    if b is not None and fn_name != "div_by":
        assert len(np.unique(b[:len(s)] >> u32(23))) == 512 and len(np.unique((a[:len(s)] ^ b[:len(s)]) >> u32(31))) == 2
    out = oracle.math_array(fn_name, a, b)
    for r in (out if isinstance(out, tuple) else (out,)):
        v = r.view(f32)
        if fn_name in NAN_RESULTS:
            assert np.isnan(v).any() and not np.isnan(v).all()
        if fn_name in SUBNORMAL_RESULTS:
            assert subnormal(v).any(), f"{fn_name}: no subnormal result"
    if fn_name in ("saturate", "signf", "exp_weight", "unpack_unorm16_fast", "unpack_snorm8_fast", "unorm8_fast", "random_float",
                   "div_by"):
        assert fn_name == "div_by" or not np.isnan(out.view(f32)).any()  # NaN-free by construction of the function


def test_small_domains_are_whole():
    a, _ = mc.cases("unpack_unorm16_fast")
    assert len(np.unique(a[-65536:])) == 65536 and a[-65536:].max() == 65535
    a, _ = mc.cases("unorm8_fast")
    assert np.array_equal(a[-256:], np.arange(256, dtype=u32))
    a, b = mc.cases("unpack_snorm8_fast")
    words, lanes = a[-1024:], b[-1024:]
    for lane in range(4):
        sel = lanes == lane
        assert sel.sum() == 256 and np.array_equal(np.sort((words[sel] >> u32(8 * lane)) & u32(0xFF)), np.arange(256))
        for other in set(range(4)) - {lane}:  # a decode of another lane reads the complement
            assert np.all(((words[sel] >> u32(8 * other)) & u32(0xFF)) == (~(words[sel] >> u32(8 * lane)) & u32(0xFF)))
    a, _ = mc.cases("unpack_f16")
    w = a[-131072:]
    assert np.array_equal(w[:65536] & u32(0xFFFF), np.arange(65536)) and np.array_equal(w[65536:] >> u32(16), np.arange(65536))
    assert np.all(((w & u32(0xFFFF)) ^ (w >> u32(16))) == 0xFFFF)
    t = mc.unorm16_ties()
    assert len(t) == 65535
    a, _ = mc.cases("unorm16")
    assert np.isin(mc.fb(t), a).all() and np.isin(mc.fb(mc.snorm8_ties()), mc.cases("snorm8")[0]).all()


def test_windows_hold_both_neighbours_and_both_signs():
    w = mc.window(mc.fb(1.0))
    assert len(w) == 2 * mc.WINDOW + 1 and w.min() == 0x3F800000 - 64 and w.max() == 0x3F800000 + 64
    for name in ("exp2", "sqrt", "f2i32", "signf"):
        a = mc.cases(name)[0][len(mc.sweep()):]  # (what follows the sweep)
        for v in mc.COMMON_EDGES:
            for s in (v, -v):
                c = mc.fb(s)
                assert np.isin(mc.window(c), a).all(), (name, s)
                if np.isfinite(s) and abs(s) < 3e38:
                    assert np.isin(mc.fb([np.nextafter(f32(s), INF), np.nextafter(f32(s), -INF)]), a).all()
    # min / max: every ordered pair of the special operands
    a, b = mc.cases("minf")
    have = set(zip(a.tolist()[len(mc.sweep()):], b.tolist()[len(mc.sweep()):]))
    assert all((p, q) in have for p in mc.MINMAX_SPECIALS for q in mc.MINMAX_SPECIALS)


def test_exp_weight_leaves_out_only_the_undefined_conversions():
    a, _ = mc.cases("exp_weight")
    full = np.concatenate([mc.sweep(), mc.common()])
    kept = mc.exp_weight_defined(full)
    x = mc.bf(full)
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.all(kept[(x <= 0) | np.isnan(x)])  # the function's whole domain stays
        assert np.all(x[~kept] * mc.INV_LN2 >= f32(2.0 ** 31)) and np.any(kept & (x > 0))
    assert np.array_equal(a[:kept.sum()], full[kept])


def test_div_by_cases_are_the_claimed_domain():
    a, b = mc.cases("div_by")
    nd = len(mc.DIV_BY_DIVISORS)
    a, b = a.reshape(nd, -1), b.reshape(nd, -1)  # one row per divisor, the same dividends in each
    assert np.all(a == a[:1]) and np.all(b == b[:, :1])
    assert np.array_equal(mc.bf(b[:, 0]), np.array(mc.DIV_BY_DIVISORS, f32))
    x = mc.bf(a[0])
    with np.errstate(invalid="ignore"):
        inside = (np.abs(x) >= f32(2.0 ** -100)) & (np.abs(x) < f32(2.0 ** 100))
    zero_window = mc.window(mc.both(mc.fb(0.0)))
    assert np.array_equal(np.sort(a[0][~inside]), np.sort(zero_window))
    s = mc.sweep()
    with np.errstate(invalid="ignore"):
        sx = np.abs(mc.bf(s))
        assert np.array_equal(a[0][inside], s[(sx >= f32(2.0 ** -100)) & (sx < f32(2.0 ** 100))])  # no share left out
    assert inside.sum() > 5_000_000


def test_math_array_equals_the_scalar_entry_points(oracle_lib):
    import oracle
    rng = np.random.default_rng(11)
    a = np.concatenate([rng.integers(0, 1 << 32, 900, dtype=np.uint64).astype(u32), mc.common()[:100]])
    b = rng.integers(0, 1 << 32, len(a), dtype=np.uint64).astype(u32)
    assert len(a) == 1000
    x, y = mc.bf(a), mc.bf(b)

    def scalar(f, *args):
        return np.array([f(*[float(v) for v in t]) for t in zip(*args)], f32).view(u32)

    def same(got, want):
        return bool(np.all((got == want) | (np.isnan(got.view(f32)) & np.isnan(want.view(f32)))))

    L = oracle_lib
    assert same(oracle.math_array("exp2", a), scalar(L.hko_exp2, x))
    assert same(oracle.math_array("log2", a), scalar(L.hko_log2, x))
    s, c = oracle.math_array("sincos", a)
    assert same(s, scalar(L.hko_sin, x)) and same(c, scalar(L.hko_cos, x))
    assert same(oracle.math_array("pow", a, b), scalar(L.hko_pow, x, y))
    for n in (2, 5, 16):
        want = np.array([L.hko_pow_int(float(v), n) for v in x], f32).view(u32)
        assert same(oracle.math_array(f"pow{n}", a), want)
    # hko_f32_to_f16's inverse: the decode of every f16 code encodes back to the code (NaNs to a NaN of the same sign)
    codes = np.arange(65536, dtype=u32)
    lo, hi = oracle.math_array("unpack_f16", codes | (codes << u32(16)))
    assert np.array_equal(lo, hi)
    pick = np.concatenate([rng.integers(0, 65536, 900), np.array([0, 1, 0x3FF, 0x400, 0x7BFF, 0x7C00, 0x7C01, 0x7E00, 0x8000, 0x8001,
                                                                  0xFBFF, 0xFC00, 0xFE00, 0xFFFF])])
    pick = np.concatenate([pick, np.arange(0x3F0, 0x3F0 + 1000 - len(pick))])
    assert len(pick) == 1000
    for h in pick:
        back = L.hko_f32_to_f16(float(lo.view(f32)[h])) if not np.isnan(lo.view(f32)[h]) else None
        if back is None:
            assert (h & 0x7C00) == 0x7C00 and (h & 0x3FF) and (int(lo[h]) >> 31) == (h >> 15)
        else:
            assert back == h, hex(h)
    # refusals
    assert L.hko_math_array(-1, a.ctypes.data, None, 4, a.ctypes.data, None) == -1
    assert L.hko_math_array(len(names()), a.ctypes.data, None, 4, a.ctypes.data, None) == -1
