"""The sRGB8 thresholds of include/hk_overlay.h, computed exactly.

The present pass stores the sRGB code of a linear value c as  code(c) = #{k in 1..255 : c >= T[k]},  where T[k] is the
smallest f32 whose exact sRGB encode, times 255, is >= k - 0.5.  The encode is the piecewise definition of the sRGB
standard (IEC 61966-2-1), monotone over [0, 1]:
    c <= 0.0031308:  12.92 c          otherwise:  1.055 c^(1 / 2.4) - 0.055
so with e = (k - 0.5) / 255 the condition `encode(c) >= e` is a comparison of rationals:
    12.92 c >= e          or          c^5 >= ((e + 0.055) / 1.055)^12        (both sides positive, 1 / 2.4 = 5 / 12)
It is evaluated in `fractions`, never in float, and T[k] is found by bisection over the f32 bit patterns (positive
floats are ordered like their bits).

usage: python tools/srgb_thresholds.py            print the table as the header holds it (hex floats)
       python tools/srgb_thresholds.py --check    compare with include/hk_overlay.h; exit status 1 on a difference
"""
import re
import struct
import sys
from fractions import Fraction
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "hk_overlay.h"
KNEE = Fraction(31308, 10**7)
A, B, S = Fraction(1055, 1000), Fraction(55, 1000), Fraction(1292, 100)


def f32(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def reaches(c: Fraction, e: Fraction) -> bool:
    """encode(c) >= e, exactly."""
    if c <= KNEE:
        return S * c >= e
    return c ** 5 >= ((e + B) / A) ** 12


def threshold_bits(k: int) -> int:
    e = Fraction(2 * k - 1, 510)
    lo, hi = 0, 0x3F800000  # encode(0) = 0 < e <= encode(1) = 1
    assert not reaches(Fraction(f32(lo)), e) and reaches(Fraction(f32(hi)), e)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if reaches(Fraction(f32(mid)), e):
            hi = mid
        else:
            lo = mid
    return hi


def thresholds_bits():
    """[bits of T[1], ..., bits of T[255]]"""
    return [threshold_bits(k) for k in range(1, 256)]


def thresholds():
    """T[0..255] as Python floats (each exactly an f32); T[0] = 0 is never counted."""
    return [0.0] + [f32(b) for b in thresholds_bits()]


def header_values():
    """The 256 literals of HK_OVERLAY_SRGB_T in include/hk_overlay.h as floats."""
    text = HEADER.read_text()
    body = text[text.index("#define HK_OVERLAY_SRGB_T"):]
    body = body[:body.index("\n\n")]
    return [float.fromhex(m) for m in re.findall(r"(0x[0-9a-f.]+p[+-]?\d+)f", body)]


def literal(x: float) -> str:
    mantissa, exponent = float(x).hex().split("p")
    return mantissa.rstrip("0").rstrip(".") + "p" + exponent + "f"


def table_text() -> str:
    t = thresholds()
    lines = ["#define HK_OVERLAY_SRGB_T \\"]
    for i in range(0, 256, 8):
        row = ", ".join(literal(v) for v in t[i:i + 8])
        lines.append("    " + row + ("," if i + 8 < 256 else "") + " \\")
    lines[-1] = lines[-1][:-2]
    return "\n".join(lines)


if __name__ == "__main__":
    if "--check" in sys.argv:
        ok = header_values() == thresholds()
        print("include/hk_overlay.h matches" if ok else "include/hk_overlay.h DIFFERS from the exact thresholds")
        sys.exit(0 if ok else 1)
    print(table_text())
