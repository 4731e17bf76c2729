"""The premise of every parity test: include/hk_math.h and the IEEE operations the kernels lean on give, compiled by
hipcc for the device, the bits the gcc-built oracle gives.

hk_selftest_math runs one scalar function per call, each as the frame kernels call it, on the inputs of
tests/math_cases.py (the strided sweep of all 2^32 patterns, windows around every edge the code selects on, the whole
small domains; tests/test_math_cases.py shows the sets hold them) and must return hko_math_array's words: hk_math.h's
function on the host, or the plain IEEE restatement for the device-only helpers (rcp_exact and rcp_fast against 1 / x,
div_by against x / d).  A NaN equals any NaN (texture_numpy.same_words' rule); nothing else is tolerated and no input
is left out.  tools/math_sweep.py runs all 2^32 patterns of the one-operand ids the same way."""
import numpy as np
import pytest

import math_cases as mc

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24  # words per call: at most five 64-MiB device buffers


def _names():
    from hikari_amd import _abi
    return _abi.MATH_FN_NAMES


def pytest_generate_tests(metafunc):
    if "fn_name" in metafunc.fixturenames:
        metafunc.parametrize("fn_name", _names())


@pytest.fixture(scope="module")
def device():
    from hikari_amd import HikariRenderer
    r = HikariRenderer(0)
    yield r
    r.close()


def _pair(x):
    return x if isinstance(x, tuple) else (x,)


def differing(got, want):
    """Indices where two word arrays differ, a NaN equal to any NaN (as texture_numpy.same_words)."""
    g, w = got.view(np.float32), want.view(np.float32)
    return np.flatnonzero(~((got == want) | (np.isnan(g) & np.isnan(w))))


def mismatches(r, name, float_results=True):
    """Run `name` on its cases, device and host: (inputs, differing words, the first of them as (output index, a, b, got,
    want))."""
    import oracle
    from hikari_amd import _abi
    a, b = mc.cases(name)
    count, first = 0, []
    for lo in range(0, len(a), CHUNK):
        ca = a[lo:lo + CHUNK]
        cb = None if b is None else b[lo:lo + CHUNK]
        got, want = _pair(r.selftest_math(name, ca, cb)), _pair(oracle.math_array(name, ca, cb))
        assert len(got) == len(want) == (2 if name in _abi.MATH_FN_TWO_RESULTS else 1)
        for k, (g, w) in enumerate(zip(got, want)):
            idx = differing(g, w) if float_results else np.flatnonzero(g != w)
            count += len(idx)
            first += [(k, int(ca[i]), None if cb is None else int(cb[i]), int(g[i]), int(w[i])) for i in idx[:5]]
    return len(a), count, first[:5]


def report(name, n, count, first, hint=""):
    lines = [f"out{k}: a={a:08x}" + ("" if b is None else f" b={b:08x}") + f" got={g:08x} want={w:08x}"
             for k, a, b, g, w in first]
    return f"{hint}{name}: {count} of {n} words differ from the host's; first (hex): " + "; ".join(lines)


INTEGER_RESULTS = ("unorm16", "snorm8", "f2u32", "f2i32")  # codes: every bit counts, no NaN rule
FLAGS_HINT = ("look first at the compile flags (bevy-hikari_amd/Makefile HIPFLAGS: the correctly rounded f32 divide "
              "and sqrt are hipcc's compile-time choice; no -ffast-math, -fhip-fp32-correctly-rounded-divide-sqrt on); ")


def test_device_function_equals_the_hosts_bits(device, fn_name):
    n, count, first = mismatches(device, fn_name, fn_name not in INTEGER_RESULTS)
    assert count == 0, report(fn_name, n, count, first)


def test_device_divide_and_sqrt_are_ieee(device):
    """a / b and sqrtf on the device are the IEEE quotient and root (the host's).  The two device-side self-tests of
    rcp_exact and div_by compare with the device's own divide; with this, and with the rcp_exact and div_by ids above
    against the host's quotient, they stand on the host's arithmetic."""
    for name in ("div", "sqrt"):
        n, count, first = mismatches(device, name)
        assert count == 0, report(name, n, count, first, FLAGS_HINT)


def test_selftest_math_refusals_leave_the_context_usable(device):
    from hikari_amd import _abi
    r = device
    call = r._L.hk_selftest_math
    a = np.array([0x3F800000, 0x40000000], np.uint32)
    b = np.array([0x40400000, 0x3F000000], np.uint32)
    out0 = np.full(2, 7, np.uint32)
    out1 = np.full(2, 7, np.uint32)
    p = lambda x: x.ctypes.data
    F = _abi.MATH_FN
    for fn in (-1, len(_abi.MATH_FN_NAMES), 1000):
        assert call(r.ctx, fn, p(a), p(b), 2, p(out0), p(out1)) == _abi.HK_ERR_INVALID
    assert call(None, F["exp2"], p(a), None, 2, p(out0), None) == _abi.HK_ERR_INVALID
    assert call(r.ctx, F["exp2"], None, None, 2, p(out0), None) == _abi.HK_ERR_INVALID
    assert call(r.ctx, F["exp2"], p(a), None, 2, None, None) == _abi.HK_ERR_INVALID
    for two in _abi.MATH_FN_TWO_OPERANDS:
        assert call(r.ctx, F[two], p(a), None, 2, p(out0), p(out1)) == _abi.HK_ERR_INVALID
    assert call(r.ctx, F["sincos"], p(a), None, 2, p(out0), None) == _abi.HK_ERR_INVALID
    assert np.all(out0 == 7) and np.all(out1 == 7)
    assert call(r.ctx, F["exp2"], None, None, 0, None, None) == _abi.HK_OK  # n == 0: nothing to do
    assert call(r.ctx, F["unpack_f16"], p(a), None, 2, p(out0), None) == _abi.HK_OK  # out1 optional here
    assert list(out0) == [0, 0] and np.all(out1 == 7)
    assert len(r.selftest_math("exp2", np.zeros(0, np.uint32))) == 0
    assert list(r.selftest_math("div", a, b).view(np.float32)) == [np.float32(1.0) / np.float32(3.0), 4.0]
    s, c = r.selftest_math("sincos", np.zeros(1, np.uint32))
    assert (s.view(np.float32)[0], c.view(np.float32)[0]) == (0.0, 1.0)
