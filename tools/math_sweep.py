#!/usr/bin/env python3
"""All 2^32 bit patterns of every one-operand function id of hk_selftest_math, device against host.

    python tools/math_sweep.py [--fn NAME[,NAME...]]

One process, one context: 256 calls of 2^24 patterns per function through HikariRenderer.selftest_math, each compared
word for word with the oracle's hko_math_array (a NaN equals any NaN; the codes of unorm16 / snorm8 / f2u32 / f2i32 bit
for bit; hk_exp_weight without the inputs whose int32 conversion C leaves undefined, tests/math_cases.py).  Prints one
line per function, the count of differing words and the first of them, and stops at the first failing call's error.
A tool, not a test: the host side costs tens of seconds per function.  tests/test_gpu_math.py runs the strided sweep and
the edges of the same comparison on every run; the result of this one is recorded in DESIGN.md §3."""
import argparse
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "bevy-hikari_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

CALLS, CHUNK = 256, 1 << 24
INTEGER_RESULTS = ("unorm16", "snorm8", "f2u32", "f2i32")


def main() -> int:
    import math_cases as mc
    import oracle
    from hikari_amd import HikariRenderer, _abi
    one_operand = [n for n in _abi.MATH_FN_NAMES if n not in _abi.MATH_FN_TWO_OPERANDS]
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--fn", default=",".join(one_operand), help="function names, comma-separated (default: all)")
    names = ap.parse_args().fn.split(",")
    for n in names:
        if n not in one_operand:
            ap.error(f"{n}: not a one-operand function id ({', '.join(one_operand)})")
    r = HikariRenderer(0)
    pool = ThreadPoolExecutor(1)
    total_bad = 0
    for name in names:
        t0 = time.time()
        bad, first, words = 0, None, 0
        for k in range(CALLS):
            a = np.arange(k * CHUNK, (k + 1) * CHUNK, dtype=np.uint64).astype(np.uint32)
            if name == "exp_weight":
                a = a[mc.exp_weight_defined(a)]
            dev = pool.submit(r.selftest_math, name, a)  # (raises here, at result(), on a failing call)
            want = oracle.math_array(name, a)
            got = dev.result()
            for j, (g, w) in enumerate(zip(*[x if isinstance(x, tuple) else (x,) for x in (got, want)])):
                same = g == w
                if name not in INTEGER_RESULTS:
                    same |= np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32))
                idx = np.flatnonzero(~same)
                bad += len(idx)
                if len(idx) and first is None:
                    i = idx[0]
                    first = f"out{j}: a={int(a[i]):08x} got={int(g[i]):08x} want={int(w[i]):08x}"
            words += len(a)
        total_bad += bad
        print(f"{name}: {bad} of {words} inputs differ" + (f"; first {first}" if first else "") +
              f" ({time.time() - t0:.0f} s)", flush=True)
    r.close()
    return 1 if total_bad else 0


if __name__ == "__main__":
    sys.exit(main())
