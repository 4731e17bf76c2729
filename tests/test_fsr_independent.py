"""FSR1 (EASU + RCAS) pinned by an independent restatement, on the CPU.

include/hk_fsr.h holds the per-pixel bodies that the gfx950 kernels and the CPU side of the GPU parity test
(tests/fsr_cpu.c) both compile, so GPU == CPU alone cannot catch a misreading of the shaders made in the header.
Here tests/fsr_cpu.c, built with the oracle's flags, is compared with tests/fsr_numpy.py, a vectorised float32
restatement written from the GLSL.  Every operation of both passes is an exactly rounded f32 operation, an integer
operation or an f16 round-to-nearest-even conversion, so the requirement is equality of every stored word (NaNs
canonicalised).  RCAS's constant is the one transcendental: sharpness 0, 1, 2 use the restatement's own
float32(2 ** -sharpness), sharpness 0.2 the C side's hk_exp2, itself held to hk_math's 4 ulp.
"""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fsr_numpy as fn
from parity import canon_f16

ROOT = Path(__file__).resolve().parent.parent
CFLAGS = ["-O3", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]  # oracle/Makefile's

SIZES = [(1, 1), (2, 3), (5, 4), (21, 16), (32, 24)]  # input (w, h)
RATIOS = [1.0, 1.3, 1.5, 1.7, 2.0]
KINDS = ["constant", "black", "edge_h", "edge_v", "edge_30", "edge_45", "edge_60", "checker", "noise",
         "black_half", "non_finite"]
MUTATIONS = ["gather_order", "rcas_clamp", "set_weights", "no_dering", "no_newton"]


class FsrCpu:
    """tests/fsr_cpu.c compiled into `directory` and loaded with ctypes."""

    def __init__(self, directory):
        so = Path(directory) / "libfsr_cpu.so"
        subprocess.run(["gcc", *CFLAGS, "-I", str(ROOT / "include"), "-shared", "-o", str(so),
                        str(ROOT / "tests" / "fsr_cpu.c"), "-lm"], check=True)
        L = C.CDLL(str(so))
        vp, u32, f = C.c_void_p, C.c_uint32, C.c_float
        L.fsr_cpu_easu_constants.argtypes = [f, f, f, f, vp]
        L.fsr_cpu_easu_constants.restype = None
        L.fsr_cpu_rcas_constant.argtypes = [f]
        L.fsr_cpu_rcas_constant.restype = f
        for name in ("fsr_cpu_easu", "fsr_cpu_easu_tiled"):
            getattr(L, name).argtypes = [vp, u32, u32, vp, u32, u32]
        L.fsr_cpu_easu.restype = None
        L.fsr_cpu_easu_tiled.restype = C.c_int
        L.fsr_cpu_rcas.argtypes = [vp, u32, u32, f, vp]
        L.fsr_cpu_rcas.restype = None
        self.L = L

    def easu_constants(self, iw, ih, ow, oh):
        out = np.zeros(14, np.float32)
        self.L.fsr_cpu_easu_constants(iw, ih, ow, oh, out.ctypes.data)
        return out

    def rcas_constant(self, sharpness):
        return np.float32(self.L.fsr_cpu_rcas_constant(sharpness))

    def easu(self, words, ow, oh, tiled=False):
        """words: (h, w, 4) uint16 RGBA16F -> (oh, ow, 4) uint16 (tiled: and the blocks that were not staged)."""
        src = np.ascontiguousarray(words, np.uint16)
        out = np.zeros((oh, ow, 4), np.uint16)
        fnc = self.L.fsr_cpu_easu_tiled if tiled else self.L.fsr_cpu_easu
        rc = fnc(src.ctypes.data, src.shape[1], src.shape[0], out.ctypes.data, ow, oh)
        return (out, rc) if tiled else out

    def rcas(self, words, con):
        src = np.ascontiguousarray(words, np.uint16)
        out = np.zeros_like(src)
        self.L.fsr_cpu_rcas(src.ctypes.data, src.shape[1], src.shape[0], float(con), out.ctypes.data)
        return out


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return FsrCpu(tmp_path_factory.mktemp("fsr_cpu"))


def output_size(s, ratio):
    """The largest display size whose integrator size is s: s = ceil((1 / ratio) S) in f32 (light.rs:318-319)."""
    S = int(math.floor(s * ratio))
    assert int(np.ceil(np.float32(1.0) / np.float32(ratio) * np.float32(S))) == s
    return S


def image(kind, w, h):
    """A synthetic RGBA16F image (h, w, 4) as uint16 words; finite values in [0, 1]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(0xF5A1 + 97 * w + h)

    def edge(deg):
        a = math.radians(deg)
        side = (x - (w - 1) / 2) * math.cos(a) + (y - (h - 1) / 2) * math.sin(a) > 0.2
        return np.where(side[..., None], [0.9, 0.7, 0.2], [0.1, 0.25, 0.6])
    if kind == "constant":
        rgb = np.broadcast_to([0.5, 0.25, 0.75], (h, w, 3))
    elif kind == "black":
        rgb = np.zeros((h, w, 3))
    elif kind == "edge_h":
        rgb = edge(90)
    elif kind == "edge_v":
        rgb = edge(0)
    elif kind.startswith("edge_"):
        rgb = edge(int(kind[5:]))
    elif kind == "checker":
        rgb = np.where((((x + y) % 2) == 0)[..., None], [1.0, 0.9, 0.8], [0.0, 0.1, 0.05])
    elif kind in ("noise", "non_finite"):
        rgb = rng.uniform(0.0, 1.0, (h, w, 3))
    elif kind == "black_half":
        rgb = rng.uniform(0.0, 1.0, (h, w, 3)) * (x >= w / 2)[..., None]
    else:
        raise KeyError(kind)
    img = np.concatenate([rgb, np.ones((h, w, 1))], axis=-1).astype(np.float16)
    if kind == "non_finite":
        for k in range(max(1, (w * h) // 40)):
            img[rng.integers(h), rng.integers(w), rng.integers(3)] = np.inf if k % 2 == 0 else np.nan
    return np.ascontiguousarray(img).view(np.uint16)


def decode(words):
    return words.view(np.float16).astype(np.float32)


def cases():
    for (w, h) in SIZES:
        for r in RATIOS:
            yield w, h, output_size(w, r), output_size(h, r)


def same(got, want):
    return np.array_equal(canon_f16(got), canon_f16(want))


def test_output_sizes_are_odd_and_even():
    sizes = {S for w, h, ow, oh in cases() for S in (ow, oh)}
    assert any(S % 2 for S in sizes) and any(S % 2 == 0 for S in sizes)
    assert any(ow % 16 and ow > 16 for _, _, ow, _ in cases())  # partial 16 x 16 blocks next to whole ones


def test_constants(cpu):
    """FsrEasuCon word for word, hk_exp2 at the tested sharpness values."""
    for w, h, ow, oh in cases():
        want = np.concatenate([np.asarray(c, np.float32) for c in fn.easu_con(w, h, ow, oh)])
        assert cpu.easu_constants(w, h, ow, oh).tobytes() == want.tobytes(), (w, h, ow, oh)
    for s in (0.0, 1.0, 2.0):
        assert cpu.rcas_constant(s) == fn.rcas_con(s)  # exact powers of two
    got, exact = float(cpu.rcas_constant(0.2)), 2.0 ** -0.2
    assert abs(got - exact) <= 4 * np.spacing(np.float32(exact))  # hk_math's stated accuracy


@pytest.mark.parametrize("kind", KINDS)
def test_easu_matches_restatement(cpu, kind):
    for w, h, ow, oh in cases():
        src = image(kind, w, h)
        want = fn.easu(decode(src), ow, oh)
        got = cpu.easu(src, ow, oh)
        assert same(got, want), f"{kind} {w}x{h} -> {ow}x{oh}: {int((canon_f16(got) != canon_f16(want)).sum())} words"
        tiled, unstaged = cpu.easu(src, ow, oh, tiled=True)
        assert unstaged == 0 and np.array_equal(tiled, got), f"{kind} {w}x{h} -> {ow}x{oh}: staged tiles differ"


@pytest.mark.parametrize("kind", KINDS)
def test_rcas_matches_restatement(cpu, kind):
    """On the synthetic images themselves and on their EASU upscales (ratio 1.5)."""
    c02 = cpu.rcas_constant(0.2)
    for (w, h) in SIZES:
        src = image(kind, w, h)
        for words in (src, cpu.easu(src, output_size(w, 1.5), output_size(h, 1.5))):
            for sharp in (0.0, 1.0, 2.0):
                assert same(cpu.rcas(words, fn.rcas_con(sharp)), fn.rcas(decode(words), sharp)), (kind, w, h, sharp)
            assert same(cpu.rcas(words, c02), fn.rcas(decode(words), con=c02)), (kind, w, h, 0.2)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_misreadings_are_caught(cpu, mutation):
    """Each misreading, applied to the restatement, changes the stored words of at least one image."""
    caught = []
    for kind in KINDS:
        for w, h, ow, oh in cases():
            src = image(kind, w, h)
            if mutation in ("rcas_clamp", "no_newton"):
                bad, good = fn.rcas(decode(src), 0.0, mutate=mutation), cpu.rcas(src, fn.rcas_con(0.0))
            else:
                bad, good = fn.easu(decode(src), ow, oh, mutate=mutation), cpu.easu(src, ow, oh)
            if not same(bad, good):
                caught.append((kind, w, h, ow, oh))
        if caught:
            break
    assert caught, f"{mutation} changed no image"


def test_pipeline_on_oracle_frames(cpu):
    """cornell 32x24 -> 64x48 with TAA, 3 frames: the shared bodies on the oracle's TAA output against the
    restatement, and the sharpness constant the right way round (a larger value sharpens less)."""
    from hikari_amd import HikariSettings, Taa, Upscale, examples, frame_inputs, load_noise
    from oracle import Oracle
    W, H = 64, 48
    st = HikariSettings(upscale=Upscale.fsr1(2.0, 0.0), taa=Taa.Jasmine)
    scene, cam, lights = examples.cornell()
    o = Oracle(scene.build(), load_noise(), W, H, st.upscale.ratio(), threads=4)
    s = st.to_c()
    for f in range(3):
        fi = frame_inputs(f, cam, lights, W, H)
        o.render_gbuffer(fi)
        o.render_frame(s, fi)
        o.denoise(s, fi)
        o.tone_sum(s)
        o.post_process(s, fi)
        taa = o.output(19).view(np.uint16)
        assert taa.shape == (24, 32, 4)
        easu = cpu.easu(taa, W, H)
        assert same(easu, fn.easu(decode(taa), W, H)), f"frame {f} EASU"
        mad = {}
        for sharp in (0.0, 2.0):
            rcas = cpu.rcas(easu, cpu.rcas_constant(sharp))
            assert same(rcas, fn.rcas(decode(easu), sharp)), f"frame {f} RCAS {sharp}"
            mad[sharp] = float(np.abs(decode(rcas)[..., :3] - decode(easu)[..., :3]).mean())
        assert np.isfinite(decode(easu)).all() and mad[0.0] > mad[2.0] > 0.0, mad


def test_abi_exposes_fsr1():
    import hikari_amd
    A = hikari_amd._abi
    assert hasattr(A.lib(), "hk_set_fsr1_sharpness") and "hk_set_fsr1_sharpness" in A.EXPORTED_SYMBOLS
    assert (A.OUT_FSR_EASU, A.OUT_FSR_RCAS) == (21, 22)
    header = (ROOT / "include" / "hikari_amd.h").read_text()
    assert "HK_OUT_FSR_EASU = 21" in header and "HK_OUT_FSR_RCAS = 22" in header and "HK_OUT_COUNT = 23" in header
    doc = header[header.index("Runtime options"):header.index("int hk_set_option")]
    assert "fsr_tiled" in doc
    assert hasattr(hikari_amd.HikariRenderer, "set_fsr1_sharpness")
