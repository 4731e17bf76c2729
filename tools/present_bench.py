"""Present-pass kernel timing (development aid): cornell at display size 3840x2160, the input from SMAA TU4x + Jasmine at
ratio 2 (the TAA plane, 3840x2160) and from Fsr1 at ratio 1.5 (the RCAS plane, 3840x2160), presented into the context's
own 3840x2160 plane in each format.  The variants present_run 1 and 0 alternate call by call in one process; kernel
durations come from hk_enable_kernel_timing (device events around the call's launches).  Per configuration: warm-up
calls, then two blocks of timed hk_present calls per variant; the larger difference between the two block medians of a
variant is the run's spread, and present_run 1 is "faster" only if it wins by more than that.  Compulsory traffic:
8 B read per input texel + 4 B (sRGB8) or 8 B (RGBA16F) stored per target texel, against 8.0 TB/s.
usage: python tools/present_bench.py [calls-per-block (default 60)]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'bevy-hikari_amd'))
from hikari_amd import (HikariRenderer, HikariSettings, PresentFormat, Taa, Upscale, _abi, examples,  # noqa: E402
                        frame_inputs)
from hikari_amd.plugin import _check  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 60
WARMUP = 10
W, H = 3840, 2160
HBM = 8.0e12


def one_call(r, s, target, run):
    import ctypes as C
    r.set_option("present_run", run)
    r.enable_kernel_timing(True)  # clears the sums: the next reading is this call's
    _check(r.ctx, _abi.lib().hk_present(r.ctx, C.byref(s), C.byref(target), None), "hk_present")
    return r.kernel_timing()["present"]


def bench(st, label):
    scene, cam, lights = examples.cornell()
    s = st.to_c()
    ratio = st.upscale.ratio()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    r.resize(W, H, ratio)
    r.set_fsr1_sharpness(st.upscale.sharpness())
    for f in range(2):
        fi = frame_inputs(f, cam, lights, W, H)
        r.render_gbuffer(fi)
        r.render_frame(s, fi)
        r.denoise(s, fi)
        r.tone_sum(s)
        r.post_process(s, fi)
    iw, ih, _ = r.output_info(22 if st.upscale.kind == "Fsr1" else 19)
    for fmt in (PresentFormat.RGBA8_SRGB, PresentFormat.RGBA16F):
        target = _abi.hk_present_target(None, W, H, 0, int(fmt), 0, 0, 0, 0, -1)
        for k in range(WARMUP):
            one_call(r, s, target, k & 1)
        blocks = []
        for _ in range(2):
            t = {1: [], 0: []}
            for k in range(2 * CALLS):
                t[k & 1].append(one_call(r, s, target, k & 1))
            blocks.append(t)
        out = {"input": label, "input_size": [iw, ih], "target": [W, H], "format": fmt.name, "calls_per_block": CALLS}
        nbytes = 8.0 * iw * ih + (8.0 if fmt == PresentFormat.RGBA16F else 4.0) * W * H
        for run, name in ((1, "run"), (0, "per_texel")):
            med = [statistics.median(b[run]) for b in blocks]
            ms = statistics.median(x for b in blocks for x in b[run])
            out[f"{name}_ms"] = {"median": ms, "block_medians": med, "share_of_hbm": nbytes / (ms * 1e-3) / HBM}
        spread = max(abs(out[f"{n}_ms"]["block_medians"][0] - out[f"{n}_ms"]["block_medians"][1]) for n in ("run", "per_texel"))
        out["spread_ms"] = spread
        diff = out["per_texel_ms"]["median"] - out["run_ms"]["median"]
        out["faster"] = "run" if diff > spread else ("per_texel" if -diff > spread else "within the spread")
        print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    bench(HikariSettings(upscale=Upscale.smaa_tu4x(2.0), taa=Taa.Jasmine), "smaa_tu4x ratio 2 + jasmine (TAA plane)")
    bench(HikariSettings(upscale=Upscale.fsr1(1.5, 0.2), taa=Taa.Jasmine), "fsr1 ratio 1.5 (RCAS plane)")
