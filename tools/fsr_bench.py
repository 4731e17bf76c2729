"""FSR1 kernel timing (development aid): cornell at display size 3840x2160, ratio 2 (s 1920x1080) and ratio 1.5
(s 2560x1440), the EASU variants fsr_tiled 1 and 0 alternating call by call in one process, kernel durations from
hk_enable_kernel_timing (device events around each launch).  Per configuration: warm-up calls, then two blocks of
timed hk_post_process calls; per kernel the median of each block, so the difference between the two blocks of one
variant is the run-to-run spread the variants' difference is judged against.  Compulsory traffic: EASU 8 B per input
texel + 8 B per output texel, RCAS 16 B per output texel, against 8.0 TB/s.
usage: python tools/fsr_bench.py [calls-per-block (default 60)]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'bevy-hikari_amd'))
from hikari_amd import HikariRenderer, HikariSettings, Taa, Upscale, examples, frame_inputs  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 60
WARMUP = 10
W, H = 3840, 2160
HBM = 8.0e12


def one_call(r, s, fi, tiled):
    r.set_option("fsr_tiled", tiled)
    r.enable_kernel_timing(True)  # clears the sums: the next reading is this call's
    r.post_process(s, fi)
    t = r.kernel_timing()
    return t["fsr_easu"], t["fsr_rcas"]


def bench(ratio):
    scene, cam, lights = examples.cornell()
    st = HikariSettings(upscale=Upscale.fsr1(ratio, 0.2), taa=Taa.Jasmine)
    s = st.to_c()
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
    sw, sh, _ = r.output_info(19)
    for k in range(WARMUP):
        one_call(r, s, fi, k & 1)
    blocks = []
    for _ in range(2):
        t = {1: [], 0: []}
        for k in range(2 * CALLS):
            tiled = k & 1
            t[tiled].append(one_call(r, s, fi, tiled))
        blocks.append(t)
    out = {"ratio": ratio, "input": [sw, sh], "output": [W, H], "calls_per_block": CALLS}
    easu_bytes, rcas_bytes = 8.0 * sw * sh + 8.0 * W * H, 16.0 * W * H
    for tiled, name in ((1, "tiled"), (0, "plain")):
        med = [statistics.median(e for e, _ in b[tiled]) for b in blocks]
        every = sorted(e for b in blocks for e, _ in b[tiled])
        ms = statistics.median(every)
        out[f"easu_{name}_ms"] = {"median": ms, "block_medians": med, "p10": every[len(every) // 10],
                                  "p90": every[9 * len(every) // 10],
                                  "share_of_hbm": easu_bytes / (ms * 1e-3) / HBM}
    rc = sorted(x for b in blocks for v in (0, 1) for _, x in b[v])
    rc_blocks = [statistics.median(x for v in (0, 1) for _, x in b[v]) for b in blocks]
    ms = statistics.median(rc)
    out["rcas_ms"] = {"median": ms, "block_medians": rc_blocks, "p10": rc[len(rc) // 10], "p90": rc[9 * len(rc) // 10],
                      "share_of_hbm": rcas_bytes / (ms * 1e-3) / HBM}
    spread = max(abs(out[f"easu_{n}_ms"]["block_medians"][0] - out[f"easu_{n}_ms"]["block_medians"][1])
                 for n in ("tiled", "plain"))
    out["easu_spread_ms"] = spread
    diff = out["easu_plain_ms"]["median"] - out["easu_tiled_ms"]["median"]
    out["faster"] = "tiled" if diff > spread else ("plain" if -diff > spread else "within the spread")
    r.close()
    return out


if __name__ == "__main__":
    for ratio in (2.0, 1.5):
        print(json.dumps(bench(ratio)), flush=True)
