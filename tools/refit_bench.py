"""Cost of a BLAS refit against the rebuild it stands in for, and what the refit tree then costs to walk, in one process
on one machine.

Call time: hk_refit_meshes against hk_update_meshes, and hk_skin_meshes_refit against hk_skin_meshes, per call with its
one stream wait included, on the city example's UV sphere (36 x 18; 2 joints) and on a single mesh of 20,000 triangles
(32 joints).  The two sides alternate in blocks on one context: 10 warm-up calls each, then 2 x 2 blocks of 30 calls;
the median of a side's 60 calls, and the difference between its two block medians as its spread.  The refit call's
launches by name from hk_kernel_timing, in a separate run of 30 calls.

Walk cost: the 20,000-triangle mesh deformed at three amplitudes (a small wave, mesh_bench's own, folded over itself)
away from the shape its tree was built for; ms per 1280 x 720 frame (G-buffer, light passes, denoiser, tone) and the ray
counters on the refit tree against the rebuilt tree of the same vertices.  (The counters count rays, not node visits:
the library exposes no visit count, so the frame time and the walking kernels' times are the measure.)

Every JSON line is printed and appended to profiles/refit_bench.jsonl."""
import json
import sys
import time
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np  # noqa: E402

from hikari_amd import (Camera, HikariRenderer, HikariSettings, Transform, Upscale, frame_inputs,  # noqa: E402
                        make_lights)
from mesh_bench import big_grid, city_sphere, deform  # noqa: E402
from skin_bench import palette, rig  # noqa: E402

WARMUP, BLOCK = 10, 30
OUT = ROOT / "profiles" / "refit_bench.jsonl"


def emit(record: dict) -> None:
    line = json.dumps(record)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def alternating(prepare, sides: dict) -> dict:
    """prepare(k) makes call k's input (not timed); sides: {name: call}.  Blocks alternate between the sides."""
    k = 0
    for call in sides.values():
        for _ in range(WARMUP):
            prepare(k)
            call()
            k += 1
    torch.cuda.synchronize()
    times = {name: [] for name in sides}
    for _ in range(2):
        for name, call in sides.items():
            t = []
            for _ in range(BLOCK):
                prepare(k)
                k += 1
                t0 = time.perf_counter()
                call()
                t.append(time.perf_counter() - t0)
            times[name].append(t)
    out = {}
    for name, blocks in times.items():
        med = [float(np.median(b)) for b in blocks]
        out[name] = {"median_ms": round(float(np.median(sum(blocks, []))) * 1e3, 4),
                     "block_medians_ms": [round(m * 1e3, 4) for m in med],
                     "spread_ms": round(abs(med[0] - med[1]) * 1e3, 4)}
    return out


def timed_kernels(r, prepare, call) -> dict:
    r.enable_kernel_timing(True)
    for k in range(30):
        prepare(k)
        call()
    r.sync()
    out = {k: round(v, 4) for k, v in r.kernel_timing().items()}
    r.enable_kernel_timing(False)
    return out


def verdict(out: dict, refit: str, rebuild: str) -> None:
    a, b = out[refit], out[rebuild]
    out["ratio_rebuild_over_refit"] = round(b["median_ms"] / a["median_ms"], 2)
    out["faster_by_more_than_both_spreads"] = b["median_ms"] - a["median_ms"] > a["spread_ms"] + b["spread_ms"]


def update_calls(label: str, scene, mesh_id: int) -> None:
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    mesh = scene.meshes[mesh_id]
    rest = np.asarray(mesh.positions, np.float64).copy()
    aabbs = scene.instance_local_aabbs()

    def prepare(k):
        deform(mesh, rest, k)

    def refit():
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs, refit=True)

    def rebuild():
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs)

    out = {"measure": "call time", "workload": label, "triangles": (scene.mesh_index(mesh_id)[3] + 2) // 3}
    out.update(alternating(prepare, {"hk_refit_meshes": refit, "hk_update_meshes": rebuild}))
    verdict(out, "hk_refit_meshes", "hk_update_meshes")
    out["refit_kernel_ms_per_call"] = timed_kernels(r, prepare, refit)
    emit(out)
    r.close()


def skin_calls(label: str, scene, mesh_id: int, joints: int) -> None:
    rig(scene.meshes[mesh_id], joints, np.random.default_rng(7))
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    r.set_mesh_skins(scene, [mesh_id])
    aabbs = scene.instance_local_aabbs()
    state = {}

    def prepare(k):
        state["joints"] = palette(joints, k)

    def refit():
        r.skin_meshes(scene, {mesh_id: state["joints"]}, local_aabbs=aabbs, refit=True)

    def rebuild():
        r.skin_meshes(scene, {mesh_id: state["joints"]}, local_aabbs=aabbs)

    out = {"measure": "call time", "workload": label, "joints": joints,
           "triangles": (scene.mesh_index(mesh_id)[3] + 2) // 3}
    out.update(alternating(prepare, {"hk_skin_meshes_refit": refit, "hk_skin_meshes": rebuild}))
    verdict(out, "hk_skin_meshes_refit", "hk_skin_meshes")
    out["refit_kernel_ms_per_call"] = timed_kernels(r, prepare, refit)
    emit(out)
    r.close()


def fold(mesh, rest) -> None:
    """The grid folded over itself along x = 0, the folded half a little in front."""
    p = rest.copy()
    p[:, 0] = np.abs(rest[:, 0]) - 0.5
    p[:, 2] = np.where(rest[:, 0] < 0, 0.05, 0.0)
    mesh.positions = p.astype(np.float32)


def wave(amplitude: float):
    def shape(mesh, rest):
        w = amplitude * np.sin(7.0 * rest[:, 0] + 0.37) * np.cos(5.0 * rest[:, 1] - 0.185)
        mesh.positions = (rest + np.array([0.0, 0.0, 1.0]) * w[:, None]).astype(np.float32)
    return shape


def frame_ms(r, cam, lights, size, frames: int = 20) -> dict:
    w, h = size
    s = HikariSettings(upscale=Upscale.SMAA_TU_1_0).to_c()

    def one(f):
        fi = frame_inputs(f, cam, lights, w, h)
        r.render_gbuffer(fi)
        r.render_frame(s, fi)
        r.denoise(s, fi)
        r.tone_sum(s)
    def wait():  # hk_sync makes the null stream wait for the context's streams; the host then waits for the device
        r.sync()
        torch.cuda.synchronize()
    for f in range(5):
        one(f)
    wait()
    r.reset_counters()
    med = []
    for b in range(2):
        t0 = time.perf_counter()
        for f in range(frames):
            one(5 + b * frames + f)
        wait()
        med.append((time.perf_counter() - t0) / frames)
    out = {"ms_per_frame": round(float(np.mean(med)) * 1e3, 4), "block_ms": [round(m * 1e3, 4) for m in med],
           "spread_ms": round(abs(med[0] - med[1]) * 1e3, 4), "counters": r.counters()}
    r.enable_kernel_timing(True)  # (a separate run: the events serialise nothing, but the window above stays clean)
    for f in range(frames):
        one(5 + 2 * frames + f)
    wait()
    out["kernel_ms_per_frame"] = {k: round(v, 4) for k, v in r.kernel_timing().items()}
    r.enable_kernel_timing(False)
    return out


def walk_cost() -> None:
    scene, mesh_id = big_grid()
    scene.build()
    size = (1280, 720)
    cam = Camera(Transform.from_xyz(0.9, -0.7, 2.8).looking_at((0.0, 0.0, 0.0)))  # (past the lamp, not through it)
    lights = make_lights(None)
    mesh = scene.meshes[mesh_id]
    rest = np.asarray(mesh.positions, np.float64).copy()
    aabbs = scene.instance_local_aabbs()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    r.resize(*size, 1.0)
    for label, shape in (("small wave, amplitude 0.01", wave(0.01)), ("mesh_bench's wave, amplitude 0.08", wave(0.08)),
                         ("folded over itself", fold)):
        mesh.positions = rest.astype(np.float32)
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs)  # the tree of the rest shape
        shape(mesh, rest)
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs, refit=True)
        refit = frame_ms(r, cam, lights, size)
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs)
        rebuilt = frame_ms(r, cam, lights, size)
        emit({"measure": "walk cost", "workload": "single mesh, 20,000 triangles, 1280 x 720", "deformation": label,
              "refit_tree": refit, "rebuilt_tree": rebuilt,
              "ratio_refit_over_rebuilt": round(refit["ms_per_frame"] / rebuilt["ms_per_frame"], 3)})
    r.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["walk"]:  # the walk cost alone
        walk_cost()
        sys.exit(0)
    update_calls("city, UV sphere 36 x 18 deformed", *city_sphere())
    update_calls("single mesh, 20,000 triangles", *big_grid())
    skin_calls("city, UV sphere 36 x 18 on 2 joints", *city_sphere(), 2)
    skin_calls("single mesh, 20,000 triangles on 32 joints", *big_grid(), 32)
    walk_cost()
