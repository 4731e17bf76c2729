"""Cost of an instance refit against the rebuild it stands in for, and what the kept trees then cost to walk, in one
process on one machine.

Call time: hk_refit_instances against hk_update_instances per call with its one stream wait included, on the city
example (1,130 instances), on mesh_bench's single 20,000-triangle mesh (two instances: the floor of the call) and on a
seeded scene of 10,000 instances; hk_refit_meshes_all against hk_refit_meshes on city's sphere.  The two sides alternate
in blocks on one context: 10 warm-up calls each, then 2 x 2 blocks of 30 calls; the median of a side's 60 calls, and the
difference between its two block medians as its spread.  Each side's launches by name from hk_kernel_timing, in separate
runs of 30 calls: where the rebuild's time is, and what of it the refit still pays.

Walk cost: whole 3840 x 2160 frames on city (G-buffer, light passes, denoiser, tone) on the refit trees against rebuilt
trees of the same models: bench.py's per-frame rotation of the sphere after 1, 30 and 300 frames, and every instance
displaced by a tenth of, once and ten times its own size from where the trees were built (the ground plane stays).

    python tools/instance_refit_bench.py [calls | walk]

Every JSON line is printed and appended to profiles/instance_refit_bench.jsonl."""
import json
import sys
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np  # noqa: E402

import refit_bench as rb  # noqa: E402
from hikari_amd import HikariRenderer, Scene, StandardMaterial, examples, make_lights, plane_mesh  # noqa: E402
from mesh_bench import big_grid, city_sphere, deform  # noqa: E402

OUT = ROOT / "profiles" / "instance_refit_bench.jsonl"
rb.OUT = OUT  # (refit_bench.emit appends there)
SEED = 0x49524654


def seeded_scene(n: int = 10000, emitters: int = 100):
    """n small quads at seeded places in a 40 x 40 x 10 box, every (n // emitters)-th one emissive."""
    rng = np.random.default_rng(SEED)
    s = Scene()
    quad = s.add_mesh(plane_mesh(0.3))
    grey = s.add_material(StandardMaterial(base_color=(0.7, 0.65, 0.6, 1.0)))
    glow = s.add_material(StandardMaterial(emissive=(1.0, 0.9, 0.7, 0.3)))
    for k in range(n):
        m = np.eye(4)
        m[:3, 3] = rng.uniform((-20.0, 0.0, -20.0), (20.0, 10.0, 20.0))
        s.add_instance(quad, glow if k % (n // emitters) == 0 else grey, m)
    return s


def jitter(models0: np.ndarray, k: int, amount: float = 0.05) -> np.ndarray:
    """Call k's models: every instance moved a little (a seeded offset per call), as props that move per frame."""
    rng = np.random.default_rng([SEED, k])
    m = models0.copy()
    m[:, 12:15] += rng.uniform(-amount, amount, (len(m), 3)).astype(np.float32)
    return m


def instance_calls(label: str, scene) -> None:
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    models0, aabbs = scene.instance_models(), scene.instance_local_aabbs()
    state = {}

    def prepare(k):
        state["m"] = jitter(models0, k)

    def refit():
        r.update_instances(state["m"], aabbs, refit=True)

    def rebuild():
        r.update_instances(state["m"], aabbs)

    out = {"measure": "call time", "workload": label, "instances": len(models0),
           "emitters": int(scene.desc.emissives.count)}
    out.update(rb.alternating(prepare, {"hk_refit_instances": refit, "hk_update_instances": rebuild}))
    rb.verdict(out, "hk_refit_instances", "hk_update_instances")
    out["refit_kernel_ms_per_call"] = rb.timed_kernels(r, prepare, refit)
    out["rebuild_kernel_ms_per_call"] = rb.timed_kernels(r, prepare, rebuild)
    rb.emit(out)
    r.close()


def mesh_calls(label: str, scene, mesh_id: int) -> None:
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    mesh = scene.meshes[mesh_id]
    rest = np.asarray(mesh.positions, np.float64).copy()
    aabbs = scene.instance_local_aabbs()

    def prepare(k):
        deform(mesh, rest, k)

    def refit_all():
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs, refit="all")

    def refit_blas():
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs, refit=True)

    out = {"measure": "call time", "workload": label, "instances": len(scene.instances)}
    out.update(rb.alternating(prepare, {"hk_refit_meshes_all": refit_all, "hk_refit_meshes": refit_blas}))
    rb.verdict(out, "hk_refit_meshes_all", "hk_refit_meshes")
    out["refit_kernel_ms_per_call"] = rb.timed_kernels(r, prepare, refit_all)
    out["rebuild_kernel_ms_per_call"] = rb.timed_kernels(r, prepare, refit_blas)
    rb.emit(out)
    r.close()


def walk_cost() -> None:
    scene, cam, lights = examples.SCENES["city"]()
    scene.build()
    size = (3840, 2160)
    models0, aabbs = scene.instance_models(), scene.instance_local_aabbs()
    sphere = [i for i, (m, _, _) in enumerate(scene.instances) if len(scene.meshes[m].positions) == 37 * 19][-1]
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    r.resize(*size, 1.0)

    def rotated(frames):  # bench.py's city-4k-dynamic step after `frames` frames
        a = 0.2 * (frames / 60.0)
        rz = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        m = models0.copy()
        m[sphere] = (models0[sphere].reshape(4, 4).T @ rz).T.reshape(16).astype(np.float32)
        return m

    def displaced(factor):  # every instance moved by `factor` times its own world extent, in a seeded direction
        rng = np.random.default_rng([SEED, int(factor * 10)])
        m = models0.copy()
        extent = np.array([2.0 * np.linalg.norm(np.abs(m[k].reshape(4, 4).T[:3, :3]) @ aabbs[k, 3:6])
                           for k in range(len(m))])
        for k in range(len(m)):
            if k == int(np.argmax(extent)):  # the ground plane, 100 wide: it stays, or it would cover the camera
                continue
            d = rng.normal(size=3)
            m[k, 12:15] += (factor * extent[k] * d / np.linalg.norm(d)).astype(np.float32)
        return m

    moves = [(f"sphere rotated as by bench.py after {f} frames", rotated(f)) for f in (1, 30, 300)]
    moves += [(f"every instance displaced by {f} x its own size", displaced(f)) for f in (0.1, 1.0, 10.0)]
    for label, models in moves:
        r.update_instances(models0, aabbs)  # the trees of the uploaded layout
        r.update_instances(models, aabbs, refit=True)
        kept = rb.frame_ms(r, cam, lights, size)
        r.update_instances(models, aabbs)
        rebuilt = rb.frame_ms(r, cam, lights, size)
        rb.emit({"measure": "walk cost", "workload": "city, 3840 x 2160", "models": label, "refit_trees": kept,
                 "rebuilt_trees": rebuilt,
                 "ratio_refit_over_rebuilt": round(kept["ms_per_frame"] / rebuilt["ms_per_frame"], 3)})
    r.close()


if __name__ == "__main__":
    what = sys.argv[1:] or ["calls", "walk"]
    if "calls" in what:
        instance_calls("city, 1,130 instances", examples.SCENES["city"]()[0])
        instance_calls("single mesh of 20,000 triangles and a lamp", big_grid()[0])
        instance_calls("seeded quads, 10,000 instances", seeded_scene())
        mesh_calls("city, UV sphere 36 x 18 deformed", *city_sphere())
    if "walk" in what:
        walk_cost()
