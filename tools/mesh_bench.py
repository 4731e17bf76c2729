"""Cost of a deforming mesh: hk_update_meshes on the GPU (per call, its one stream wait included) against the path it
replaces, Scene.build() + upload_scene (hks_build on the host, then hk_scene_upload), in one process on one machine.

Two workloads: the city example with its emissive UV sphere (36 x 18) deformed every call, and a single mesh of 20,000
triangles.  Each side: 10 warm-up calls, then two blocks of 30; the medians of the blocks' 60 calls, and the difference
between the two block medians as the spread.  One JSON line per workload."""
import json
import sys
import time
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
import numpy as np  # noqa: E402

from hikari_amd import HikariRenderer, Mesh, Scene, StandardMaterial, examples  # noqa: E402
from hikari_amd.scene import uv_sphere_mesh  # noqa: E402

WARMUP, BLOCK = 10, 30


def city_sphere():
    scene, _, _ = examples.SCENES["city"]()
    return scene, 1  # examples.city: mesh 0 is the ground plane, mesh 1 the sphere


def big_grid(cells: int = 100):
    """One mesh of 2 x cells^2 = 20,000 triangles and a small emitter."""
    g = np.linspace(-1.0, 1.0, cells + 1)
    x, y = np.meshgrid(g, g)
    pos = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1).astype(np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(pos), 1))
    uv = np.stack([x.ravel() * 0.5 + 0.5, y.ravel() * 0.5 + 0.5], axis=1).astype(np.float32)
    a = (np.arange(cells)[:, None] * (cells + 1) + np.arange(cells)[None, :]).ravel()
    b = a + cells + 1
    idx = np.stack([a, a + 1, b + 1, a, b + 1, b], axis=1).ravel().astype(np.uint32)
    scene = Scene()
    mesh = scene.add_mesh(Mesh(pos, nrm, uv, idx))
    grey = scene.add_material(StandardMaterial(base_color=(0.7, 0.7, 0.7, 1.0)))
    glow = scene.add_material(StandardMaterial(emissive=(1.0, 1.0, 1.0, 0.5)))
    m = np.eye(4)
    scene.add_instance(mesh, grey, m)
    lamp = np.eye(4)
    lamp[:3, 3] = (0.0, 0.0, 2.0)
    scene.add_instance(scene.add_mesh(uv_sphere_mesh(0.2, 8, 4)), glow, lamp)
    return scene, mesh


def deform(mesh: Mesh, rest: np.ndarray, k: int) -> None:
    """Call k's shape: the rest positions pushed along a travelling wave."""
    phase = 0.37 * k
    wave = 0.08 * np.sin(7.0 * rest[:, 0] + phase) * np.cos(5.0 * rest[:, 1] - 0.5 * phase)
    scale = 1.0 + wave[:, None]
    flat = np.ptp(rest[:, 2]) == 0.0
    mesh.positions = (rest + np.array([0.0, 0.0, 1.0]) * wave[:, None] if flat else rest * scale).astype(np.float32)


def blocks(prepare, call) -> dict:
    """prepare(k) makes call k's shape (not timed), call() is what is timed."""
    for k in range(WARMUP):
        prepare(k)
        call()
    torch.cuda.synchronize()
    med = []
    times = []
    for b in range(2):
        t = []
        for k in range(BLOCK):
            prepare(WARMUP + b * BLOCK + k)
            t0 = time.perf_counter()
            call()
            t.append(time.perf_counter() - t0)
        med.append(float(np.median(t)))
        times += t
    return {"median_ms": round(float(np.median(times)) * 1e3, 4), "block_medians_ms": [round(m * 1e3, 4) for m in med],
            "spread_ms": round(abs(med[0] - med[1]) * 1e3, 4)}


def run(label: str, scene: Scene, mesh_id: int) -> None:
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    mesh = scene.meshes[mesh_id]
    rest = np.asarray(mesh.positions, np.float64).copy()
    aabbs = scene.instance_local_aabbs()  # (the entity's Aabb: Bevy keeps it when a mesh is modified)

    def prepare(k):
        deform(mesh, rest, k)

    def gpu():
        r.update_meshes(scene, [mesh_id], local_aabbs=aabbs)  # returns after its one wait

    def host():
        scene.build()
        r.upload_scene(scene)  # synchronises its stream before it returns

    out = {"workload": label, "instances": len(scene.instances),
           "triangles": (scene.mesh_index(mesh_id)[3] + 2) // 3,
           "hk_update_meshes": blocks(prepare, gpu), "build_and_upload": blocks(prepare, host)}
    out["ratio"] = round(out["build_and_upload"]["median_ms"] / out["hk_update_meshes"]["median_ms"], 2)
    # the two paths agree on the last shape (primitives byte for byte)
    deform(mesh, rest, 999)
    r.update_meshes(scene, [mesh_id], local_aabbs=aabbs)
    scene.build()
    got = r.scene_array(1, np.dtype((np.void, 48)), scene.desc.primitives.count).tobytes()
    out["matches_host_build"] = got == scene.arrays()["primitives"].tobytes()
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    run("city, UV sphere 36 x 18 deformed", *city_sphere())
    run("single mesh, 20,000 triangles", *big_grid())
