"""Cost of posing a skinned mesh: hk_skin_meshes on the GPU (per call, its one stream wait included; the host sends one
joint palette) against the path it replaces (hks_skin_vertices and the posed bounds on the host, then hk_update_meshes
with the posed positions and normals), and against Scene.build() + upload_scene of the posed scene, in one process on
one machine.

Two workloads: the city example's emissive UV sphere (36 x 18) on a two-joint rig, and a single mesh of 20,000 triangles
on 32 joints.  Each side: 10 warm-up calls, then two blocks of 30; the medians of the blocks' 60 calls, and the
difference between the two block medians as the spread.  One JSON line per workload, with the device path's per-kernel
times from hk_kernel_timing (a separate, timed run of 30 calls)."""
import json
import sys
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np  # noqa: E402

from hikari_amd import HikariRenderer, Skin, skin_vertices  # noqa: E402
from mesh_bench import big_grid, blocks, city_sphere  # noqa: E402


def rig(mesh, joints: int, rng) -> None:
    """Joints spread along x; each vertex follows the two nearest and two seeded others with small weights."""
    p = np.asarray(mesh.positions, np.float64)
    lo, hi = p[:, 0].min(), p[:, 0].max()
    t = (p[:, 0] - lo) / max(hi - lo, 1e-9) * (joints - 1)
    a = np.clip(np.floor(t).astype(np.int64), 0, joints - 1)
    b = np.clip(a + 1, 0, joints - 1)
    f = (t - a).astype(np.float32)
    ix = np.stack([a, b, rng.integers(0, joints, len(p)), rng.integers(0, joints, len(p))], axis=1).astype(np.uint16)
    w = np.stack([(1 - f) * 0.9, f * 0.9, np.full(len(p), 0.06, np.float32), np.full(len(p), 0.04, np.float32)], axis=1)
    mesh.skin = Skin(ix, w.astype(np.float32), joints)


def palette(joints: int, k: int) -> np.ndarray:
    """Call k's pose: every joint turns about z and sways, by a phase that travels along the chain."""
    out = np.empty((joints, 16), np.float32)
    for j in range(joints):
        a = 0.35 * np.sin(0.37 * k + 0.6 * j)
        m = np.eye(4)
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = (0.0, 0.05 * np.cos(0.21 * k + j), 0.03 * np.sin(0.3 * k + 0.5 * j))
        out[j] = m.T.reshape(16)
    return out


def run(label: str, scene, mesh_id: int, joints: int) -> None:
    rng = np.random.default_rng(7)
    rig(scene.meshes[mesh_id], joints, rng)
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    r.set_mesh_skins(scene, [mesh_id])
    aabbs = scene.instance_local_aabbs()
    rows = [i for i, (m, _, _) in enumerate(scene.instances) if m == mesh_id]
    state = {}

    def prepare(k):
        state["joints"] = palette(joints, k)

    def device():
        r.skin_meshes(scene, {mesh_id: state["joints"]}, local_aabbs=aabbs)  # returns after its one wait

    def host_posed():
        posed, box = skin_vertices(scene.meshes[mesh_id], state["joints"], aabb=True)
        s = scene.posed({})
        s.meshes[mesh_id] = posed
        a = aabbs.copy()
        a[rows] = box
        return s, a

    def host():
        s, a = host_posed()
        r.update_meshes(s, [mesh_id], local_aabbs=a)

    def rebuild():
        s, _ = host_posed()
        s.build()
        r.upload_scene(s)  # synchronises its stream before it returns

    out = {"workload": label, "instances": len(scene.instances), "joints": joints,
           "vertices": len(scene.meshes[mesh_id].positions), "triangles": (scene.mesh_index(mesh_id)[3] + 2) // 3,
           "hk_skin_meshes": blocks(prepare, device), "host_skin_and_hk_update_meshes": blocks(prepare, host),
           "build_and_upload": blocks(prepare, rebuild)}
    out["ratio_to_host_skin"] = round(out["host_skin_and_hk_update_meshes"]["median_ms"] / out["hk_skin_meshes"]["median_ms"], 2)
    out["ratio_to_build_and_upload"] = round(out["build_and_upload"]["median_ms"] / out["hk_skin_meshes"]["median_ms"], 2)
    # the paths agree on the last pose (vertices, primitives and instance records byte for byte)
    prepare(999)
    r.upload_scene(scene)
    r.set_mesh_skins(scene, [mesh_id])
    device()
    s, _ = host_posed()
    s.build()
    out["matches_host_build"] = all(
        r.scene_array(i, np.dtype((np.void, size)), getattr(s.desc, name).count).tobytes() == s.arrays()[name].tobytes()
        for i, name, size in ((0, "vertices", 32), (1, "primitives", 48), (4, "instances", 176)))
    r.enable_kernel_timing(True)
    for k in range(30):
        prepare(k)
        device()
    r.sync()
    out["kernel_ms_per_call"] = {k: round(v, 4) for k, v in r.kernel_timing().items()}
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    run("city, UV sphere 36 x 18 on 2 joints", *city_sphere(), 2)
    run("single mesh, 20,000 triangles on 32 joints", *big_grid(), 32)
