"""Cost of posing a mesh with morph targets: hk_morph_meshes, hk_morph_meshes_refit and hk_morph_meshes_refit_all on the GPU
(per call, its one stream wait included; the host sends one weight vector, and a joint palette under a skin) against what
a caller had before them: hks_morph_vertices (and hks_skin_vertices) and the bounds on the host, then hk_update_meshes,
hk_refit_meshes or hk_refit_meshes_all with the posed positions and normals.  One process, one context per workload.

Workloads: the city example's UV sphere (703 vertices) with 8 targets, 2 of them active; a single mesh of 20,000
triangles (10,201 vertices) with 4, 16 and 64 targets, half of them active, with normals and normal deltas (24 B per
vertex per target) and without either (12 B), and once with 16 targets under a 32-joint skin.

Method (tools/skin_bench.py's, the sides interleaved): 10 warm-up calls per side, then the two sides alternate in blocks
of 30 calls, two blocks each; a side's figure is the median of its 60 calls and its spread the difference of its two
block medians.  One JSON line per workload, with k_morph_vertices alone from the timed span refit_morph_vertices (a
separate, timed run of 30 calls), the bytes it has to read and write, and the fraction of the 8 TB/s HBM peak that gives.
--kernel-only prints that part alone, and --batch N records N as "morph_batch" in every line: for library builds with
another MORPH_BATCH (csrc/hk_launch.h), which the tool is told about, since the constant is compiled in.  The lines of
profiles/morph_bench.jsonl: one full run at the committed batch, then kernel-only runs at 1, 2, 4 and 8."""
import json
import sys
import time
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np  # noqa: E402

from hikari_amd import HikariRenderer, Mesh, Morph, morph_vertices  # noqa: E402
from mesh_bench import big_grid, city_sphere  # noqa: E402
from skin_bench import palette, rig  # noqa: E402

WARMUP, BLOCK = 10, 30
HBM_PEAK = 8.0e12  # bytes per second (spec)
BATCH = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else None


def alternate(prepare, a, b) -> tuple:
    """(side a, side b): prepare(k) makes call k's pose (not timed); the sides take turns block by block."""
    for side in (a, b):
        for k in range(WARMUP):
            prepare(k)
            side()
    torch.cuda.synchronize()
    t = {0: [[], []], 1: [[], []]}
    for blk in range(2):
        for s, side in enumerate((a, b)):
            for k in range(BLOCK):
                prepare(WARMUP + blk * BLOCK + k)
                t0 = time.perf_counter()
                side()
                t[s][blk].append(time.perf_counter() - t0)

    def figure(x):
        med = [float(np.median(v)) for v in x]
        return {"median_ms": round(float(np.median(x[0] + x[1])) * 1e3, 4), "block_medians_ms": [round(m * 1e3, 4) for m in med],
                "spread_ms": round(abs(med[0] - med[1]) * 1e3, 4)}
    return figure(t[0]), figure(t[1])


def targets(mesh, count: int, normals: bool, rng) -> None:
    """Smooth seeded bumps: target t pushes the vertices near its own centre along z and tilts their normals."""
    p = np.asarray(mesh.positions, np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    dp = np.zeros((count, len(p), 3), np.float32)
    dn = np.zeros((count, len(p), 3), np.float32) if normals else None
    for t in range(count):
        c = lo + rng.uniform(0.1, 0.9, 3) * (hi - lo)
        r2 = ((p - c) ** 2).sum(axis=1) / (0.05 * float(((hi - lo) ** 2).sum()) + 1e-12)
        bump = np.exp(-r2)
        dp[t] = (bump[:, None] * rng.normal(size=3) * 0.05 * np.linalg.norm(hi - lo)).astype(np.float32)
        if normals:
            dn[t] = (bump[:, None] * rng.normal(size=3) * 0.2).astype(np.float32)
    mesh.morph = Morph(dp, dn)


def weights(count: int, active: int, k: int) -> np.ndarray:
    """Call k's weights: `active` targets, spread over the list, swing with a phase; the others are zero."""
    w = np.zeros(count, np.float32)
    on = np.linspace(0, count - 1, active).round().astype(np.int64) if active > 1 else np.array([count // 2])
    w[on] = (0.5 + 0.45 * np.sin(0.37 * k + 0.9 * np.arange(len(on)))).astype(np.float32)
    return w


def run(label: str, scene, mesh_id: int, count: int, active: int, normals: bool, joints: int = 0,
        kernel_only: bool = False) -> None:
    rng = np.random.default_rng(7)
    mesh = scene.meshes[mesh_id]
    targets(mesh, count, normals, rng)
    if joints:
        rig(mesh, joints, rng)
    keep = () if normals else (mesh_id,)
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    r.set_mesh_morphs(scene, [mesh_id], keep)
    if joints:
        r.set_mesh_skins(scene, [mesh_id], keep)
    source = mesh if normals else Mesh(mesh.positions, None, mesh.uvs, mesh.indices, mesh.topology, mesh.skin, mesh.morph)
    aabbs = scene.instance_local_aabbs()
    rows = [i for i, (m, _, _) in enumerate(scene.instances) if m == mesh_id]
    state = {}

    def prepare(k):
        w = weights(count, active, k)
        state["pose"] = (w, palette(joints, k)) if joints else w

    def device(refit):
        return lambda: r.morph_meshes(scene, {mesh_id: state["pose"]}, local_aabbs=aabbs, refit=refit)

    def host_posed():
        w, j = state["pose"] if joints else (state["pose"], None)
        s = scene.posed({})
        s.meshes[mesh_id], box = morph_vertices(source, w, j, aabb=True)  # (no normals: hk_update_meshes keeps them)
        a = aabbs.copy()
        a[rows] = box
        return s, a

    def host(refit):
        def call():
            s, a = host_posed()
            r.update_meshes(s, [mesh_id], local_aabbs=a, refit=refit)
        return call

    nv = len(mesh.positions)
    per = 24 if normals else 12
    out = {"workload": label, "instances": len(scene.instances), "vertices": nv,
           "triangles": (scene.mesh_index(mesh_id)[3] + 2) // 3, "targets": count, "active": active,
           "normals": normals, "joints": joints}
    if BATCH is not None:
        out["morph_batch"] = BATCH
    if kernel_only:
        out["kernel_only"] = True
    if not kernel_only:
        for name, refit, theirs in (("hk_morph_meshes", False, "hk_update_meshes"),
                                    ("hk_morph_meshes_refit", True, "hk_refit_meshes"),
                                    ("hk_morph_meshes_refit_all", "all", "hk_refit_meshes_all")):
            d, h = alternate(prepare, device(refit), host(refit))
            out[name] = d
            out["hks_morph_vertices_and_" + theirs] = h
            out["ratio_" + name] = round(h["median_ms"] / d["median_ms"], 3)
        # the paths agree on the last pose (vertices, primitives and instance records byte for byte)
        prepare(999)
        device(False)()
        s, _ = host_posed()
        pm = s.meshes[mesh_id]
        if pm.normals is None:
            s.meshes[mesh_id] = Mesh(pm.positions, mesh.normals, pm.uvs, pm.indices, pm.topology)
        s.build()
        out["matches_host_build"] = all(
            r.scene_array(i, np.dtype((np.void, size)), getattr(s.desc, name).count).tobytes() == s.arrays()[name].tobytes()
            for i, name, size in ((0, "vertices", 32), (1, "primitives", 48), (4, "instances", 176)))
    for k in range(WARMUP):
        prepare(k)
        device(True)()
    r.enable_kernel_timing(True)
    for k in range(BLOCK):
        prepare(k)
        device(True)()
    r.sync()
    spans = r.kernel_timing()
    out["kernel_ms_per_call"] = {k: round(v, 4) for k, v in spans.items()}
    # what k_morph_vertices must move: the active deltas, the base, the rig and the palette in; the staged streams out
    moved = active * nv * per + nv * per + (nv * 24 + joints * 64 if joints else 0) + nv * per
    ms = spans.get("refit_morph_vertices", 0.0)
    out["k_morph_vertices"] = {"ms": round(ms, 4), "bytes": moved,
                               "hbm_peak_fraction": round(moved / (ms * 1e-3) / HBM_PEAK, 4) if ms else None}
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    kernel_only = "--kernel-only" in sys.argv
    if not kernel_only:
        run("city, UV sphere 36 x 18, 8 targets, 2 active", *city_sphere(), 8, 2, True)
    for count in (4, 16, 64):
        for normals in (True, False):
            run(f"single mesh, 20,000 triangles, {count} targets, {count // 2} active, "
                f"{'with' if normals else 'without'} normals", *big_grid(), count, count // 2, normals,
                kernel_only=kernel_only)
    run("single mesh, 20,000 triangles, 16 targets, 8 active, with normals, under 32 joints", *big_grid(), 16, 8, True,
        joints=32, kernel_only=kernel_only)
