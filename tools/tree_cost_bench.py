"""What hk_tree_costs costs, against the only thing a caller could do before it, and what its number means in frame
time, in one process on one machine.

Call time: r.tree_costs (hk_tree_costs: one launch, one readback of 24 bytes per tree, one wait) against
hk_read_scene_array of the same node arrays plus hks_tree_cost on the host, per query, on the city example (its TLAS,
its light BVH and the sphere's BLAS; the readback side has to read the whole asset-node array, which is what
hk_read_scene_array gives), on a seeded scene of 10,000 instances (both instance trees) and on mesh_bench's single
20,000-triangle mesh (its BLAS and the two small instance trees).  Both sides give the same words, checked first.  The
two sides alternate in blocks on one context as in tools/instance_refit_bench.py: 10 warm-up calls each, then 2 x 2
blocks of 30; the median of a side's 60 calls, and the difference between its two block medians as its spread.  Beside
them hk_refit_instances on the same context, the call the query accompanies, and the query's one launch by name from
hk_kernel_timing.

Meaning: row f13's own walk-cost experiments again (city at 3840 x 2160, every instance but the ground displaced by a
tenth of, once and ten times its own size from where the trees were built), now with the cost ratio refit / rebuilt of
the TLAS and of the light BVH from the device printed beside the frame-time ratio.

    python tools/tree_cost_bench.py [calls | walk]

Every JSON line is printed and appended to profiles/tree_cost_bench.jsonl."""
import sys
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np  # noqa: E402

import refit_bench as rb  # noqa: E402
from hikari_amd import HikariRenderer, examples, tree_cost  # noqa: E402
from instance_refit_bench import SEED, jitter, seeded_scene  # noqa: E402
from mesh_bench import big_grid, city_sphere  # noqa: E402

OUT = ROOT / "profiles" / "tree_cost_bench.jsonl"
rb.OUT = OUT  # (refit_bench.emit appends there)
NODE = np.dtype((np.void, 32))


def known_slice_id(scene, mesh_id: int) -> int:
    """Where the mesh stands among the context's known slices after the upload: the distinct meshes in the order in
    which the instances first carry them."""
    order = []
    for mesh, _, _ in scene.instances:
        if mesh not in order:
            order.append(mesh)
    return order.index(mesh_id)


def query_calls(label: str, scene, mesh_ids) -> None:
    scene.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    ids = [known_slice_id(scene, m) for m in mesh_ids]
    slices = [scene.mesh_index(m)[2:4] for m in mesh_ids]
    counts = r.scene_counts()
    models0, aabbs = scene.instance_models(), scene.instance_local_aabbs()

    def query():
        return r.tree_costs(ids)

    def readback():
        asset = r.scene_array(2, NODE, counts[2]) if slices else None
        return {"tlas": tree_cost(r.scene_array(5, NODE, counts[5])),
                "lights": tree_cost(r.scene_array(7, NODE, counts[7])),
                "meshes": [tree_cost(asset[n0:n0 + nc]) for n0, nc in slices]}

    r.update_instances(jitter(models0, 0), aabbs, refit=True)  # (kept trees, as where the query is used)
    assert query() == readback()
    nodes = counts[5] + counts[7] + sum(int(nc) for _, nc in slices)
    out = {"measure": "query time", "workload": label, "instances": len(models0), "emitters": counts[8],
           "nodes_costed": int(nodes), "asset_nodes_read_back": int(counts[2]) if slices else 0}
    out.update(rb.alternating(lambda k: None, {"hk_tree_costs": query, "readback_and_hks_tree_cost": readback}))
    a, b = out["hk_tree_costs"], out["readback_and_hks_tree_cost"]
    out["ratio_readback_over_query"] = round(b["median_ms"] / a["median_ms"], 2)
    out["faster_by_more_than_both_spreads"] = b["median_ms"] - a["median_ms"] > a["spread_ms"] + b["spread_ms"]
    state = {}

    def prepare(k):
        state["m"] = jitter(models0, k)

    out.update(rb.alternating(prepare, {"hk_refit_instances": lambda: r.update_instances(state["m"], aabbs, refit=True)}))
    out["query_kernel_ms_per_call"] = rb.timed_kernels(r, lambda k: None, query)
    rb.emit(out)
    r.close()


def meaning() -> None:
    scene, cam, lights = examples.SCENES["city"]()
    scene.build()
    size = (3840, 2160)
    models0, aabbs = scene.instance_models(), scene.instance_local_aabbs()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(scene)
    r.resize(*size, 1.0)

    def displaced(factor):  # tools/instance_refit_bench.py walk_cost's, with its seeds
        rng = np.random.default_rng([SEED, int(factor * 10)])
        m = models0.copy()
        extent = np.array([2.0 * np.linalg.norm(np.abs(m[k].reshape(4, 4).T[:3, :3]) @ aabbs[k, 3:6])
                           for k in range(len(m))])
        for k in range(len(m)):
            if k == int(np.argmax(extent)):  # the ground plane stays
                continue
            d = rng.normal(size=3)
            m[k, 12:15] += (factor * extent[k] * d / np.linalg.norm(d)).astype(np.float32)
        return m

    for factor in (0.1, 1.0, 10.0):
        models = displaced(factor)
        r.update_instances(models0, aabbs)  # the trees of the uploaded layout
        r.update_instances(models, aabbs, refit=True)
        kept_cost = r.tree_costs()
        kept = rb.frame_ms(r, cam, lights, size)
        r.update_instances(models, aabbs)
        rebuilt_cost = r.tree_costs()
        rebuilt = rb.frame_ms(r, cam, lights, size)
        ratio = {k: round(kept_cost[k].total() / rebuilt_cost[k].total(), 3) for k in ("tlas", "lights")}
        rb.emit({"measure": "cost ratio beside frame ratio", "workload": "city, 3840 x 2160",
                 "models": f"every instance displaced by {factor} x its own size",
                 "cost_refit": {k: round(kept_cost[k].total(), 3) for k in ratio},
                 "cost_rebuilt": {k: round(rebuilt_cost[k].total(), 3) for k in ratio},
                 "cost_ratio_refit_over_rebuilt": ratio,
                 "frame_ms_refit": kept["ms_per_frame"], "frame_ms_rebuilt": rebuilt["ms_per_frame"],
                 "frame_spread_ms": [kept["spread_ms"], rebuilt["spread_ms"]],
                 "frame_ratio_refit_over_rebuilt": round(kept["ms_per_frame"] / rebuilt["ms_per_frame"], 3)})
    r.close()


if __name__ == "__main__":
    what = sys.argv[1:] or ["calls", "walk"]
    if "calls" in what:
        query_calls("city: TLAS, light BVH, the sphere's BLAS", *(lambda s, m: (s, [m]))(*city_sphere()))
        query_calls("seeded quads, 10,000 instances: TLAS, light BVH", seeded_scene(), [])
        query_calls("single mesh of 20,000 triangles and a lamp: its BLAS, TLAS, light BVH",
                    *(lambda s, m: (s, [m]))(*big_grid()))
    if "walk" in what:
        meaning()
