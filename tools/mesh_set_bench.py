"""Cost of a mesh asset that is removed or replaced by one of another topology after the upload: one hk_set_meshes call
(its two stream waits included) against the path it replaces, Scene.build() + upload_scene of the final scene (hks_build
on the host, then hk_scene_upload), in one process on one machine.

The workload: the city example, and its UV sphere (36 x 18: 1,224 triangles) (a) removed with its instance, (b) replaced
at its position by a 48 x 24 sphere, its instance keeping its place in the set.  Each side: 10 warm-up calls, then two
blocks of 30; the medians of the blocks' 60 calls, and the difference between the two block medians as the spread.
Before each timed hk_set_meshes the context is put back on the city scene by an upload that is not timed.  Both paths are
checked to leave the same nine arrays.  One JSON line, with the kernel-timing breakdown of one call of each kind
(move_meshes: k_move_mesh_slices alone) and the bytes the move reads and writes."""
import copy
import json
import sys
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from hikari_amd import HikariRenderer, examples  # noqa: E402
from hikari_amd.scene import uv_sphere_mesh  # noqa: E402
from mesh_add_bench import SIZES, arrays, blocks  # noqa: E402

SPHERE = 1  # examples.city: mesh 1 is its sphere


def variant(city, mesh):
    """(final scene, entries, previous): city with its sphere dropped (mesh None) or replaced by `mesh`."""
    final = copy.copy(city)
    final._h, final.desc = None, None
    entries, final.meshes, at = [], [], {}
    for j, m in enumerate(city.meshes):
        if j == SPHERE and mesh is None:
            continue
        at[j] = len(final.meshes)
        final.meshes.append(mesh if j == SPHERE else m)
        entries.append(mesh if j == SPHERE else (city.mesh_index(j), len(m.positions)))
    final.instances, previous = [], []
    for i, (j, mat, model) in enumerate(city.instances):
        if j in at:
            final.instances.append((at[j], mat, model))
            previous.append(i)
    return final, entries, previous


def main() -> None:
    city, _, _ = examples.SCENES["city"]()
    city.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(city)
    out = {"workload": "city, its UV sphere 36 x 18 removed / replaced by 48 x 24", "instances": len(city.instances)}
    for label, mesh in (("remove", None), ("replace", uv_sphere_mesh(0.5, 48, 24))):
        final, entries, previous = variant(city, mesh)
        aabbs = final.instance_local_aabbs()

        def reset():
            r.upload_scene(city)

        def gpu():
            r.set_meshes(final, entries, previous=previous, local_aabbs=aabbs)  # returns after its waits

        def host():
            final.build()
            r.upload_scene(final)  # synchronises its stream before it returns

        res = {"set_meshes": blocks(reset, gpu), "build_and_upload": blocks(lambda: None, host)}
        res["ratio"] = round(res["build_and_upload"]["median_ms"] / res["set_meshes"]["median_ms"], 2)
        host()
        want = arrays(r)
        reset()
        r.enable_kernel_timing(True)
        gpu()
        res["breakdown_ms"] = {k: round(v, 4) for k, v in r.kernel_timing().items()}
        r.enable_kernel_timing(False)
        res["matches_build_and_upload"] = arrays(r) == want
        counts = r.scene_counts()
        kept = sum(c * s for c, s in zip(counts[:3], SIZES[:3]))
        if mesh is not None:
            v, p, n0, nc = final.mesh_index(SPHERE)
            kept -= len(mesh.positions) * SIZES[0] + (nc + 2) // 3 * SIZES[1] + nc * SIZES[2]
        res["move_bytes_read_and_written"] = 2 * kept
        out[label] = res
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    main()
