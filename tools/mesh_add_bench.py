"""Cost of a mesh asset that arrives after the upload: hk_add_meshes followed by the hk_set_instances that spawns it (per
pair of calls, their two stream waits included) against the path they replace, Scene.build() + upload_scene of the
final scene (hks_build on the host, then hk_scene_upload), in one process on one machine.

The workload: the city example, and a second UV sphere (36 x 18: 1,224 triangles) added as a new mesh and spawned with
the first sphere's material.  Each side: 10 warm-up calls, then two blocks of 30; the medians of the blocks' 60 calls,
and the difference between the two block medians as the spread.  Before each timed add the context is put back on the
city scene by an upload that is not timed.  Both paths are checked to leave the same nine arrays.  One JSON line, with
the kernel-timing breakdown of one add + spawn."""
import copy
import json
import sys
import time
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
import numpy as np  # noqa: E402

from hikari_amd import HikariRenderer, examples  # noqa: E402
from hikari_amd.scene import uv_sphere_mesh  # noqa: E402

WARMUP, BLOCK = 10, 30
SIZES = (32, 48, 32, 8, 176, 32, 80, 32, 64)  # record sizes of the nine arrays, hk_scene_desc order


def blocks(prepare, call) -> dict:
    """prepare() puts the context where the call starts (not timed), call() is what is timed."""
    for _ in range(WARMUP):
        prepare()
        call()
    torch.cuda.synchronize()
    med, times = [], []
    for _ in range(2):
        t = []
        for _ in range(BLOCK):
            prepare()
            t0 = time.perf_counter()
            call()
            t.append(time.perf_counter() - t0)
        med.append(float(np.median(t)))
        times += t
    return {"median_ms": round(float(np.median(times)) * 1e3, 4), "block_medians_ms": [round(m * 1e3, 4) for m in med],
            "spread_ms": round(abs(med[0] - med[1]) * 1e3, 4)}


def arrays(r) -> list:
    counts = r.scene_counts()
    return [r.scene_array(i, np.dtype((np.void, SIZES[i])), n).tobytes() if n else b"" for i, n in enumerate(counts)]


def main() -> None:
    city, _, _ = examples.SCENES["city"]()
    city.build()
    sphere = uv_sphere_mesh(0.5, 36, 18)
    _, glow, _ = next(i for i in city.instances if i[0] == 1)  # examples.city: mesh 1 is its sphere
    final = copy.copy(city)
    final._h, final.desc = None, None
    final.meshes = list(city.meshes) + [sphere]
    at = np.eye(4)
    at[:3, 3] = (2.0, 3.0, 1.0)
    final.instances = list(city.instances) + [(len(city.meshes), glow, at)]
    previous = list(range(len(city.instances))) + [None]
    aabbs = final.instance_local_aabbs()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(city)

    def reset():
        r.upload_scene(city)

    def gpu():
        r.add_meshes([sphere])                                     # returns after its one wait
        r.set_instances(final, previous=previous, local_aabbs=aabbs)  # likewise

    def host():
        final.build()
        r.upload_scene(final)  # synchronises its stream before it returns

    out = {"workload": "city + UV sphere 36 x 18 added and spawned", "instances": len(final.instances),
           "triangles": (final.mesh_index(len(city.meshes))[3] + 2) // 3,
           "add_meshes_and_set_instances": blocks(reset, gpu), "build_and_upload": blocks(lambda: None, host)}
    out["ratio"] = round(out["build_and_upload"]["median_ms"] / out["add_meshes_and_set_instances"]["median_ms"], 2)
    host()
    want = arrays(r)
    reset()
    r.enable_kernel_timing(True)
    gpu()
    out["breakdown_ms"] = {k: round(v, 4) for k, v in r.kernel_timing().items()}
    out["matches_build_and_upload"] = arrays(r) == want
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    main()
