"""Cost of a changed instance set: hk_set_instances on the GPU (per call, its one stream wait included) against the
path it replaces, Scene.build() + upload_scene (hks_build on the host, then hk_scene_upload), in one process on one
machine.  The instance descs, models and local AABBs are made before the clock starts.

The workload: the city example (1,130 instances), its emissive sphere alternately despawned and spawned back.  Each
side: 10 warm-up calls, then two blocks of 30; the median of the blocks' 60 calls, and the difference between the two
block medians as the spread.  Both paths are checked to leave the same arrays.  One JSON line."""
import copy
import json
import sys
import time
from pathlib import Path

import torch  # noqa: F401  (import before the HIP library, see bench.py)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "bevy-hikari_amd"))
import numpy as np  # noqa: E402

from hikari_amd import HikariRenderer, examples, instance_descs  # noqa: E402

WARMUP, BLOCK = 10, 30
SIZES = {3: 8, 4: 176, 5: 32, 7: 32, 8: 64}  # the arrays hk_set_instances rebuilds: bytes per record


def city_pair():
    """(the city, the city without its emissive sphere, each one's `previous` map when set after the other)."""
    full, _, _ = examples.SCENES["city"]()
    lamp = [k for k, (mesh, _, _) in enumerate(full.instances) if mesh == 1]  # examples.city: mesh 1 is the sphere
    assert lamp == [1] and full.materials[full.instances[1][1]].emissive[3] > 0
    less = copy.copy(full)
    less._h, less.desc = None, None
    less.instances = [inst for k, inst in enumerate(full.instances) if k != lamp[0]]
    n = len(full.instances)
    to_less = [k for k in range(n) if k != lamp[0]]
    to_full = [None if k == lamp[0] else (k if k < lamp[0] else k - 1) for k in range(n)]
    return full, less, to_full, to_less


def blocks(call) -> dict:
    """call(k) is what is timed."""
    for k in range(WARMUP):
        call(k)
    torch.cuda.synchronize()
    med, times = [], []
    for b in range(2):
        t = []
        for k in range(BLOCK):
            t0 = time.perf_counter()
            call(WARMUP + b * BLOCK + k)
            t.append(time.perf_counter() - t0)
        med.append(float(np.median(t)))
        times += t
    return {"median_ms": round(float(np.median(times)) * 1e3, 4), "block_medians_ms": [round(m * 1e3, 4) for m in med],
            "spread_ms": round(abs(med[0] - med[1]) * 1e3, 4)}


def device_arrays(r, desc) -> bytes:
    counts = r.scene_counts()
    return b"".join(r.scene_array(i, np.dtype((np.void, size)), counts[i]).tobytes() for i, size in SIZES.items()
                    if i != 5 and counts[i])  # (the device TLAS carries leaf boxes the host's does not)


def run() -> None:
    full, less, to_full, to_less = city_pair()
    full.build()
    r = HikariRenderer(0)
    r.set_noise()
    r.upload_scene(full)
    # call k leaves `less` when k is even and `full` when it is odd
    targets = [(less, to_less, less.instance_local_aabbs()), (full, to_full, full.instance_local_aabbs())]

    # what a caller hands to the C call, made before the clock starts: the instance descs, models and local AABBs
    args = []
    for scene, previous, aabbs in targets:
        m = np.ascontiguousarray(scene.instance_models(), np.float32)
        a = np.ascontiguousarray(aabbs, np.float32)
        args.append((instance_descs(scene, previous), m, a, len(m)))

    def gpu(k):
        descs, m, a, n = args[k % 2]
        rc = r._L.hk_set_instances(r.ctx, descs, m.ctypes.data, a.ctypes.data, n, None, None)  # returns after its one wait
        assert rc == 0, r._L.hk_last_error(r.ctx).decode()

    def host(k):
        scene = targets[k % 2][0]
        scene.build()
        r.upload_scene(scene)  # synchronises its stream before it returns

    out = {"workload": "city, emissive sphere despawned / spawned", "instances": len(full.instances),
           "hk_set_instances": blocks(gpu), "build_and_upload": blocks(host)}
    out["ratio"] = round(out["build_and_upload"]["median_ms"] / out["hk_set_instances"]["median_ms"], 2)
    # the two paths leave the same arrays, on both sides of the toggle (the host path ended on `full`)
    same = []
    for k in (0, 1):
        host(k)
        want = device_arrays(r, targets[k % 2][0].desc)
        host(k + 1)
        gpu(k)
        same.append(device_arrays(r, targets[k % 2][0].desc) == want and r.scene_counts() == [
            getattr(targets[k % 2][0].desc, a).count for a in ("vertices", "primitives", "asset_nodes", "alias_table",
                                                                "instances", "instance_nodes", "materials",
                                                                "emissive_nodes", "emissives")])
    out["matches_host_build"] = all(same)
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    run()
