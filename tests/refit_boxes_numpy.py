"""The refit over given shape boxes restated in numpy, from its text (include/hk_refit.h's second half, the comment of
hikari_scene.h hks_refit_boxes) and without the header's bodies: what tests/test_instance_refit_independent.py
holds hks_refit_boxes and Scene.refitted_instances against.

A tree is a bvh-0.7.1 flatten (NODE_DT records) over `count` shapes.  A leaf has entry >= 0x80000000, its payload the
shape's index; an entry node i carries the box of the subtree stored in (i, exit).  The refit leaves every leaf and every
index as it is and gives entry node i

    min[c] = the least S[t][c] over the leaves t in (i, exit), a NaN skipped, -0 below +0
    max[c] = the greatest S[t][3 + c] likewise, +0 above -0; with nothing left, +inf / -inf

The shapes of the two instance-level trees come from the records:
    TLAS       S[t] = words 0..2 and 4..6 of instance t (its world box)
    light BVH  S[e] = position - radius, position + radius of emitter e (words 4..6 and 7), one float32 operation each
and every node_index (instance word 7, emitter word 13) is the one the kept tree was built with.

Each entry node GATHERS the shapes of the leaves in its range and reduces over them; the host function's recurrence (a
node's box from its two children's) is not used.  The keyword arguments switch on one misreading each."""
from __future__ import annotations

import numpy as np

LEAF = 0x80000000
NODE_DT = np.dtype([("min", "<f4", 3), ("entry", "<u4"), ("max", "<f4", 3), ("exit", "<u4")])


def _bound(values, greatest=False, nan_propagates=False):
    """One bound from a range's gathered values (m,)."""
    values = np.asarray(values, np.float32)
    nan = np.isnan(values)
    if nan.any():
        if nan_propagates:  # the misreading
            return np.float32(np.nan)
        values = values[~nan]
    if not len(values):
        return np.float32(-np.inf if greatest else np.inf)
    v = values.max() if greatest else values.min()
    if v != 0.0:
        return np.float32(v)
    negative = np.signbit(values[values == 0.0])
    if greatest:
        return np.float32(-0.0) if negative.all() else np.float32(0.0)
    return np.float32(-0.0) if negative.any() else np.float32(0.0)


def refit(nodes, boxes, *, closed_range=False, nan_propagates=False):
    """A copy of `nodes` (NODE_DT) refit over `boxes` (count, 6).  Misreadings: closed_range: the range is [i, exit), so
    node i's own stored box joins in; nan_propagates: a NaN component makes the bounds above it NaN."""
    nodes = np.array(nodes, NODE_DT)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
    out = nodes.copy()
    leaf = nodes["entry"] >= LEAF
    for i in np.flatnonzero(~leaf):
        inside = np.arange(i + 1, int(nodes["exit"][i]))
        shapes = (nodes["entry"][inside][leaf[inside]] - LEAF).astype(np.int64)  # the gather, in leaf order
        lo, hi = boxes[shapes, 0:3], boxes[shapes, 3:6]
        if closed_range:
            lo, hi = np.vstack([nodes["min"][i][None], lo]), np.vstack([nodes["max"][i][None], hi])
        for c in range(3):
            out["min"][i][c] = _bound(lo[:, c], False, nan_propagates)
            out["max"][i][c] = _bound(hi[:, c], True, nan_propagates)
    return out


def instance_words(records) -> np.ndarray:
    return np.frombuffer(np.ascontiguousarray(records).tobytes(), np.uint32).reshape(-1, 44).copy()


def emitter_words(records) -> np.ndarray:
    return np.frombuffer(np.ascontiguousarray(records).tobytes(), np.uint32).reshape(-1, 16).copy()


def tlas_shapes(instances) -> np.ndarray:
    f = instance_words(instances).view(np.float32)
    return np.concatenate([f[:, 0:3], f[:, 4:7]], axis=1)


def light_shapes(emissives, instances=None, from_instance_box=False) -> np.ndarray:
    """The emitters' sphere boxes.  Misreading from_instance_box: the box of the emitter's instance instead."""
    e = emitter_words(emissives)
    if from_instance_box:
        return tlas_shapes(instances)[e[:, 8]]
    f = e.view(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([f[:, 4:7] - f[:, 7:8], f[:, 4:7] + f[:, 7:8]], axis=1).astype(np.float32)


def refitted_scene(arrays0: dict, arrays1: dict, *, from_instance_box=False, node_index_of_scene1=False, **misreadings):
    """What an instance refit leaves, from the arrays of the scene before (arrays0) and of the scene as the host builds
    it for the new models (arrays1), each {"instances", "instance_nodes", "emissives", "emissive_nodes"}: the same four
    arrays after the call.  Misreading node_index_of_scene1: the records keep the rebuilt scene's node_index."""
    inst, em = instance_words(arrays1["instances"]), emitter_words(arrays1["emissives"])
    if not node_index_of_scene1:
        inst[:, 7] = instance_words(arrays0["instances"])[:, 7]
        if len(em):
            em[:, 13] = emitter_words(arrays0["emissives"])[:, 13]
    out = {"instances": inst, "emissives": em,
           "instance_nodes": refit(arrays0["instance_nodes"], tlas_shapes(inst), **misreadings),
           "emissive_nodes": np.zeros(0, NODE_DT)}
    if len(em):
        out["emissive_nodes"] = refit(arrays0["emissive_nodes"], light_shapes(em, inst, from_instance_box), **misreadings)
    return out


def words(nodes) -> np.ndarray:
    """The stored words of a node array, for comparisons that tell -0 from +0 and one NaN from another."""
    return np.frombuffer(np.ascontiguousarray(nodes).tobytes(), np.uint32).reshape(-1, 8)
