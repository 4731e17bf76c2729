"""The tree cost restated in numpy, from its text (the comment of include/hk_cost.h, hikari_amd.h hk_tree_cost, DESIGN
§3) and without the header's bodies: what tests/test_tree_cost_independent.py holds hks_tree_cost against, and with it
the device (tests/test_gpu_tree_cost.py compares hk_tree_costs with hks_tree_cost).

A tree is a bvh-0.7.1 flatten (NODE_DT records) of 3k - 2 nodes over k shapes.  A leaf has entry >= 0x80000000; an entry
node i carries the box of the subtree stored in (i, exit).  With float32 arithmetic, one rounding per operation:

    e[c]   = max[c] - min[c]
    H      = (e.x * e.y + e.y * e.z) + e.z * e.x
    root   = per component the least min / greatest max of nodes 0 and nodes[0].exit, a NaN skipped (+inf / -inf with
             nothing left), -0 below +0;  R = H(root)
    r      = H(node) / R
    q      = 2^32 where r >= 1, trunc(r * 2^32) where 0 < r < 1, else 0 (a NaN compares false)
    leaf   = the sum of q over the entry nodes with exit - i == 2
    inner  = the sum of q over the other entry nodes
    entries, root_half_area = the number of entry nodes, R;  k == 1 or no node: all zero

All entry nodes are weighed at once, as arrays; the host function's loop is not used.  The keyword arguments switch on
one misreading each."""
from __future__ import annotations

import numpy as np

LEAF = 0x80000000
NODE_DT = np.dtype([("min", "<f4", 3), ("entry", "<u4"), ("max", "<f4", 3), ("exit", "<u4")])
F = np.float32


def half_area(mn, mx, *, volume=False, right_to_left=False):
    """H of boxes (.., 3) float32.  Misreadings: volume: e.x * e.y * e.z; right_to_left: e.x*e.y + (e.y*e.z + e.z*e.x)."""
    with np.errstate(all="ignore"):
        e = (np.asarray(mx, F) - np.asarray(mn, F)).astype(F)
        x, y, z = e[..., 0], e[..., 1], e[..., 2]
        if volume:
            return ((x * y).astype(F) * z).astype(F)
        if right_to_left:
            return ((x * y).astype(F) + ((y * z).astype(F) + (z * x).astype(F)).astype(F)).astype(F)
        return (((x * y).astype(F) + (y * z).astype(F)).astype(F) + (z * x).astype(F)).astype(F)


def _bound(values, greatest):
    v = np.asarray(values, F)
    v = v[~np.isnan(v)]
    if not len(v):
        return F(-np.inf if greatest else np.inf)
    return F(v.max() if greatest else v.min())  # (a zero's sign does not reach H: x - (-0) == x - (+0) unless x is 0 too)


def root_box(nodes, *, node0_only=False):
    """(min, max) of the root of a tree of k >= 2 shapes.  Misreading node0_only: node 0's box alone."""
    tops = [0] if node0_only else [0, int(nodes["exit"][0])]
    mn = np.array([_bound(nodes["min"][tops, c], False) for c in range(3)], F)
    mx = np.array([_bound(nodes["max"][tops, c], True) for c in range(3)], F)
    return mn, mx


def tree_cost(nodes, *, node0_only=False, volume=False, round_nearest=False, right_to_left=False,
              leaf_entries_into_inner=False) -> dict:
    """{"inner", "leaf", "entries" (Python ints), "root_half_area" (float32)} of a flatten.  Misreadings: node0_only,
    volume, right_to_left (above); round_nearest: q rounded to the nearest integer instead of truncated;
    leaf_entries_into_inner: the entry nodes over one leaf counted into `inner`."""
    nodes = np.asarray(nodes, NODE_DT)
    out = {"inner": 0, "leaf": 0, "entries": 0, "root_half_area": F(0.0)}
    if len(nodes) <= 1:
        return out
    area = dict(volume=volume, right_to_left=right_to_left)
    R = F(half_area(*root_box(nodes, node0_only=node0_only), **area))
    at = np.flatnonzero(nodes["entry"] < LEAF)
    with np.errstate(all="ignore"):
        r = (half_area(nodes["min"][at], nodes["max"][at], **area) / R).astype(F)
        scaled = (r * F(4294967296.0)).astype(F).astype(np.float64)  # (exact: a power of two)
    below = (r > 0) & (r < 1)
    part = np.where(below, scaled, 0.0)
    part = np.rint(part) if round_nearest else np.trunc(part)
    q = [1 << 32 if x >= 1 else int(p) for x, p in zip(r.tolist(), part.tolist())]  # (NaN >= 1 is False; its part is 0)
    over_leaf = (nodes["exit"][at].astype(np.int64) - at) == 2
    if leaf_entries_into_inner:
        over_leaf = np.zeros(len(at), bool)
    out["leaf"] = sum(x for x, o in zip(q, over_leaf.tolist()) if o)
    out["inner"] = sum(x for x, o in zip(q, over_leaf.tolist()) if not o)
    out["entries"] = len(at)
    out["root_half_area"] = R
    return out


def same(got, want) -> bool:
    """A hikari_amd.TreeCost (or anything with its fields) equals a tree_cost() dict in every field, R bit for bit (NaN
    for NaN of any payload)."""
    a, b = F(got.root_half_area), F(want["root_half_area"])
    r_same = (np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()
    return bool(r_same) and (int(got.inner), int(got.leaf), int(got.entries)) == (want["inner"], want["leaf"],
                                                                                 want["entries"])


def known_slices(instances) -> list:
    """The distinct (offset, length) node ranges the hk_instance records (176 bytes each) carry, in the order of their
    first use: the context's known slices after hk_scene_upload, which hk_tree_costs' mesh ids index."""
    w = np.frombuffer(np.ascontiguousarray(instances).tobytes(), np.uint32).reshape(-1, 44)
    seen = []
    for mesh in w[:, 40:44].tolist():
        if mesh not in seen:
            seen.append(mesh)
    return [(m[2], m[3]) for m in seen]


# ------------------------------------------------------------------ hand-made trees
def flat_tree(boxes, shape=None) -> np.ndarray:
    """A well-formed flatten over `boxes` ((k, 6): min xyz, max xyz) with the topology `shape`: a nested pair of shape
    indices, default a balanced split in index order.  Entry nodes carry the union of their leaves' boxes (NaN
    skipped), leaves the empty box, as the host builder stores them."""
    boxes = np.asarray(boxes, F).reshape(-1, 6)

    def balanced(ids):
        return ids[0] if len(ids) == 1 else (balanced(ids[:len(ids) // 2]), balanced(ids[len(ids) // 2:]))

    shape = balanced(list(range(len(boxes)))) if shape is None else shape
    nodes = []

    def leaves(s):
        return [s] if isinstance(s, int) else leaves(s[0]) + leaves(s[1])

    def leaf(t):
        nodes.append(((np.inf,) * 3, LEAF + t, (-np.inf,) * 3, len(nodes) + 1))

    def emit(s):
        i = len(nodes)
        nodes.append(None)
        if isinstance(s, int):
            leaf(s)
        else:
            emit(s[0])
            emit(s[1])
        b = boxes[leaves(s)]
        with np.errstate(all="ignore"):
            mn = [_bound(b[:, c], False) for c in range(3)]
            mx = [_bound(b[:, 3 + c], True) for c in range(3)]
        nodes[i] = (tuple(mn), i + 1, tuple(mx), len(nodes))

    if isinstance(shape, int):
        leaf(shape)
    else:
        emit(shape[0])
        emit(shape[1])
    return np.array(nodes, NODE_DT)
