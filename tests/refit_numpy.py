"""The BLAS refit rule restated in numpy, from its text (the comment of hikari_scene.h hks_refit_nodes) and
without include/hk_refit.h: what tests/test_refit_independent.py holds hks_refit_nodes against.

A slice is a bvh-0.7.1 flatten (parity.NODE_DT records, indices relative to the slice).  A leaf has
entry >= 0x80000000, its payload the mesh-local primitive; an entry node i carries the box of the subtree stored in
(i, exit).  The refit leaves every leaf and every index as it is and gives entry node i

    min[c] = the least S[t].min[c] over the leaves t in (i, exit), -0 below +0
    max[c] = the greatest S[t].max[c] likewise, +0 above -0

where S[t] is primitive t's shape box as the build folds it: from +inf / -inf over the corners 0, 1, 2 in order with
std::fmin / std::fmax, which skip a NaN and, of two equal operands (the two zeros are equal), keep the second.

The restatement does not use the recurrence of the host function (a node's box from its two children's): each entry
node GATHERS the primitives of the leaves in its range and reduces over them.  The keyword arguments switch on one
misreading of the rule each; the tests show that each gives other words somewhere."""
from __future__ import annotations

import numpy as np

LEAF = 0x80000000
NODE_DT = np.dtype([("min", "<f4", 3), ("entry", "<u4"), ("max", "<f4", 3), ("exit", "<u4")])


def corners_of(primitives) -> np.ndarray:
    """(k, 3, 3) float32 corner positions of k hk_primitive records (48 bytes: three corners of position xyz, index)."""
    words = np.frombuffer(np.ascontiguousarray(primitives).tobytes(), np.float32).reshape(-1, 3, 4)
    return np.ascontiguousarray(words[:, :, :3])


def _std_fmin(a, b, nan_propagates=False):
    if nan_propagates:
        return np.minimum(a, b)
    return np.where((a < b) | (b != b), a, b)


def _std_fmax(a, b, nan_propagates=False):
    if nan_propagates:
        return np.maximum(a, b)
    return np.where((a > b) | (b != b), a, b)


def shape_boxes(corners, nan_propagates=False):
    """(S.min, S.max), each (k, 3): the fold over the corners in order, from empty."""
    k = len(corners)
    mn = np.full((k, 3), np.inf, np.float32)
    mx = np.full((k, 3), -np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            mn = _std_fmin(mn, corners[:, c, :], nan_propagates)
            mx = _std_fmax(mx, corners[:, c, :], nan_propagates)
    return mn.astype(np.float32), mx.astype(np.float32)


def _least(values, positional=False, greatest=False):
    """One bound from a subtree's gathered values (m,), none of them NaN unless a misreading made one."""
    values = np.asarray(values, np.float32)
    if np.isnan(values).any():
        return np.float32(np.nan)
    v = values.max() if greatest else values.min()
    if v != 0.0:
        return np.float32(v)
    zeros = values[values == 0.0]
    if positional:  # the misreading: the sign of the last zero in leaf order, as a std::fmin fold would leave it
        return np.float32(zeros[-1])
    negative = np.signbit(zeros)
    if greatest:
        return np.float32(-0.0) if negative.all() else np.float32(0.0)
    return np.float32(-0.0) if negative.any() else np.float32(0.0)


def refit(nodes, corners, *, closed_range=False, positional=False, nan_propagates=False, host_leaf_boxes=False):
    """A copy of `nodes` (NODE_DT) refit over `corners` (k, 3, 3).  Misreadings: closed_range: the range is [i, exit),
    so node i's own stored box joins in; positional: a zero bound takes the sign of the last zero in leaf order;
    nan_propagates: a NaN corner makes its bounds NaN; host_leaf_boxes: the leaves get their shape box."""
    nodes = np.array(nodes, NODE_DT)
    smin, smax = shape_boxes(np.asarray(corners, np.float32), nan_propagates)
    out = nodes.copy()
    leaf = nodes["entry"] >= LEAF
    for i in range(len(nodes)):
        if leaf[i]:
            if host_leaf_boxes:
                t = int(nodes["entry"][i] - LEAF)
                out["min"][i], out["max"][i] = smin[t], smax[t]
            continue
        e = int(nodes["exit"][i])
        inside = np.arange(i + 1, e)
        prims = (nodes["entry"][inside][leaf[inside]] - LEAF).astype(np.int64)  # the gather, in leaf order
        lo, hi = smin[prims], smax[prims]
        if closed_range:
            lo, hi = np.vstack([nodes["min"][i][None], lo]), np.vstack([nodes["max"][i][None], hi])
        for c in range(3):
            out["min"][i][c] = _least(lo[:, c], positional)
            out["max"][i][c] = _least(hi[:, c], positional, greatest=True)
    return out


def words(nodes) -> np.ndarray:
    """The stored words of a node array, for comparisons that tell -0 from +0 and one NaN from another."""
    return np.frombuffer(np.ascontiguousarray(nodes).tobytes(), np.uint32).reshape(-1, 8)
