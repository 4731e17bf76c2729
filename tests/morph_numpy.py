"""The morph rule (include/hk_morph.h) restated in vectorised float32 numpy, written from the rule's text without the
header's code: per component acc = base, then for the targets t in ascending order whose weight is not zero (of either
sign), acc = acc + w[t] * d[t], where the product and the sum are each one float32 operation on float32 arrays (numpy
rounds each to nearest even and never fuses).  The deltas are target-major, (targets, vertices, 3).  Normals take the same
fold over the normal deltas and are not normalised; without normal deltas they are the base normals.
tests/test_morph_independent.py holds hks_morph_vertices to it word for word.

`wrong` names one deliberate misreading of the rule; each must change some stored word on the test's inputs:
  "no_skip"       zero weights take part (base -0.0 becomes +0.0, 0 x inf becomes NaN)
  "sum_first"     the weighted deltas summed first (in ascending order), the sum added to the base last
  "descending"    the targets in descending order
  "normalised"    the normals normalised
  "f64"           each multiply-add evaluated in float64 and rounded to float32 once
  "vertex_major"  the deltas read as (vertices, targets, 3)
"""
import numpy as np

F = np.float32


def _fold(base, deltas, weights, wrong):
    base = np.asarray(base, F)
    w = np.asarray(weights, F).reshape(-1)
    d = np.asarray(deltas, F)
    T, V = len(w), len(base)
    d = d.reshape(V, T, 3).transpose(1, 0, 2) if wrong == "vertex_major" else d.reshape(T, V, 3)
    order = [t for t in range(T) if wrong == "no_skip" or w[t] != 0]  # (a NaN is not zero)
    if wrong == "descending":
        order = order[::-1]
    acc = base.copy()
    if wrong == "sum_first":
        if not order:
            return acc
        s = w[order[0]] * d[order[0]]
        for t in order[1:]:
            s = s + w[t] * d[t]
        return acc + s
    for t in order:
        if wrong == "f64":
            acc = (acc.astype(np.float64) + np.float64(w[t]) * d[t].astype(np.float64)).astype(F)
        else:
            acc = acc + w[t] * d[t]
    return acc


def morph(positions, normals, position_deltas, normal_deltas, weights, wrong=None):
    """(morphed positions, morphed normals or None), float32, by the rule."""
    with np.errstate(all="ignore"):
        out_p = _fold(positions, position_deltas, weights, wrong)
        if normals is None:
            return out_p, None
        n = np.asarray(normals, F)
        out_n = n.copy() if normal_deltas is None else _fold(n, normal_deltas, weights, wrong)
        if wrong == "normalised":
            out_n = out_n / np.sqrt((out_n[:, 0] * out_n[:, 0] + out_n[:, 1] * out_n[:, 1]) + out_n[:, 2] * out_n[:, 2])[:, None]
        return out_p, out_n
