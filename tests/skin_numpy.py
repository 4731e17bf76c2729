"""The skin rule (include/hk_skin.h) restated in vectorised float32 numpy, written from the rule's text without the
header: every product and sum below is one float32 operation on float32 arrays (numpy rounds each to nearest even and
never fuses), in the pinned left-to-right order, with IEEE division.  tests/test_skin_independent.py holds
hks_skin_vertices to it word for word.

`wrong` names one deliberate misreading of the rule; each must change some stored word on the test's inputs:
  "mat3"        the normal through mat3(M) instead of its inverse transpose
  "pairing"     weight k paired with index k + 1 (cyclically)
  "normalised"  the normal normalised
  "det_order"   det as dot(c0, X) (equal in exact arithmetic, another rounding)
  "right_left"  the weighted sum associated right to left: w.x J0 + (w.y J1 + (w.z J2 + w.w J3))
"""
import numpy as np

F = np.float32


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def skin_matrix(indices, weights, joints, wrong=None):
    """(n, 4, 4) skin matrices, [v, column, row], from (n, 4) u16 indices, (n, 4) f32 weights, (j, 16) column-major."""
    J = np.asarray(joints, F).reshape(-1, 4, 4)  # [joint, column, row]
    ix = np.asarray(indices, np.int64)
    w = np.asarray(weights, F)
    if wrong == "pairing":
        ix = np.roll(ix, -1, axis=1)
    t = [w[:, k, None, None] * J[ix[:, k]] for k in range(4)]
    if wrong == "right_left":
        return t[0] + (t[1] + (t[2] + t[3]))
    return ((t[0] + t[1]) + t[2]) + t[3]


def skin(positions, normals, indices, weights, joints, wrong=None):
    """(posed positions, posed normals or None), float32, by the rule."""
    with np.errstate(all="ignore"):
        M = skin_matrix(indices, weights, joints, wrong)
        p = np.asarray(positions, F)
        c0, c1, c2, c3 = M[:, 0, :3], M[:, 1, :3], M[:, 2, :3], M[:, 3, :3]
        out_p = ((c0 * p[:, 0:1] + c1 * p[:, 1:2]) + c2 * p[:, 2:3]) + c3
        if normals is None:
            return out_p, None
        n = np.asarray(normals, F)
        if wrong == "mat3":
            return out_p, (c0 * n[:, 0:1] + c1 * n[:, 1:2]) + c2 * n[:, 2:3]
        X, Y, Z = _cross(c1, c2), _cross(c2, c0), _cross(c0, c1)
        det = _dot(c0, X) if wrong == "det_order" else _dot(c2, Z)
        det = det[:, None]
        out_n = ((X / det) * n[:, 0:1] + (Y / det) * n[:, 1:2]) + (Z / det) * n[:, 2:3]
        if wrong == "normalised":
            out_n = out_n / np.sqrt(_dot(out_n, out_n))[:, None]
        return out_p, out_n


def bounds(positions):
    """The Bevy Aabb (centre xyz, half extents xyz) of posed positions by the rule's order-free statement: each bound the
    fminf / fmaxf value (a NaN loses), a bound equal to zero with the sign of the last vertex whose component is a zero."""
    p = np.asarray(positions, F)
    with np.errstate(all="ignore"):
        mn = np.fmin.reduce(p, axis=0, initial=F(np.inf))
        mx = np.fmax.reduce(p, axis=0, initial=F(-np.inf))
        for k in range(3):
            zeros = p[p[:, k] == 0.0, k]
            if mn[k] == 0.0:
                mn[k] = zeros[-1]
            if mx[k] == 0.0:
                mx[k] = zeros[-1]
        return np.concatenate([(mn + mx) * F(0.5), (mx - mn) * F(0.5)]).astype(F)
