"""hks_skin_vertices (csrc/hk_scene.cpp over include/hk_skin.h) against tests/skin_numpy.py, an independent float32
restatement of the skin rule: every stored word equal, NaN for NaN, on seeded vertices and palettes and on the rule's
edges; the bounds rule on meshes with zeros of both signs; and five misreadings of the rule, each of which the same
inputs tell apart from the library.  No GPU: this pins the host side that tests/test_gpu_skin.py holds the device to."""
import ctypes as C

import numpy as np
import pytest

import skin_numpy as sn

SEED = 0x534B494E  # "SKIN"


def _lib():
    import hikari_amd
    return hikari_amd._abi.lib()


def host_skin(p, n, ix, w, joints, aabb=True):
    """hks_skin_vertices: (rc, positions, normals or None, aabb or None)."""
    p = np.ascontiguousarray(p, np.float32)
    n = None if n is None else np.ascontiguousarray(n, np.float32)
    ix, w = np.ascontiguousarray(ix, np.uint16), np.ascontiguousarray(w, np.float32)
    j = np.ascontiguousarray(joints, np.float32).reshape(-1, 16)
    op, on = np.full_like(p, 7.0), None if n is None else np.full_like(n, 7.0)
    box = np.full(6, 7.0, np.float32)
    rc = _lib().hks_skin_vertices(p.ctypes.data, None if n is None else n.ctypes.data, ix.ctypes.data, w.ctypes.data,
                                  len(p), j.ctypes.data, len(j), op.ctypes.data, None if on is None else on.ctypes.data,
                                  box.ctypes.data if aabb else None)
    return rc, op, on, box


def same_words(a, b):
    """Bit for bit, but any NaN equals any NaN (the sign and payload of a produced NaN are the FPU's)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


# ------------------------------------------------------------------ inputs
def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = axis
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _mat(linear, t):
    m = np.eye(4)
    m[:3, :3] = linear
    m[:3, 3] = t
    return m.T.reshape(16).astype(np.float32)  # column-major


def random_palette(rng, joints):
    out = []
    for _ in range(joints):
        lin = _rot(rng.normal(size=3), rng.uniform(-2.0, 2.0)) @ np.diag(rng.uniform(0.5, 1.8, 3))
        out.append(_mat(lin, rng.uniform(-1.0, 1.0, 3)))
    return np.stack(out)


def random_rig(rng, n, joints):
    ix = rng.integers(0, joints, (n, 4)).astype(np.uint16)
    w = rng.dirichlet(np.ones(4), n).astype(np.float32)
    return ix, w


def random_vertices(rng, n):
    p = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    nr = rng.normal(size=(n, 3))
    return p, (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(np.float32)


def edge_inputs():
    """{name: (positions, normals, indices, weights, joints)}: the rule's edges."""
    rng = np.random.default_rng([SEED, 1])
    n = 40
    p, nr = random_vertices(rng, n)
    pal = random_palette(rng, 6)
    ix, w = random_rig(rng, n, 6)
    one = np.zeros((n, 4), np.uint16)
    unit = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), (n, 1))
    off = (w * rng.uniform(0.3, 1.9, (n, 1))).astype(np.float32)  # sums other than 1: used as given
    # a zero weight on an out-of-pattern joint: joint 5 holds infinities and NaNs, and 0 * inf is a NaN the rule keeps
    wild = pal.copy()
    wild[5] = np.array([np.inf, -np.inf, np.nan, 1.0] * 4, np.float32)
    zix = ix.copy()
    zix[:, 3] = 5
    zw = w.copy()
    zw[:, 3] = 0.0
    special = {
        "rotation": _mat(_rot([1, 2, 3], 1.1), [0.1, -0.2, 0.3]),
        "non_uniform_scale": _mat(np.diag([3.0, 0.25, 1.5]), [0.0, 1.0, 0.0]),
        "mirror": _mat(np.diag([-1.0, 1.0, 1.0]) @ _rot([0, 1, 0], 0.4), [0.5, 0.0, 0.0]),
        "singular": _mat(np.diag([1.0, 0.0, 2.0]), [0.0, 0.0, 0.0]),
    }
    cases = {
        "single_joint": (p, nr, one, w, pal[:1]),
        "unit_weight": (p, nr, ix, unit, pal),
        "weights_off_one": (p, nr, ix, off, pal),
        "zero_weight_wild_joint": (p, nr, zix, zw, wild),
    }
    for name, m in special.items():
        cases[name] = (p, nr, one, unit, m[None, :])
        cases[name + "_blend"] = (p, nr, ix, w, np.concatenate([pal[:5], m[None, :]]))
    q = p.copy()
    q[:8, 0] = [1e-42, -3e-45, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-39]
    q[8:12, 1] = [0.0, -0.0, 5e-41, -np.inf]
    cases["special_positions"] = (q, nr, ix, w, pal)
    cases["special_positions_rigid"] = (q, nr, one, unit, special["rotation"][None, :])
    return cases


def random_inputs():
    rng = np.random.default_rng([SEED, 2])
    out = {}
    for n, joints in ((1, 1), (3, 2), (257, 7), (1000, 256)):
        p, nr = random_vertices(rng, n)
        out[f"random_{n}_{joints}"] = (p, nr) + random_rig(rng, n, joints) + (random_palette(rng, joints),)
    return out


INPUTS = {**edge_inputs(), **random_inputs()}


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(INPUTS))
def test_every_stored_word_equals_the_restatement(name):
    p, nr, ix, w, pal = INPUTS[name]
    rc, op, on, box = host_skin(p, nr, ix, w, pal)
    assert rc == 0
    want_p, want_n = sn.skin(p, nr, ix, w, pal)
    assert same_words(op, want_p), name
    assert same_words(on, want_n), name
    assert same_words(box, sn.bounds(want_p)), name


def test_the_edges_are_live():
    """The edge inputs do what their names say: the wild joint makes NaNs, the singular joint non-finite normals, the
    special positions reach the outputs, the weights off one scale the result."""
    I = INPUTS
    _, op, on, _ = host_skin(*I["zero_weight_wild_joint"])
    assert np.isnan(op).any()
    _, op, on, _ = host_skin(*I["singular"])
    assert np.isfinite(op).all() and not np.isfinite(on).all()
    _, op, _, box = host_skin(*I["special_positions_rigid"])
    assert np.isnan(op).any() and np.isinf(op).any() and np.isinf(box).any()
    a, b = host_skin(*I["weights_off_one"])[1], host_skin(*I["unit_weight"])[1]
    assert not same_words(a, b)
    # mirror: the inverse transpose flips the normal's handedness with the geometry (det < 0)
    p, nr, ix, w, pal = I["mirror"]
    M = pal[0].reshape(4, 4).T[:3, :3].astype(np.float64)
    assert np.linalg.det(M) < 0
    _, _, on, _ = host_skin(p, nr, ix, w, pal)
    assert np.allclose(on, nr.astype(np.float64) @ np.linalg.inv(M), rtol=1e-4, atol=1e-5)


def test_normals_are_optional_and_positions_do_not_depend_on_them():
    p, nr, ix, w, pal = INPUTS["random_257_7"]
    rc, op, on, box = host_skin(p, None, ix, w, pal)
    assert rc == 0 and on is None
    assert same_words(op, host_skin(p, nr, ix, w, pal)[1])
    rc, op2, _, untouched = host_skin(p, nr, ix, w, pal, aabb=False)
    assert rc == 0 and same_words(op, op2) and (untouched == 7.0).all()


@pytest.mark.parametrize("wrong", ["mat3", "pairing", "normalised", "det_order", "right_left"])
def test_misreadings_of_the_rule_are_told_apart(wrong):
    """Each misreading, applied to the restatement, differs from the library on seeded inputs (and the restatement
    itself does not)."""
    p, nr, ix, w, pal = INPUTS["random_1000_256"]
    _, op, on, _ = host_skin(p, nr, ix, w, pal)
    good_p, good_n = sn.skin(p, nr, ix, w, pal)
    assert same_words(op, good_p) and same_words(on, good_n)
    bad_p, bad_n = sn.skin(p, nr, ix, w, pal, wrong=wrong)
    assert not (same_words(op, bad_p) and same_words(on, bad_n)), wrong


FLIP = np.array([1.0, 0.0, -0.0, 0.0,  0.0, 1.0, -0.0, 0.0,  0.0, 0.0, -1.0, 0.0,  0.0, 0.0, -0.0, 1.0], np.float32)


def zeros_pose(rng, n, last):
    """A mesh in the plane z = +0 and a one-joint pose whose z row is (-0, -0, -1, -0): z' = ((-0 x + -0 y) + -1 * 0) + -0
    is -0 where x and y are positive (every term is -0) and +0 elsewhere (a +0 term wins the sum).  Seeded quadrants;
    the last vertex is in the quadrant that makes its zero's sign `last`."""
    p = np.zeros((n, 3), np.float32)
    p[:, :2] = rng.uniform(0.1, 1.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    p[0, :2], p[1, :2] = (0.5, 0.5), (-0.5, 0.5)  # both signs occur
    p[-1, :2] = (0.7, 0.3) if last else (-0.7, 0.3)
    ix, unit = np.zeros((n, 4), np.uint16), np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), (n, 1))
    return p, ix, unit, FLIP.reshape(1, 16)


def fold(p):
    """The rule's own words, literally: std::fmin / std::fmax folded from empty in vertex order, where of two equal
    operands the second is kept and a NaN operand loses."""
    mn, mx = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    for v in np.asarray(p, np.float32):
        for k in range(3):
            if not (mn[k] < v[k] or v[k] != v[k]):
                mn[k] = v[k]
            if not (mx[k] > v[k] or v[k] != v[k]):
                mx[k] = v[k]
    return np.concatenate([(mn + mx) * np.float32(0.5), (mx - mn) * np.float32(0.5)])


@pytest.mark.parametrize("last", [0, 1])
@pytest.mark.parametrize("n", [3, 64, 257])
def test_bounds_carry_the_sign_of_the_last_zero(n, last):
    """The posed z holds zeros of both signs, so both z bounds are zeros whose sign is the last vertex's: the host's
    fold, the restatement's order-free statement and the literal fold agree, and the centre's and half extent's z have
    the bits that sign gives ((-0 + -0) / 2 = -0, (-0 - -0) / 2 = +0)."""
    rng = np.random.default_rng([SEED, 3, n, last])
    p, ix, unit, pal = zeros_pose(rng, n, last)
    rc, op, _, box = host_skin(p, None, ix, unit, pal)
    assert rc == 0
    assert same_words(op, sn.skin(p, None, ix, unit, pal)[0])
    signs = np.signbit(op[:, 2])
    assert (op[:, 2] == 0.0).all() and signs.any() and not signs.all() and signs[-1] == bool(last)
    assert same_words(box, sn.bounds(op))
    assert same_words(box, fold(op))
    assert box.view(np.uint32)[[2, 5]].tolist() == [0x80000000 if last else 0, 0]


def test_refusals_write_nothing():
    L = _lib()
    p, nr, ix, w, pal = INPUTS["random_3_2"]
    rc, op, on, box = host_skin(p, nr, np.full_like(ix, 2), w, pal)  # an index == joint_count
    assert rc == -1 and (op == 7.0).all() and (on == 7.0).all() and (box == 7.0).all()
    out = np.zeros_like(p)
    args = [p.ctypes.data, None, ix.ctypes.data, w.ctypes.data, len(p), pal.ctypes.data, len(pal), out.ctypes.data, None,
            None]
    assert L.hks_skin_vertices(*args) == 0
    for null in (0, 2, 3, 5, 7):
        bad = list(args)
        bad[null] = None
        assert L.hks_skin_vertices(*bad) == -1, null
    bad = list(args)
    bad[6] = 0
    assert L.hks_skin_vertices(*bad) == -1
    bad = list(args)
    bad[1] = nr.ctypes.data  # normals without out_normals
    assert L.hks_skin_vertices(*bad) == -1
    assert C.sizeof(C.c_uint16) == 2
