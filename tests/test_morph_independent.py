"""hks_morph_vertices (csrc/hk_scene.cpp over include/hk_morph.h) against tests/morph_numpy.py, an independent float32
restatement of the morph rule: every stored word equal, NaN for NaN, positions, normals and Aabb alike, on seeded bases,
deltas and weights and on the rule's edges; a morph under a skin against tests/skin_numpy.py applied afterwards; six
misreadings of the rule, each of which some input tells apart from the library; and the refusals.  No GPU: this pins the
host side that tests/test_gpu_morph.py holds the device to."""
import numpy as np
import pytest

import morph_numpy as mn
import skin_numpy as sn
from test_skin_independent import random_palette, random_rig, random_vertices, same_words

SEED = 0x4D4F5250  # "MORP"
VERTEX_COUNTS = (1, 3, 65)
TARGET_COUNTS = (1, 2, 7, 256)
DENORMAL = np.float32(1e-40)
WEIGHT_KINDS = np.array([0.0, -0.0, 1.0, -0.75, 1.5, DENORMAL], np.float32)


def _lib():
    import hikari_amd
    return hikari_amd._abi.lib()


def host_morph(p, n, dp, dn, w, aabb=True, targets=None):
    """hks_morph_vertices: (rc, positions, normals or None, aabb)."""
    p = np.ascontiguousarray(p, np.float32)
    n = None if n is None else np.ascontiguousarray(n, np.float32)
    dp = np.ascontiguousarray(dp, np.float32)
    dn = None if dn is None else np.ascontiguousarray(dn, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    op, on = np.full_like(p, 7.0), None if n is None else np.full_like(n, 7.0)
    box = np.full(6, 7.0, np.float32)
    rc = _lib().hks_morph_vertices(p.ctypes.data, None if n is None else n.ctypes.data, dp.ctypes.data,
                                   None if dn is None else dn.ctypes.data, len(p), w.ctypes.data,
                                   len(w) if targets is None else targets, op.ctypes.data,
                                   None if on is None else on.ctypes.data, box.ctypes.data if aabb else None)
    return rc, op, on, box


# ------------------------------------------------------------------ inputs
def random_deltas(rng, targets, n):
    return (rng.normal(size=(targets, n, 3)) * 0.3).astype(np.float32), (rng.normal(size=(targets, n, 3)) * 0.2).astype(np.float32)


def random_weights(rng, targets):
    """Half of the weights from WEIGHT_KINDS (zeros of both signs, 1, negative, above 1, denormal), half seeded."""
    w = rng.uniform(-1.0, 2.0, targets).astype(np.float32)
    kind = rng.random(targets) < 0.5
    w[kind] = rng.choice(WEIGHT_KINDS, int(kind.sum()))
    return w


def random_inputs():
    out = {}
    for n in VERTEX_COUNTS:
        for targets in TARGET_COUNTS:
            rng = np.random.default_rng([SEED, n, targets])
            p, nr = random_vertices(rng, n)
            dp, dn = random_deltas(rng, targets, n)
            w = random_weights(rng, targets)
            if targets >= 2:
                w[[0, -1]] = (0.625, -1.25)  # two targets take part whatever the draw
            out[f"random_{n}_{targets}"] = (p, nr, dp, dn, w)
    return out


def edge_inputs():
    rng = np.random.default_rng([SEED, 1])
    n, targets = 65, 7
    p, nr = random_vertices(rng, n)
    dp, dn = random_deltas(rng, targets, n)
    w = random_weights(rng, targets)
    w[[1, 4]] = (0.5, 1.75)
    signed = p.copy()
    signed[::3, 0], signed[1::3, 1], signed[2::3, 2] = -0.0, 0.0, -0.0  # zeros of both signs in the base
    zeros = np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0, 0.0], np.float32)
    wild = dp.copy()
    wild[2] = np.inf
    wild[5, ::2] = -np.inf
    wild[3, 1::2] = np.nan
    skip = w.copy()
    skip[[2, 3, 5]] = (0.0, -0.0, 0.0)  # the wild targets do not take part
    nan_w = w.copy()
    nan_w[3] = np.nan
    every = np.array([0.0, -0.0, 1.0, -0.75, 1.5, DENORMAL, 0.3], np.float32)
    return {
        "all_weights_zero": (signed, nr, dp, dn, zeros),
        "zero_weight_on_infinite_delta": (signed, nr, wild, (wild * np.float32(0.5)).astype(np.float32), skip),
        "nan_weight": (p, nr, dp, dn, nan_w),
        "every_weight_kind": (signed, nr, dp, dn, every),
        "infinite_delta_takes_part": (p, nr, wild, dn, w),
        "no_normal_deltas": (p, nr, dp, None, w),
        "no_normals": (p, None, dp, None, w),
    }


INPUTS = {**random_inputs(), **edge_inputs()}


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(INPUTS))
def test_every_stored_word_equals_the_restatement(name):
    p, nr, dp, dn, w = INPUTS[name]
    rc, op, on, box = host_morph(p, nr, dp, dn, w)
    assert rc == 0
    want_p, want_n = mn.morph(p, nr, dp, dn, w)
    assert same_words(op, want_p), name
    assert (on is None and want_n is None) or same_words(on, want_n), name
    assert same_words(box, sn.bounds(want_p)), name


def test_the_edges_are_live():
    """The edge inputs do what their names say."""
    I = INPUTS
    p, nr, dp, dn, w = I["all_weights_zero"]
    _, op, on, _ = host_morph(p, nr, dp, dn, w)
    assert op.tobytes() == p.tobytes() and on.tobytes() == nr.tobytes()  # byte for byte, -0.0 included
    assert (p.view(np.uint32) == 0x80000000).any() and (p.view(np.uint32) == 0).any()
    p, nr, dp, dn, w = I["zero_weight_on_infinite_delta"]
    _, op, on, _ = host_morph(p, nr, dp, dn, w)
    assert np.isinf(dp).any() and np.isnan(dp).any() and np.isfinite(op).all() and np.isfinite(on).all()
    _, op, on, _ = host_morph(*I["nan_weight"])
    assert np.isnan(op).all() and np.isnan(on).all()  # a NaN weight is not zero: it takes part in every vertex
    _, op, _, box = host_morph(*I["infinite_delta_takes_part"])
    assert not np.isfinite(op).all() and not np.isfinite(box).all()
    p, nr, dp, dn, w = I["no_normal_deltas"]
    _, op, on, _ = host_morph(p, nr, dp, dn, w)
    assert on.tobytes() == nr.tobytes() and op.tobytes() != p.tobytes()
    p, nr, dp, dn, w = I["every_weight_kind"]
    assert set(w.view(np.uint32).tolist()) >= set(WEIGHT_KINDS.view(np.uint32).tolist())
    # the denormal weight reaches the sum: without it some word differs
    only = np.zeros_like(w)
    only[5] = DENORMAL
    big = (dp * np.float32(1e38)).astype(np.float32)
    rc, op, _, _ = host_morph(p, nr, big, dn, only)
    assert rc == 0 and same_words(op, mn.morph(p, nr, big, dn, only)[0]) and not same_words(op, p)


def test_normals_are_optional_and_positions_do_not_depend_on_them():
    p, nr, dp, dn, w = INPUTS["random_65_7"]
    rc, op, on, box = host_morph(p, None, dp, None, w)
    assert rc == 0 and on is None
    assert same_words(op, host_morph(p, nr, dp, dn, w)[1])
    rc, op2, _, untouched = host_morph(p, nr, dp, dn, w, aabb=False)
    assert rc == 0 and same_words(op, op2) and (untouched == 7.0).all()


@pytest.mark.parametrize("joints", [1, 6])
def test_morph_under_a_skin_is_the_skin_rule_applied_afterwards(joints):
    """hikari_amd.morph_vertices with joints (hks_morph_vertices, then hks_skin_vertices) against the two restatements
    one after the other: glTF's order, morph then skin."""
    from hikari_amd import Mesh, Morph, Skin, morph_vertices
    rng = np.random.default_rng([SEED, 2, joints])
    n, targets = 65, 7
    p, nr = random_vertices(rng, n)
    dp, dn = random_deltas(rng, targets, n)
    w = random_weights(rng, targets)
    w[[0, 3]] = (0.8, -0.4)
    ix, sw = random_rig(rng, n, joints)
    pal = random_palette(rng, joints)
    mesh = Mesh(p, nr, np.zeros((n, 2), np.float32), None, 0, Skin(ix, sw, joints), Morph(dp, dn))
    got, box = morph_vertices(mesh, w, pal, aabb=True)
    mp, mnr = mn.morph(p, nr, dp, dn, w)
    want_p, want_n = sn.skin(mp, mnr, ix, sw, pal)
    assert same_words(got.positions, want_p) and same_words(got.normals, want_n)
    assert same_words(box, sn.bounds(want_p))
    assert not same_words(got.positions, sn.skin(p, nr, ix, sw, pal)[0])  # the morph shows under the skin
    alone, box = morph_vertices(mesh, w, aabb=True)
    assert same_words(alone.positions, mp) and same_words(alone.normals, mnr) and same_words(box, sn.bounds(mp))
    assert got.morph is mesh.morph and got.skin is mesh.skin


WRONG = ["no_skip", "sum_first", "descending", "normalised", "f64", "vertex_major"]


@pytest.mark.parametrize("wrong", WRONG)
def test_misreadings_of_the_rule_are_told_apart(wrong):
    """Each misreading, applied to the restatement, differs from the library on at least one of the inputs (and the
    restatement itself differs on none: test_every_stored_word_equals_the_restatement)."""
    told = []
    for name, (p, nr, dp, dn, w) in INPUTS.items():
        _, op, on, _ = host_morph(p, nr, dp, dn, w)
        bad_p, bad_n = mn.morph(p, nr, dp, dn, w, wrong=wrong)
        if not (same_words(op, bad_p) and (on is None or same_words(on, bad_n))):
            told.append(name)
    assert told, wrong


def test_zero_skipping_is_told_apart_by_the_signed_base_alone():
    """The first misreading on the input made for it: -0.0 + 0 * d is +0.0, and 0 * inf is NaN."""
    for name in ("all_weights_zero", "zero_weight_on_infinite_delta"):
        p, nr, dp, dn, w = INPUTS[name]
        _, op, _, _ = host_morph(p, nr, dp, dn, w)
        assert not same_words(op, mn.morph(p, nr, dp, dn, w, wrong="no_skip")[0]), name


def test_refusals_write_nothing():
    L = _lib()
    p, nr, dp, dn, w = INPUTS["random_3_2"]
    for targets in (0, 257):
        rc, op, on, box = host_morph(p, nr, dp, dn, w, targets=targets)
        assert rc == -1 and (op == 7.0).all() and (on == 7.0).all() and (box == 7.0).all(), targets
    out, out_n = np.zeros_like(p), np.zeros_like(nr)
    args = [p.ctypes.data, nr.ctypes.data, dp.ctypes.data, dn.ctypes.data, len(p), w.ctypes.data, len(w),
            out.ctypes.data, out_n.ctypes.data, None]
    assert L.hks_morph_vertices(*args) == 0
    good = out.copy()
    out[:], out_n[:] = 7.0, 7.0
    for null in (0, 2, 5, 7):  # positions, position_deltas, weights, out_positions
        bad = list(args)
        bad[null] = None
        assert L.hks_morph_vertices(*bad) == -1, null
    for null in (1, 8):  # normals without out_normals and the reverse
        bad = list(args)
        bad[null] = None
        assert L.hks_morph_vertices(*bad) == -1, null
    bad = list(args)
    bad[1] = bad[8] = None  # normal_deltas without normals
    assert L.hks_morph_vertices(*bad) == -1
    assert (out == 7.0).all() and (out_n == 7.0).all()
    ok = list(args)
    ok[3] = None  # normal_deltas may be NULL with normals
    assert L.hks_morph_vertices(*ok) == 0 and same_words(out, good) and same_words(out_n, nr)
    w256 = np.zeros(256, np.float32)
    d256 = np.zeros((256, len(p), 3), np.float32)
    assert host_morph(p, nr, d256, d256, w256)[0] == 0  # HK_MORPH_MAX_TARGETS itself is taken
