"""The instance-rebuild cases (tests/dynamic_cases.py) on the CPU: the host builder alone confirms that every case
sits where its name says — its counts, the `halves` shape of the coincident trees, more big segments on one tree level
than the device's list holds, the alias tables' special entries, zeros of both signs among the corner sums, the
stack bounds of the deep trees, the singular transform.  tests/test_gpu_dynamic_sizes.py runs the same cases through
hk_update_instances."""
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import dynamic_cases as dc
from parity import NODE_DT, host_scene_array

EMISSIVE_WORDS = dict(instance=8, alias_offset=10, alias_count=11)  # include/hk_types.h hk_emissive, 16 words


def _tlas(desc):
    return host_scene_array(desc, 5, NODE_DT)


def _emissives(desc):
    return np.frombuffer(host_scene_array(desc, 8, np.dtype((np.void, 64))).tobytes(), np.uint32).reshape(-1, 16)


def _alias(desc):
    return host_scene_array(desc, 3, np.dtype([("prob", "<f4"), ("index", "<u4")]))


def _expected_counts():
    """case -> (instances, alias entries per emitter in upload order)."""
    out = {name: (n, [2] if n > 1 else []) for name, n in dc.TLAS_SIZES.items()}
    out["big_overflow"] = (dc.BIG_OVERFLOW_N, [2])
    for name, (m, n) in dc.LIGHT_SIZES.items():
        out[name] = (n, [1 + j % 3 for j in range(m)])
    for name, counts in dc.ALIAS_SIZES.items():
        out[name] = (2 * len(counts) + 2, counts)
    out.update({"coincident_100": (100, [2]), "coincident_300": (300, [2]), "clustered": (400, [2]),
                "equal_spacing": (200, [])})
    for name in dc.TRANSFORMS:
        out[name] = (dc.TRANSFORM_N, [3, 5, 7, 9, 11])
    for name, (n, _, _, _) in dc.DEPTH.items():
        out[name] = (n, [])
    return out


EXPECTED = _expected_counts()


def test_every_case_is_listed():
    assert set(EXPECTED) | {"singular"} == set(dc.CASES)
    assert set(dc.ARRAY_CASES) == set(dc.CASES) - {"singular", "too_deep"}
    assert set(dc.FRAME_CASES) | set(dc.SECOND_UPDATE_CASES) <= set(dc.ARRAY_CASES)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_counts_are_exact(name):
    """Instances, emitters and the alias entries of each emitter, in both scenes of the pair; 3k - 2 nodes in the
    TLAS and the light BVH."""
    n, alias = EXPECTED[name]
    scene0, scene1 = dc.case(name)
    for desc in (scene0.desc, dc.built1(name)):
        assert desc.instances.count == n and desc.instance_nodes.count == 3 * n - 2
        em = _emissives(desc)
        assert len(em) == len(alias) and desc.emissive_nodes.count == (3 * len(alias) - 2 if alias else 0)
        assert em[:, EMISSIVE_WORDS["alias_count"]].tolist() == alias
        assert em[:, EMISSIVE_WORDS["alias_offset"]].tolist() == [sum(alias[:j]) for j in range(len(alias))]
        assert desc.alias_table.count == sum(alias)
        assert len(dc.subtrees(_tlas(desc))) == 2 * n - 1  # the flat tree parses as bvh 0.7.1 flattens it
    assert np.all(np.diff(_emissives(scene0.desc)[:, EMISSIVE_WORDS["instance"]].astype(np.int64)) > 0)
    assert scene0.instance_local_aabbs().tobytes() == scene1.instance_local_aabbs().tobytes()


def test_sizes_straddle_the_builder_limits():
    """The TLAS, light-BVH and alias sizes are each limit and one more (dynamic_cases' constants restate
    hk_dynamic.hip's)."""
    src = (Path(__file__).resolve().parent.parent / "bevy-hikari_amd" / "csrc" / "hk_dynamic.hip").read_text()
    for text in ("COOP_MIN = 128;", "BVH_LDS_SHAPES = 1280;", "BIG_MAX = 64;", "ALIAS_LDS = 3072;",
                 "base += 256u", "base += 64u"):
        assert text in src, text
    sizes = set(dc.TLAS_SIZES.values())
    for limit in (dc.COOP_MIN, dc.BALLOT_CHUNK, dc.BVH_LDS_SHAPES):
        assert {limit, limit + 1} <= sizes
    assert {1, 2} <= sizes and max(sizes) > 2 * dc.BVH_LDS_SHAPES
    lights = {m for m, _ in dc.LIGHT_SIZES.values()}
    assert {1, 2, dc.COOP_MIN + 1} <= lights and max(lights) > dc.BALLOT_CHUNK
    alias = {c[0] for c in dc.ALIAS_SIZES.values()}
    assert {1, dc.WAVE, dc.WAVE + 1, dc.ALIAS_LDS, dc.ALIAS_LDS + 1} <= alias
    a, b, c = dc.ALIAS_SIZES["two_large"]
    assert a > dc.ALIAS_LDS and b > dc.ALIAS_LDS and c < dc.WAVE  # the second one's scratch offset is a, not 0


@pytest.mark.parametrize("name", list(dc.COINCIDENT))
def test_coincident_trees_have_the_halves_shape(name):
    """All centroids coincide: every split is idx[:k / 2] | idx[k / 2:] in index order, down to the leaves; 100 shapes
    stay on the per-thread split, 300 enter the cooperative one."""
    n = dc.COINCIDENT[name]
    assert (n > dc.COOP_MIN) == (name == "coincident_300")
    nodes = _tlas(dc.built1(name))
    sub = {a: k for a, k, _ in dc.subtrees(nodes)}
    for a, k in sub.items():
        if k > 1:
            assert sub[a + 1] == k // 2
    leaves = nodes["entry"][nodes["entry"] >= 0x80000000] - 0x80000000
    assert leaves.tolist() == list(range(n))  # halves keep the index order


def test_clustered_tree_splits_by_sah_first_then_by_halves():
    """8 clusters of 50 identical transforms: SAH splits between the clusters, and every subtree of one cluster (50
    shapes with one centroid) has the halves shape below it."""
    nodes = _tlas(dc.built1("clustered"))
    st = dc.subtrees(nodes)
    sub = {a: k for a, k, _ in st}
    assert st[0][1] == 400 and sub[1] not in (200,) and sub[1] % 50 == 0  # the root: whole clusters, not halves
    heads = [a for a, k, _ in st if k == 50]
    assert len(heads) == 8
    for h in heads:
        leaves = nodes["entry"][h: h + 3 * 50 - 2]
        ids = leaves[leaves >= 0x80000000] - 0x80000000
        assert ids.tolist() == list(range(int(ids[0]), int(ids[0]) + 50)) and ids[0] % 50 == 0
        for a, k in sub.items():
            if h <= a < h + 148 and k > 1:
                assert sub[a + 1] == k // 2
    assert any(k > dc.COOP_MIN for _, k, d in st if d > 0)  # cooperative splits above the clusters


def test_equal_spacing_ties_go_to_the_first_split():
    """200 identical boxes 1 / 64 apart on x: a subtree of three of them has the mirror-image splits 1 | 2 and 2 | 1
    at exactly equal cost (the same extents, the same counts swapped), and `cost < best` keeps the first."""
    _, scene1 = dc.case("equal_spacing")
    x = scene1.instance_models()[:, 12]
    assert np.array_equal(np.diff(x), np.full(199, np.float32(1 / 64)))
    nodes = _tlas(dc.built1("equal_spacing"))
    sub = {a: k for a, k, _ in dc.subtrees(nodes)}
    threes = [a for a, k in sub.items() if k == 3]
    assert len(threes) >= 8
    assert all(sub[a + 1] == 1 for a in threes)


def test_big_overflow_has_more_big_segments_on_a_level_than_the_list_holds():
    """At some depth the host TLAS has more than BIG_MAX subtrees of more than COOP_MIN shapes: the segments of one
    level of the device build, so its big list overflows there."""
    st = dc.subtrees(_tlas(dc.built1("big_overflow")))
    per_level = Counter(d for _, k, d in st if k > dc.COOP_MIN)
    assert max(per_level.values()) > dc.BIG_MAX, per_level
    # and no other case does: they stay within the list
    for name in ("tlas_2600", "lights_300"):
        st = dc.subtrees(_tlas(dc.built1(name)))
        assert max(Counter(d for _, k, d in st if k > dc.COOP_MIN).values()) <= dc.BIG_MAX


def test_alias_cases_have_their_entries():
    t = _alias(dc.built1("regular"))
    assert any(p == 0.0 and i == k for k, (p, i) in enumerate(t))  # probability exactly 1: in neither list
    t = _alias(dc.built1("one_degenerate"))
    assert t[9]["prob"] == 1.0 and t[9]["index"] != 9              # area 0: 1 - 0, aliased to an over entry
    assert np.isfinite(t["prob"]).all()
    t = _alias(dc.built1("skewed"))
    assert (t["index"] == 77).sum() > 150                          # the large triangle takes most entries
    for name, counts in dc.ALIAS_SIZES.items():
        t = _alias(dc.built1(name))
        assert np.isfinite(t["prob"]).all() and (t["index"] < max(counts)).all()
        if max(counts) > 1 and name != "regular":
            assert (t["prob"] > 0).any(), name                     # over and under lists both in use


def _corner_candidates(models, aabbs):
    """(n, 8, 3) float32: the corner offsets hks_build folds into an instance box, with its float operations."""
    f = np.float32
    out = np.empty((len(models), 8, 3), f)
    for k in range(8):
        sign = [f(2 * (k & 1) - 1), f(2 * ((k >> 1) & 1) - 1), f(2 * ((k >> 2) & 1) - 1)]
        v = [aabbs[:, 3 + c] * sign[c] for c in range(3)]
        for r in range(3):
            out[:, k, r] = (models[:, r] * v[0] + models[:, 4 + r] * v[1]) + models[:, 8 + r] * v[2]
    return out


def _fold(cand, second_wins):
    """min and max of 0 and the eight candidates of each instance, folded in order.  second_wins: of two equal
    operands (zeros of either sign) the fold keeps the second, as the host's fmin / fmax; otherwise -0 < +0."""
    mn = np.zeros(cand[:, 0].shape, np.float32)
    mx = mn.copy()
    for k in range(8):
        c = cand[:, k]
        if second_wins:
            mn, mx = np.where(mn < c, mn, c), np.where(mx > c, mx, c)
        else:
            mn = np.where((c < mn) | ((c == mn) & np.signbit(c)), c, mn)
            mx = np.where((c > mx) | ((c == mx) & ~np.signbit(c)), c, mx)
    return mn, mx


def test_neg_zero_has_zeros_of_both_signs_among_its_corner_sums():
    """Some instance's corner candidates hold +0 and -0 on one axis, so the box depends on which of two equal
    operands min and max return.  The host builder's boxes are those of the ordered fold (the second of two equal
    operands), and a symmetric min / max (-0 below +0) would give other bits for some of them."""
    _, scene1 = dc.case("neg_zero")
    models, aabbs = scene1.instance_models(), scene1.instance_local_aabbs()
    assert np.signbit(models[models == 0]).any() and (~np.signbit(models[models == 0])).any()
    cand = _corner_candidates(models, aabbs)
    zero = cand == 0
    both = (zero & np.signbit(cand)).any(axis=1) & (zero & ~np.signbit(cand)).any(axis=1)
    assert both.any(axis=1).sum() > 100
    inst = np.frombuffer(host_scene_array(dc.built1("neg_zero"), 4, np.dtype((np.void, 176))).tobytes(),
                         np.float32).reshape(-1, 44)
    centre = np.stack([((models[:, r] * aabbs[:, 0] + models[:, 4 + r] * aabbs[:, 1]) + models[:, 8 + r] * aabbs[:, 2])
                       + models[:, 12 + r] for r in range(3)], axis=1)
    mn, mx = _fold(cand, True)
    assert (mn + centre).tobytes() == inst[:, 0:3].tobytes() and (mx + centre).tobytes() == inst[:, 4:7].tobytes()
    smn, smx = _fold(cand, False)
    assert (smn + centre).tobytes() != inst[:, 0:3].tobytes() or (smx + centre).tobytes() != inst[:, 4:7].tobytes()
    # and the TLAS joins zeros of both signs too
    nodes = _tlas(dc.built1("neg_zero"))
    boxes = np.concatenate([nodes["min"], nodes["max"]])
    assert (boxes == 0).any() and np.signbit(boxes[boxes == 0]).any() and (~np.signbit(boxes[boxes == 0])).any()


@pytest.mark.parametrize("name", list(dc.DEPTH))
def test_depth_cases_have_their_stack_bounds(name):
    """The most inner nodes on a root-to-leaf path of scene1's host TLAS plus the BLAS part, read off the flat
    trees, and the library's own bound (hk_scene_gbuffer_stack); scene0 fits the LDS stack in every case."""
    from hikari_amd import scene_gbuffer_stack
    scene0, scene1 = dc.case(name)
    dc.built1(name)
    need = dc.stack_need(scene1)
    assert scene_gbuffer_stack(scene1) == (need, dc.GB_STACK_LDS)
    assert need == dc.DEPTH_NEED[name]
    assert dc.DEPTH_NEED == {"deep_lds_edge": dc.GB_STACK_LDS, "deep_over_lds": dc.GB_STACK_LDS + 1,
                             "deep_at_limit": dc.GB_STACK, "too_deep": dc.GB_STACK + 1}
    assert dc.stack_need(scene0) <= dc.GB_STACK_LDS and scene_gbuffer_stack(scene0)[0] == dc.stack_need(scene0)


def test_transform_cases_are_what_they_say():
    lin = {name: dc.case(name)[1].instance_models().reshape(-1, 4, 4)[:, :3, :3].transpose(0, 2, 1).astype(np.float64)
           for name in dc.TRANSFORMS}
    assert (np.linalg.det(lin["mirrored"]) < 0).all()
    sv = np.linalg.svd(lin["non_uniform"], compute_uv=False)
    assert np.allclose(sv, [20.0, 1.0, 0.05], rtol=1e-5)
    gram = np.einsum("nij,nik->njk", lin["sheared"], lin["sheared"])
    assert (np.abs(gram[:, 0, 1]) + np.abs(gram[:, 0, 2]) + np.abs(gram[:, 1, 2]) > 1e-3).all()  # columns not orthogonal
    q = lin["quarter_turns"]
    assert np.isin(q, [0.0, 1.0, -1.0]).all() and (np.linalg.det(q) == 1.0).all()
    assert len({m.tobytes() for m in q}) == len(dc.QUARTER_TURNS)
    for name, s in (("scale_1e-4", 1e-4), ("scale_1e4", 1e4)):
        assert np.allclose(np.linalg.svd(lin[name], compute_uv=False), s, rtol=1e-5)
    nz = lin["neg_zero"]
    off = nz[:, ~np.eye(3, dtype=bool)]
    assert (off == 0).all() and (np.diagonal(nz, axis1=1, axis2=2) != 0).all()


def test_singular_case_is_refused_by_the_host_builder():
    from hikari_amd import HikariError
    scene0, scene1 = dc.case("singular")
    assert scene0.desc is not None
    with pytest.raises(HikariError, match="singular instance transform"):
        scene1.build()
