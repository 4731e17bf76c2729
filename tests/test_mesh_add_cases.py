"""The cases of tests/mesh_add_cases.py sit where their names say, by the host builder alone, and hk_add_meshes_counts,
the host arithmetic hk_add_meshes sizes its allocations and launches with, gives the host build's slices and counts for
every case and step and returns every refusal of the header.  Needs no GPU."""
import ctypes

import numpy as np
import pytest

import dynamic_cases as dc
import instance_set_cases as ic
import mesh_add_cases as ac
import mesh_cases as mc
from parity import NODE_DT, host_scene_array


def _tris(mesh) -> int:
    n = len(mesh.positions) if mesh.indices is None else len(mesh.indices)
    return n - 2 if mesh.topology == 1 else n // 3


def _counts(desc) -> list:
    return ic.desc_counts(desc)


# ------------------------------------------------------------------ the edges
@pytest.mark.parametrize("name", list(ac.SIZES))
def test_size_cases_add_one_mesh_of_the_named_triangle_count(name):
    c = ac.case(name)
    n = ac.SIZES[name]
    assert [_tris(m) for m in c.new[1]] == [n]
    v, p, n0, nc = ac.new_slices(name, 1)[0]
    assert nc == 3 * n - 2
    nodes = mc.mesh_nodes(ac.built(name, 1), (v, p, n0, nc))
    assert len(dc.subtrees(nodes)) == 2 * n - 1  # a full binary tree over n leaves, read off the flat nodes
    if n > 2:
        assert dc.inner_depth(nodes) > 1


def test_the_sizes_straddle_the_kernel_limits():
    n = set(ac.SIZES.values())
    assert {1, 2} <= n
    assert {ac.COOP_MIN, ac.COOP_MIN + 1, 256, 257, ac.BVH_LDS_SHAPES, ac.BVH_LDS_SHAPES + 1} <= n
    assert max(n) > 2 * ac.BVH_LDS_SHAPES


@pytest.mark.parametrize("name", list(ac.STRIPS))
def test_strip_cases(name):
    """The strip is second in its call behind a mesh of an odd triangle count, so its first triangle's global id is
    odd while its mesh-local one is even; 6 indices: local triangles 0..3 (an odd last one), 7: 0..4."""
    c = ac.case(name)
    first, strip = c.new[1]
    assert _tris(first) % 2 == 1 and first.topology == 0
    assert strip.topology == 1 and len(strip.indices) == ac.STRIPS[name]
    tris = _tris(strip)
    assert (tris - 1) % 2 == (1 if name == "strip_even" else 0)
    # the host winds triangle t as (t, t + 1, t + 2), the first two swapped for odd t
    v, p, n0, nc = ac.new_slices(name, 1)[1]
    prims = np.frombuffer(host_scene_array(ac.built(name, 1), 1, np.dtype((np.void, 48))).tobytes(),
                          np.uint32).reshape(-1, 3, 4)[p: p + tris, :, 3]
    ix = strip.indices
    want = [[ix[t + (t & 1)], ix[t + 1 - (t & 1)], ix[t + 2]] for t in range(tris)]
    assert prims.tolist() == want
    assert not np.array_equal(np.sort(ix), ix)  # the indices are no identity


def test_non_indexed_and_shared_vertices():
    m = ac.case("non_indexed").new[1][0]
    assert m.indices is None and len(m.positions) % 3 == 0
    g = ac.case("shared_vertices").new[1][0]
    assert g.indices is not None and len(np.unique(g.indices)) < len(g.indices)


def test_neg_zero_and_degenerate_are_mesh_cases_meshes():
    z = ac.case("neg_zero").new[1][0].positions.view(np.uint32)
    assert (z == 0x80000000).any() and (z == 0).any()
    d = ac.case("degenerate").new[1][0]
    tri = d.positions[d.indices.reshape(-1, 3)]
    assert (np.abs(tri[:, 0] - tri[:, 1]).sum(axis=1) == 0).any()


def test_many_meshes_mixes_kinds_and_sizes():
    c = ac.case("many_meshes")
    new = c.new[1]
    assert len(new) == 40 and [_tris(m) for m in new] == mc.MANY_SIZES
    kinds = {(m.topology, m.indices is None) for m in new}
    assert kinds == {(0, False), (0, True), (1, False), (1, True)}
    assert sum(_tris(m) > ac.BVH_LDS_SHAPES for m in new) >= 2 and sum(_tris(m) <= ac.BVH_LDS_SHAPES for m in new) >= 2


def _grown(need, cap):
    return max(need, cap + cap // 2)


def test_three_calls_grows_twice_and_then_fits():
    """The header's capacity rule, by hand: upload leaves capacity = count; a call whose count passes the capacity
    takes max(count, 1.5 x capacity).  Arrays 0, 1 and 2 all grow in calls one and two and not in the third."""
    name = "three_calls"
    cap = _counts(ac.case(name).scenes[0].desc)[:3]
    moved = []
    for k in list(ac.steps(name))[1:]:
        need = _counts(ac.built(name, k))[:3]
        grew = [n > c for n, c in zip(need, cap)]
        cap = [_grown(n, c) if g else c for n, c, g in zip(need, cap, grew)]
        moved.append(grew)
    assert moved == [[True] * 3, [True] * 3, [False] * 3]


def test_emissive_new_spawns_an_emitter_from_new_primitives():
    name = "emissive_new"
    d0, d1 = ac.case(name).scenes[0].desc, ac.built(name, 1)
    assert _counts(d1)[8] == _counts(d0)[8] + 1
    assert _counts(d1)[3] == _counts(d0)[3] + ac.EMISSIVE_TRIS
    assert _counts(ac.add_only(name, 1).desc)[3:] == _counts(d0)[3:]


def test_deep_new_takes_the_stack_bound_to_17():
    from hikari_amd import scene_gbuffer_stack
    name = "deep_new"
    c = ac.case(name)
    before, between, after = c.scenes[0], ac.add_only(name, 1), c.scenes[1]
    ac.built(name, 1)
    assert dc.stack_need(before) <= ac.GB_STACK_LDS and dc.stack_need(between) == dc.stack_need(before)
    assert dc.stack_need(after) == ac.GB_STACK_LDS + 1
    assert scene_gbuffer_stack(after)[0] == ac.GB_STACK_LDS + 1


def test_stage_edge_add_passes_the_limit_by_the_add_alone():
    from hikari_amd import PLAN_LIGHT, scene_stage_bytes
    name = "stage_edge_add"
    c = ac.case(name)
    assert [_tris(m) for m in c.new[1]] == [1]
    b0, limit = scene_stage_bytes(c.scenes[0].desc, PLAN_LIGHT)
    b1, _ = scene_stage_bytes(ac.add_only(name, 1).desc, PLAN_LIGHT)
    b2, _ = scene_stage_bytes(ac.built(name, 1), PLAN_LIGHT)
    assert b0 == limit == 32768
    assert b1 == limit + 3 * 32 + 48 + 32  # three vertices, a primitive and a node
    assert b2 > b1


def test_then_update_rebuilds_another_tree():
    name = "then_update"
    c = ac.case(name)
    scene, ids = c.update
    assert ids == [1] and len(scene.meshes) == len(c.scenes[-1].meshes)
    index = ac.new_slices(name, 1)[0]
    a, b = mc.mesh_nodes(ac.built(name, 1), index), mc.mesh_nodes(ac.built_update(name), index)
    assert not np.array_equal(a["exit"], b["exit"])


def test_pool_tail_has_meshes_nobody_carries():
    c = ac.case("pool_tail")
    s0 = c.scenes[0]
    used = {mesh for mesh, _, _ in s0.instances}
    assert used == {0} and len(s0.meshes) == 3
    assert {mesh for mesh, _, _ in c.scenes[1].instances} == {0, 3}


# ------------------------------------------------------------------ hk_add_meshes_counts
@pytest.mark.parametrize("name", list(ac.CASES))
def test_counts_and_slices_equal_the_host_build(name):
    """For every step: the slices are the host builder's for the meshes added last (Scene.mesh_index, and what the
    instance records of the host build carry), arrays 0-2 count what the host build holds and the others stay."""
    from hikari_amd import add_meshes_counts
    c = ac.case(name)
    for k in list(ac.steps(name))[1:]:
        before = _counts(ac.built(name, k - 1))
        slices, after = add_meshes_counts(before, c.new[k])
        assert slices == [tuple(int(x) for x in s) for s in ac.new_slices(name, k)]
        host = _counts(ac.add_only(name, k).desc)
        assert after == host and after[3:] == before[3:]
        assert _counts(ac.built(name, k))[:3] == after[:3]
        carried = set(mc.mesh_slices(ac.built(name, k)))
        assert set(slices) <= carried
        for v, p, n0, nc in slices:
            assert nc == 3 * ((nc + 2) // 3) - 2
            assert len(dc.subtrees(mc.mesh_nodes(ac.built(name, k), (v, p, n0, nc)))) == 2 * ((nc + 2) // 3) - 1


def _raw_counts(descs, n=None, before=True, slices=True):
    from hikari_amd import _abi
    L = _abi.lib()
    count = len(descs) if n is None and descs is not None else (n or 0)
    arr = (_abi.hk_mesh_desc * max(1, count))(*(descs or [])) if descs is not None else None
    out = (_abi.hk_mesh_index * max(1, count))()
    after = (ctypes.c_uint32 * 9)()
    b = (ctypes.c_uint32 * 9)(*before) if before else None
    rc = L.hk_add_meshes_counts(b, arr, count, out if slices else None, after)
    return rc, L.hk_add_meshes_counts_error().decode()


def refusals(keep):
    """[(label, hk_mesh_desc list or None, count or None, the message's text)] of every refusal of the header; `keep`
    takes the arrays the descs point into."""
    from hikari_amd import _abi
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    uv = np.zeros((4, 2), np.float32)
    keep += [p, uv]

    def desc(positions=True, normals=True, uvs=True, vertices=4, indices=None, topology=0):
        ix = None if indices is None else np.asarray(indices, np.uint32)
        keep.append(ix)
        return _abi.hk_mesh_desc(p.ctypes.data if positions else None, p.ctypes.data if normals else None,
                                 uv.ctypes.data if uvs else None, vertices, None if ix is None else ix.ctypes.data,
                                 0 if ix is None else len(ix), topology)

    good = desc(indices=[0, 1, 2])
    return [
        ("null list", None, 1, "null mesh list"),
        ("no meshes", [], 0, "empty mesh list"),
        ("positions", [good, desc(positions=False, indices=[0, 1, 2])], None, "mesh 1: MissingAttributePosition"),
        ("normals", [desc(normals=False, indices=[0, 1, 2])], None, "MissingAttributeNormal"),
        ("uvs", [desc(uvs=False, indices=[0, 1, 2])], None, "MissingAttributeUV"),
        ("topology", [desc(indices=[0, 1, 2], topology=5)], None, "IncompatiblePrimitiveTopology"),
        ("list of 4 indices", [desc(indices=[0, 1, 2, 3])], None, "IncompatiblePrimitiveTopology"),
        ("list of 4 vertices", [desc()], None, "IncompatiblePrimitiveTopology"),
        ("strip of 2 indices", [desc(indices=[0, 1], topology=1)], None, "NoPrimitive"),
        ("list of no indices", [desc(indices=[])], None, "NoPrimitive"),
        ("strip of 2 vertices", [desc(vertices=2, topology=1)], None, "NoPrimitive"),
        ("index out of range", [good, desc(indices=[0, 1, 4])], None, "mesh 1: index out of range"),
    ]


BEFORE = [10, 5, 13, 0, 1, 1, 1, 0, 0]


def test_counts_refusals():
    from hikari_amd import _abi
    keep = []
    for label, descs, n, text in refusals(keep):
        rc, msg = _raw_counts(descs, n, BEFORE)
        assert rc == _abi.HK_ERR_INVALID and text in msg and "hk_add_meshes" in msg, (label, rc, msg)
    good = refusals(keep)[2][1][:1]
    rc, msg = _raw_counts(good, None, BEFORE, slices=False)
    assert rc == _abi.HK_ERR_INVALID and "null slices" in msg
    # totals past hk_update_meshes' bound of 0x40000000, in each of the three arrays
    for i in range(3):
        full = list(BEFORE)
        full[i] = 0x40000000 - 1
        rc, msg = _raw_counts(good, None, full)
        assert (rc == _abi.HK_ERR_INVALID and "too many" in msg) == (i == 0), (i, rc, msg)  # one primitive, one node: fit
        full[i] = 0x40000000
        rc, msg = _raw_counts(good, None, full)
        assert rc == _abi.HK_ERR_INVALID and "too many" in msg, (i, rc, msg)
    # a success clears the message
    rc, msg = _raw_counts(good, None, BEFORE)
    assert rc == _abi.HK_OK and msg == ""
    assert _abi.lib().hk_last_error(None) == b"null context"  # (that call is as it was)


def test_counts_of_a_valid_call_by_hand():
    from hikari_amd import Mesh, add_meshes_counts
    p = np.zeros((5, 3), np.float32)
    uv = np.zeros((5, 2), np.float32)
    meshes = [Mesh(p, p, uv, np.array([0, 1, 2, 2, 1, 3], np.uint32)), Mesh(p, p, uv, None, 1),
              Mesh(p[:3], p[:3], uv[:3], None, 0)]
    slices, after = add_meshes_counts(BEFORE, meshes)
    assert slices == [(10, 5, 13, 4), (15, 7, 17, 7), (20, 10, 24, 1)]
    assert after == [23, 11, 25] + BEFORE[3:]
