"""The cases of tests/mesh_set_cases.py sit where their names say, by the host builder alone, and hk_set_meshes_counts,
the host arithmetic of hk_set_meshes' list, gives the host build's slices and counts for every case and step and returns
the refusals of the header that need no context.  Needs no GPU."""
import ctypes

import numpy as np
import pytest

import dynamic_cases as dc
import instance_set_cases as ic
import mesh_cases as mc
import mesh_set_cases as sc
from parity import host_scene_array

PRIM_DT = np.dtype((np.void, 48))


def _tris(mesh) -> int:
    n = len(mesh.positions) if mesh.indices is None else len(mesh.indices)
    return n - 2 if mesh.topology == 1 else n // 3


def _counts(desc) -> list:
    return ic.desc_counts(desc)


def _sizes(name, k) -> list:
    return [_tris(m) for m in sc.case(name).scenes[k].meshes]


def _instanced(scene) -> set:
    return {mesh for mesh, _, _ in scene.instances}


# ------------------------------------------------------------------ the edges
@pytest.mark.parametrize("name, gone", [("drop_first", [0]), ("drop_middle", [2]), ("drop_last", [3]),
                                        ("drop_all_but_one", [1, 2, 3])])
def test_drop_cases_drop_the_named_mesh_and_its_instance(name, gone):
    c = sc.case(name)
    s0, s1 = c.scenes
    assert len(s0.meshes) == 4 and len(set(_sizes(name, 0))) == 4  # four meshes of different sizes
    kept = sc.kept_in(name, 1)
    assert None not in kept and sorted(set(range(4)) - set(kept)) == gone and kept == sorted(kept)
    assert _instanced(s0) == set(range(4))
    assert _instanced(s1) == set(range(len(s1.meshes)))  # the dropped meshes' instances went with them
    assert len(s1.instances) == len(s0.instances) - len(gone)


def test_swap_two_overlaps_source_and_destination():
    name = "swap_two"
    assert sc.kept_in(name, 1) == [0, 2, 1] and len(set(_sizes(name, 0)[1:])) == 2
    before, after = sc.slices(name, 0), sc.slices(name, 1)
    # the mesh that moves forward lands on bytes the other one still has to be read from, in all three arrays
    (v_a, p_a, n_a, c_a), (v_b, p_b, n_b, c_b) = before[1], before[2]
    v_to, p_to, n_to, c_to = after[1]
    assert (v_b, p_b, n_b, c_b)[3] == c_to and (v_to, p_to, n_to) == (v_a, p_a, n_a)
    assert n_to < n_a + c_a and n_a < n_to + c_to  # destination of b meets source of a
    v2, p2, n2, _ = after[2]
    assert n2 < n_b + c_b and n_b < n2 + c_a       # destination of a meets source of b
    assert sc.case(name).previous[1] == list(range(len(sc.case(name).scenes[1].instances)))


def test_identity_keeps_every_slice_where_it_is():
    name = "identity"
    assert sc.kept_in(name, 1) == [0, 1, 2]
    assert [e[0] for e in sc.entries(name, 1)] == sc.slices(name, 1) == sc.slices(name, 0)
    for i in range(9):
        dt = np.dtype((np.void, 1))
        assert host_scene_array(sc.built(name, 0), i, dt).tobytes() == host_scene_array(sc.built(name, 1), i, dt).tobytes()


@pytest.mark.parametrize("name, at", [("insert_front", 0), ("insert_middle", 2)])
def test_insert_cases_put_a_new_mesh_ahead_of_kept_ones(name, at):
    kept = sc.kept_in(name, 1)
    assert kept[at] is None and kept.count(None) == 1 and len(kept) == 4
    assert any(j is not None for j in kept[at + 1:])
    assert _sizes(name, 1)[at] == sc.INSERT_TRIS
    before, after = sc.slices(name, 0), sc.slices(name, 1)
    moved = [after[k] != before[j] for k, j in enumerate(kept) if j is not None]
    assert any(moved) and (all(moved) if at == 0 else not moved[0])


@pytest.mark.parametrize("name", list(sc.REPLACE))
def test_replace_cases_change_the_triangle_count_in_place(name):
    c = sc.case(name)
    n0, n1 = sc.REPLACE[name]
    assert _sizes(name, 0)[1] == n0 and _sizes(name, 1)[1] == n1 and (n1 > n0) == (name == "replace_more")
    assert sc.kept_in(name, 1) == [0, None, 2]
    s0, s1 = c.scenes
    i = s1.keys.index("e_m0")
    assert c.previous[1][i] == s0.keys.index("e_m0")          # the instance carries `previous`
    assert s1.instances[i][0] == 1 and not np.array_equal(s1.instances[i][2], s0.instances[c.previous[1][i]][2])
    assert sc.slices(name, 1)[2] != sc.slices(name, 0)[2]     # the mesh behind it moves


def test_replace_across_lds_builds_both_variants():
    name = "replace_across_lds"
    assert _sizes(name, 0)[1:] == [sc.BVH_LDS_SHAPES, sc.BVH_LDS_SHAPES + 1]
    assert _sizes(name, 1)[1:] == [sc.BVH_LDS_SHAPES + 1, sc.BVH_LDS_SHAPES]
    assert sc.kept_in(name, 1) == [0, None, None]


def test_one_triangle_kept_is_one_node_between_larger_ones():
    name = "one_triangle_kept"
    sizes = _sizes(name, 1)
    assert sizes[2] == 1 and sizes[1] > 1 and sizes[3] > 1
    v, p, n0, nc = sc.slices(name, 1)[2]
    assert nc == 1 and len(sc.case(name).scenes[1].meshes[2].positions) == 3  # 2 / 3 / 2 chunks of vertices: 6
    assert sc.kept_in(name, 1) == [0, 2, 3, 4] and sc.slices(name, 1)[2] != sc.slices(name, 0)[3]


def test_chunk_edges_by_the_table_arithmetic():
    """k_move_mesh_slices: thread t of the vertices' chunks moves chunk t, a vertex is 2 chunks, a wave 64 lanes, a
    workgroup 256 threads.  The kept slices begin at lane 8 of a wave, on thread 256 and at lane 60."""
    name = "chunk_edges"
    starts = [2 * v for v, _, _, _ in sc.slices(name, 1)]
    assert starts == [0, 8, 256, 316]
    assert starts[1] % 64 == 8 and starts[2] % 256 == 0 and starts[2] > 0 and starts[3] % 64 == 60
    assert 2 * _counts(sc.built(name, 1))[0] > 256  # more than one workgroup of vertex chunks
    # the primitives' and nodes' chunks follow: their first threads, and the kept slices' there
    n_v, n_p, n_n = _counts(sc.built(name, 1))[:3]
    prim0, node0 = 2 * n_v, 2 * n_v + 3 * n_p
    p_starts = [prim0 + 3 * p for _, p, _, _ in sc.slices(name, 1)]
    n_starts = [node0 + 2 * n for _, _, n, _ in sc.slices(name, 1)]
    assert any(t % 64 for t in p_starts) and any(t % 64 for t in n_starts)
    assert None not in sc.kept_in(name, 1) and sc.slices(name, 1)[0] != sc.slices(name, 0)[1]


def test_trailing_vertices_exceed_what_the_primitives_index():
    name = "trailing_vertices"
    m = sc.case(name).scenes[1].meshes[1]
    need = int(np.asarray(m.indices).max()) + 1
    assert len(m.positions) >= need + sc.TRAILING  # (the grid may leave a corner vertex unused itself)
    (index, count) = sc.entries(name, 1)[1]
    assert count == len(m.positions) > need and index == sc.slices(name, 0)[2]
    # the host builder concatenates them: the next mesh begins behind them
    assert sc.slices(name, 1)[2][0] == sc.slices(name, 1)[1][0] + count


def test_pooled_cases_have_meshes_nobody_carried():
    c = sc.case("pooled_kept")
    assert _instanced(c.scenes[0]) == {0, 1} and len(c.scenes[0].meshes) == 4
    assert sc.kept_in("pooled_kept", 1) == [0, 2, 1]           # m1, pooled so far, kept ahead of m0; m2 gone
    assert _instanced(c.scenes[1]) == {0, 1, 2}
    d = sc.case("pooled_dropped")
    assert _instanced(d.scenes[0]) == {0, 2} and sc.kept_in("pooled_dropped", 1) == [0, 2]


def test_many_meshes_drops_every_second_and_interleaves_five():
    name = "many_meshes"
    c = sc.case(name)
    assert _sizes(name, 0)[1:] == mc.MANY_SIZES and len(c.scenes[0].meshes) == 41
    kept = sc.kept_in(name, 1)
    assert kept.count(None) == 5 and sorted(j for j in kept if j is not None) == [0] + list(range(1, 41, 2))
    new_at = [k for k, j in enumerate(kept) if j is None]
    assert new_at == [1, 5, 9, 13, 17] and [_sizes(name, 1)[k] for k in new_at] == list(sc.MANY_NEW)
    assert sum(n > sc.BVH_LDS_SHAPES for n in sc.MANY_NEW) == 1


def test_emissive_moved_moves_an_emitters_primitives():
    name = "emissive_moved"
    d0, d1 = sc.built(name, 0), sc.built(name, 1)
    assert _counts(d0)[8] == _counts(d1)[8] == 2
    assert _counts(d0)[3] == _counts(d1)[3] == 2 + sc.EMISSIVE_TRIS
    assert sc.slices(name, 1)[1][1] < sc.slices(name, 0)[2][1]  # its primitives begin earlier now
    assert sc.kept_in(name, 1) == [0, 2]


def test_deep_dropped_brings_the_stack_bound_to_16():
    from hikari_amd import scene_gbuffer_stack
    name = "deep_dropped"
    c = sc.case(name)
    sc.built(name, 1)
    assert dc.stack_need(c.scenes[0]) == sc.GB_STACK_LDS + 1 == scene_gbuffer_stack(c.scenes[0])[0]
    assert dc.stack_need(c.scenes[1]) <= sc.GB_STACK_LDS
    assert sc.kept_in(name, 1) == [0, 2]


def test_stage_edge_drop_returns_within_the_limit():
    from hikari_amd import PLAN_LIGHT, scene_stage_bytes
    name = "stage_edge_drop"
    b0, limit = scene_stage_bytes(sc.built(name, 0), PLAN_LIGHT)
    b1, _ = scene_stage_bytes(sc.built(name, 1), PLAN_LIGHT)
    assert b1 == limit == 32768 and b0 == limit + 3 * 32 + 48 + 32
    assert _sizes(name, 0)[-1] == 1 and None not in sc.kept_in(name, 1)
    assert len(sc.case(name).scenes[0].meshes) - 1 not in _instanced(sc.case(name).scenes[0])


def test_shrink_then_grow_fits_the_old_capacity():
    name = "shrink_then_grow"
    c0, c1, c2 = (_counts(sc.built(name, k))[:3] for k in range(3))
    assert all(b < a for a, b in zip(c0, c1)) and all(b < c <= a for a, b, c in zip(c0, c1, c2))
    assert sc.kept_in(name, 2) == [0, 1, None]


def test_the_after_calls():
    assert sc.case("then_add").after[0] == "add" and len(sc.case("then_add").after[1]) == 1
    kind, scene, ids = sc.case("then_update").after
    assert kind == "update" and ids == [2]
    assert sc.kept_in("then_update", 1) == [0, 3, 2]  # the mesh it deforms was moved by the step
    index = sc.slices("then_update", 1)[2]
    a, b = mc.mesh_nodes(sc.built("then_update", 1), index), mc.mesh_nodes(sc.built_after("then_update"), index)
    assert not np.array_equal(a["exit"], b["exit"])
    kind, scene, previous = sc.case("then_set_instances").after
    assert kind == "set" and None in previous and any(p is not None for p in previous)


# ------------------------------------------------------------------ hk_set_meshes_counts
@pytest.mark.parametrize("name", list(sc.CASES))
def test_counts_and_slices_equal_the_host_build(name):
    """For every step: the slices are the host builder's for the list (Scene.mesh_index, and what the host build's
    instance records carry), counts 0-2 what the host build holds; 3-8 are `before`'s (they follow the set)."""
    from hikari_amd import set_meshes_counts
    for k in list(sc.steps(name))[1:]:
        before = _counts(sc.built(name, k - 1))
        slices, after = set_meshes_counts(before, sc.entries(name, k))
        assert slices == [tuple(int(x) for x in s) for s in sc.slices(name, k)]
        host = _counts(sc.built(name, k))
        assert after[:3] == host[:3] and after[3:] == before[3:]
        assert set(mc.mesh_slices(sc.built(name, k))) <= set(slices)
        for v, p, n0, nc in slices:
            assert len(dc.subtrees(mc.mesh_nodes(sc.built(name, k), (v, p, n0, nc)))) == 2 * ((nc + 2) // 3) - 1


def kept(v, p, n0, nc, vertices):
    from hikari_amd import _abi
    return _abi.hk_mesh_entry(None, _abi.hk_mesh_index(v, p, (ctypes.c_uint32 * 2)(n0, nc)), vertices)


def new(desc, keep):
    from hikari_amd import _abi
    keep.append(desc)
    return _abi.hk_mesh_entry(ctypes.pointer(desc), _abi.hk_mesh_index(0, 0, (ctypes.c_uint32 * 2)(0, 0)), 0)


BEFORE = [10, 5, 13, 0, 1, 1, 1, 0, 0]
A, B = (0, 0, 0, 4, 4), (4, 2, 4, 7, 6)  # two kept slices that fit BEFORE: 2 and 3 triangles


def refusals(keep):
    """[(label, hk_mesh_entry list or None, count or None, the message's text)] of every refusal that needs no context;
    `keep` takes what the entries point into."""
    from test_mesh_add_cases import refusals as add_refusals
    out = [("null list", None, 1, "null mesh list"), ("no meshes", [], 0, "empty mesh list")]
    for label, descs, n, text in add_refusals(keep)[2:]:
        out.append((label, [kept(*A)] + [new(d, keep) for d in descs], None, text.replace("mesh 1", "mesh 2")))
    return out + [
        ("not 3k - 2", [kept(0, 0, 0, 5, 4)], None, "mesh 0: kept slice refused: its BLAS is not 3k - 2 nodes"),
        ("primitives past", [kept(*A), kept(4, 4, 4, 4, 4)], None, "mesh 1: kept slice refused: its primitives reach past"),
        ("nodes past", [kept(0, 0, 10, 4, 4)], None, "kept slice refused: its nodes reach past"),
        ("vertices begin past", [kept(10, 0, 0, 4, 1)], None, "kept slice refused: its vertices begin past"),
        ("no vertices", [kept(0, 0, 0, 4, 0)], None, "vertex_count does not cover"),
        ("vertices past", [kept(8, 0, 0, 4, 3)], None, "vertex_count reaches past the vertex array"),
        ("kept twice", [kept(*A), kept(*B), kept(*A)], None, "mesh 2: the slice is kept twice"),
        ("overlap", [kept(*A), kept(4, 1, 4, 4, 4)], None, "mesh 1: it partly overlaps another kept slice"),
        ("vertices into another", [kept(0, 0, 0, 4, 6), kept(*B)], None,
         "mesh 1: vertex_count reaches into another kept slice's vertices"),
    ]


def raw_counts(entries, n=None, before=BEFORE, slices=True):
    from hikari_amd import _abi
    L = _abi.lib()
    count = len(entries) if n is None and entries is not None else (n or 0)
    arr = (_abi.hk_mesh_entry * max(1, count))(*(entries or [])) if entries is not None else None
    out = (_abi.hk_mesh_index * max(1, count))()
    after = (ctypes.c_uint32 * 9)()
    b = (ctypes.c_uint32 * 9)(*before) if before else None
    rc = L.hk_set_meshes_counts(b, arr, count, out if slices else None, after)
    got = [(s.vertex, s.primitive, s.node[0], s.node[1]) for s in out[:count]]
    return rc, L.hk_set_meshes_counts_error().decode(), got, list(after)


def test_counts_refusals():
    from hikari_amd import _abi
    keep = []
    for label, entries, n, text in refusals(keep):
        rc, msg, _, _ = raw_counts(entries, n)
        assert rc == _abi.HK_ERR_INVALID and text in msg and msg.startswith("hk_set_meshes: "), (label, rc, msg)
    rc, msg, _, _ = raw_counts([kept(*A)], slices=False)
    assert rc == _abi.HK_ERR_INVALID and "null slices" in msg
    rc, msg, _, _ = raw_counts([kept(*A)], before=None)
    assert rc == _abi.HK_ERR_INVALID and "null counts" in msg
    # totals past 0x40000000: two kept slices of 0x30000000 vertices each
    big = [0x70000000] + BEFORE[1:]
    rc, msg, _, _ = raw_counts([kept(0, 0, 0, 1, 0x30000000), kept(0x30000000, 1, 1, 1, 0x30000000)], before=big)
    assert rc == _abi.HK_ERR_INVALID and "too many" in msg
    rc, msg, _, _ = raw_counts([kept(0, 0, 0, 1, 0x20000000), kept(0x30000000, 1, 1, 1, 0x20000000)], before=big)
    assert rc == _abi.HK_OK and msg == ""  # exactly 0x40000000 fits, and a success clears the message
    assert _abi.lib().hk_add_meshes_counts_error() == b""  # (hk_add_meshes_counts' message is its own)


def test_counts_of_a_valid_call_by_hand():
    from hikari_amd import Mesh, _abi
    from hikari_amd.plugin import _mesh_descs
    p = np.zeros((5, 3), np.float32)
    uv = np.zeros((5, 2), np.float32)
    descs, hold = _mesh_descs([Mesh(p, p, uv, None, 1)])  # a strip of 5 vertices: 3 triangles, 7 nodes
    keep = []
    rc, msg, slices, after = raw_counts([kept(*B), new(descs[0], keep), kept(*A)])
    assert rc == _abi.HK_OK and msg == ""
    assert slices == [(0, 0, 0, 7), (6, 3, 7, 7), (11, 6, 14, 4)]
    assert after == [15, 8, 18] + BEFORE[3:]
