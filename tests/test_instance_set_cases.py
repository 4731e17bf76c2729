"""The cases of tests/instance_set_cases.py on the CPU: each sits where its name says, proven from the host builder's
arrays alone, and hk_instance_set_counts (the host arithmetic hk_set_instances sizes its allocations and launches with)
gives the host-built desc's nine counts on every case and step, and refuses what the header says it refuses."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import instance_set_cases as ic
import scene_ladder as sl

ROOT = Path(__file__).resolve().parent.parent


def _steps(name):
    return list(ic.steps(name))


@pytest.mark.parametrize("name", list(ic.CASES))
def test_counts_equal_the_host_build(name):
    """hk_instance_set_counts on the uploaded desc (step 0) and step k's instance list: the nine counts of step k's
    own host build, with 3n - 2 TLAS nodes and 3m - 2 (or no) light-BVH nodes."""
    from hikari_amd import instance_set_counts
    c = ic.case(name)
    for k in _steps(name):
        want = ic.desc_counts(ic.built(name, k))
        got = instance_set_counts(c.scenes[0], c.scenes[k], materials=c.materials)
        assert got == want, (name, k, got, want)
        n, m = want[4], want[8]
        assert n == len(c.scenes[k].instances) and want[5] == 3 * n - 2 and want[7] == (3 * m - 2 if m else 0)
        assert m == len(sl.emitter_instances(c.scenes[k]))
        assert want[:3] == ic.desc_counts(ic.built(name, 0))[:3] and want[6] == len(c.scenes[0].materials)


def test_previous_maps_follow_the_keys():
    c = ic.case("despawn_middle")
    assert c.previous == [None, [0, 1, 3, 4]]
    assert ic.case("spawn_copies").previous[1] == [0, 1, 2, 3, None, None]
    assert ic.case("emitters_3_5_7").previous[2] == [None, 0, 1, 2, 3, 4]
    assert ic.case("from_one_129").previous[1] == [None] * 40 + [0] + [None] * 88


def test_despawn_middle_shifts_the_emitter_behind():
    em0, em1 = (ic.emissive_records(ic.built("despawn_middle", k)) for k in (0, 1))
    assert em0[:, 8].tolist() == [1, 3] and em1[:, 8].tolist() == [1, 2]
    assert em0[:, 10:12].tolist() == em1[:, 10:12].tolist() == [[0, 3], [3, 5]]
    assert ic.desc_counts(ic.built("despawn_middle", 1))[4] == 4


def test_spawn_copies_grows_every_rebuilt_array():
    a, b = (ic.desc_counts(ic.built("spawn_copies", k)) for k in (0, 1))
    assert a[4] == 4 and b[4] == 6
    assert all(b[i] > a[i] for i in (3, 4, 5, 7, 8)) and a[8] == 1 and b[8] == 2
    assert ic.desc_counts(ic.built("there_and_back", 2)) == a and ic.desc_counts(ic.built("there_and_back", 1)) == b


def test_spawn_pooled_instances_a_mesh_unused_at_upload():
    import mesh_cases as mc
    c = ic.case("spawn_pooled")
    used0 = set(mc.mesh_slices(ic.built("spawn_pooled", 0)))
    pooled = c.scenes[0].mesh_index(1)
    assert pooled not in used0 and pooled in set(mc.mesh_slices(ic.built("spawn_pooled", 1)))
    # the pooled slice lies between instanced ones in all three arrays
    lo, hi = c.scenes[0].mesh_index(0), c.scenes[0].mesh_index(2)
    assert all(lo[j] < pooled[j] < hi[j] for j in range(3))


def test_emitter_off_and_on_are_one_to_none_and_back():
    assert [ic.desc_counts(ic.built("emitter_off", k))[8] for k in (0, 1)] == [1, 0]
    assert [ic.desc_counts(ic.built("emitter_on", k))[8] for k in (0, 1)] == [0, 1]
    off = ic.desc_counts(ic.built("emitter_off", 1))
    assert off[3] == off[7] == off[8] == 0
    # the same instance list but for one material index
    a, b = ic.case("emitter_on").scenes
    assert [(x[0], x[1]) != (y[0], y[1]) for x, y in zip(a.instances, b.instances)] == [False, False, True, False]


def test_materials_replaced_flips_emitters_by_the_records_alone():
    c = ic.case("materials_replaced")
    assert c.materials and [i[:2] for i in c.scenes[0].instances] == [i[:2] for i in c.scenes[1].instances]
    assert sl.emitter_instances(c.scenes[0]) == [1, 3, 4, 6] and sl.emitter_instances(c.scenes[1]) == [2, 6]
    e1 = [m.emissive for m in c.scenes[1].materials]
    assert e1[3][3] == 0.0 and np.isnan(e1[4][1]) and np.isnan(e1[5][3]) and np.isnan(c.scenes[0].materials[5].emissive[0])
    assert ic.emissive_records(ic.built("materials_replaced", 1))[:, 8].tolist() == [2, 6]


def test_emitters_3_5_7_alias_offsets():
    k = ic.EMITTERS_FRONT
    want = [[[0, 3], [3, 5], [8, 7]], [[0, 3], [3, 7]], [[0, k], [k, 3], [k + 3, 7]]]
    inst = [[0, 2, 4], [0, 3], [0, 1, 4]]
    for step in range(3):
        em = ic.emissive_records(ic.built("emitters_3_5_7", step))
        assert em[:, 10:12].tolist() == want[step] and em[:, 8].tolist() == inst[step]


@pytest.mark.parametrize("name", list(ic.CARRY))
def test_carry_edges(name):
    n, at = ic.CARRY[name]
    c = ic.case(name)
    assert len(c.scenes[0].instances) == n + 1 and len(c.scenes[1].instances) == n
    assert sl.emitter_instances(c.scenes[0]) == [at + 1, at + 2, n - 1]
    assert sl.emitter_instances(c.scenes[1]) == [at, at + 1, n - 2]
    assert (at + 1) % 64 == 0 and (name != "chunk_edge" or (at + 1) % 256 == 0)
    assert ic.emissive_records(ic.built(name, 1))[:, 10:12].tolist() == [[0, 3], [3, 5], [8, 2]]


def test_tlas_size_edges():
    assert [ic.desc_counts(ic.built("to_one", k))[4:6] for k in (0, 1)] == [[3, 7], [1, 1]]
    assert [ic.desc_counts(ic.built("from_one_129", k))[4] for k in (0, 1)] == [1, ic.COOP_MIN + 1]
    assert [ic.desc_counts(ic.built("lds_build_edge", k))[4] for k in (0, 1, 2)] == [
        ic.BVH_LDS_SHAPES, ic.BVH_LDS_SHAPES + 1, ic.BVH_LDS_SHAPES]


def test_stage_edge_leaves_lds_staging_and_returns():
    from hikari_amd import PLAN_LIGHT, scene_stage_bytes
    sizes = [scene_stage_bytes(ic.built("stage_edge", k), PLAN_LIGHT) for k in (0, 1, 2)]
    limit = sizes[0][1]
    assert limit == 32768 and [s[0] for s in sizes] == [limit, limit + 176 + 96, limit]


def test_deeper_blas_moves_the_stack_bound_over_the_lds_levels():
    from hikari_amd import scene_gbuffer_stack
    need = [scene_gbuffer_stack(ic.built("deeper_blas", k))[0] for k in (0, 1, 2)]
    assert need[1] == ic.GB_STACK_LDS + 1 and need[0] == need[2] <= ic.GB_STACK_LDS, need
    assert need[1] == ic.dc.stack_need(ic.case("deeper_blas").scenes[1])


# ---- hk_instance_set_counts' refusals
def _raw_counts(desc, entries, count=None, materials=None):
    from hikari_amd import _abi
    arr = (_abi.hk_instance_desc * max(1, len(entries)))(*entries)
    out = (ctypes.c_uint32 * 9)()
    return _abi.lib().hk_instance_set_counts(ctypes.byref(desc), arr, len(entries) if count is None else count,
                                             materials, out), list(out)


def test_set_counts_refusals():
    from hikari_amd import _abi
    c = ic.case("spawn_pooled")
    scene = c.scenes[0]
    desc = scene.desc
    n_v, n_p, n_n = ic.desc_counts(desc)[:3]

    def entry(index, material=0):
        v, p, n0, nc = index
        return _abi.hk_instance_desc(_abi.hk_mesh_index(v, p, (ctypes.c_uint32 * 2)(n0, nc)), material, _abi.HK_INSTANCE_NEW)

    quad, pooled, last = (scene.mesh_index(i) for i in range(3))
    ok, counts = _raw_counts(desc, [entry(quad), entry(pooled, ic.LIT[0])])
    assert ok == _abi.HK_OK and counts[3:6] == [6, 2, 4] and counts[7:] == [1, 1]
    v, p, n0, nc = pooled
    refused = {
        "count 0": dict(entries=[entry(quad)], count=0),
        "material out of range": dict(entries=[entry(quad, len(scene.materials))]),
        "not 3k - 2 nodes": dict(entries=[entry((v, p, n0, nc - 1))]),
        "no nodes": dict(entries=[entry((v, p, n0, 0))]),
        "partly overlapping the next slice": dict(entries=[entry((v, p + 1, n0 + 3, nc))]),
        "a part of an instanced slice": dict(entries=[entry((last[0], last[1] + 1, last[2] + 3, last[3] - 3))]),
        "two new slices that overlap": dict(entries=[entry(pooled), entry((v, p + 1, n0 + 3, nc - 3))]),
        "primitives past the array": dict(entries=[entry((last[0], n_p - 1, last[2], last[3]))]),
        "nodes past the array": dict(entries=[entry((last[0], last[1], n_n - 1, last[3]))]),
        "vertices past the array": dict(entries=[entry((n_v, p, n0, nc))]),
        "vertex indices past the array": dict(entries=[entry((n_v - 1, p, n0, nc))]),
    }
    for label, kw in refused.items():
        rc, _ = _raw_counts(desc, **kw)
        assert rc == _abi.HK_ERR_INVALID, (label, rc)
    assert _abi.lib().hk_instance_set_counts(None, None, 1, None, None) == _abi.HK_ERR_INVALID


# ---- the interface
def test_header_documents_and_abi_binds_the_entry_points():
    from hikari_amd import HikariPlugin, HikariRenderer, _abi
    header = (ROOT / "include" / "hikari_amd.h").read_text()
    assert re.search(r"#define\s+HK_ABI_VERSION\s+3\b", header) and _abi.lib().hk_abi_version() == 3
    assert re.search(r"#define\s+HK_INSTANCE_NEW\s+0xFFFFFFFFu", header) and _abi.HK_INSTANCE_NEW == 0xFFFFFFFF
    for name in ("hk_set_instances", "hk_scene_counts", "hk_instance_set_counts"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _abi.EXPORTED_SYMBOLS and getattr(_abi.lib(), name).argtypes is not None
    assert ctypes.sizeof(_abi.hk_instance_desc) == 24
    for text in ("HK_INSTANCE_NEW", "Capacity", "1.5 x capacity", "EMPTY set", "registered on first use"):
        assert text in header, text
    assert callable(HikariRenderer.set_instances) and callable(HikariRenderer.scene_counts)
    assert callable(HikariPlugin.set_instances)
