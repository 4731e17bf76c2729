"""hk_tree_costs (csrc/hk_dynamic.hip k_tree_cost) against hks_tree_cost, itself held to tests/tree_cost_numpy.py by
tests/test_tree_cost_independent.py: every field of every out equal, on the trees the device holds after an upload, an
instance refit, an instance rebuild and a BLAS refit, over the cases of tests/instance_refit_cases.py and
tests/refit_cases.py.  The device TLAS and BLAS carry their shapes' boxes in the leaves where the host's are empty: the
rule reads no leaf box.

What the sizes exist for in k_tree_cost: one launch lays the TLAS, the light BVH and the listed slices end to end, a
thread per node, 256 per workgroup, 64 per wave.
  n1_m0 / n1_m1 / n2           lone leaves (no entry node, all zeros), no light BVH at all, one pair of entries
  many_meshes, all 40 listed   slices of 1, 4, 7 ... 5,998 nodes: many slices inside one wave (the lane-by-lane adds),
                               slices that straddle waves and workgroups, one that spans 23 workgroups
  86 / 87 triangles            256 and 259 nodes with nothing in front: one slice exactly fills workgroup 0, the next
                               starts on workgroup 1's first thread and crosses into workgroup 2
  many_large                   a TLAS of 5,998 nodes: most waves whole inside one slice (the register sum)
The shared checks (arrays, frames, planes, rays, stream, raw calls) are tests/scene_edits.py's.
"""
import ctypes

import numpy as np
import pytest

import instance_refit_cases as ic
import mesh_cases as mc
import refit_cases as rc
import tree_cost_numpy as tc
from parity import hip_runtime, host_scene_array, passes, renderer
from scene_edits import INST_DT, EditFrames, caller_stream, device_arrays, raw_call

pytestmark = pytest.mark.gpu

BLAS_REFIT_CASES = ["small_32", "small_35", "tris_1", "tris_2", "tris_2600", "deep_65", "folded", "many_meshes"]


def _slices(desc):
    return tc.known_slices(host_scene_array(desc, 4, INST_DT))


def host_costs(desc, ids=None) -> dict:
    """What tree_costs(ids) has to return for the scene `desc`, by hks_tree_cost; ids=None: every known slice."""
    from hikari_amd import tree_cost
    known = _slices(desc)
    asset = host_scene_array(desc, 2, tc.NODE_DT)
    ids = range(len(known)) if ids is None else ids
    return {"tlas": tree_cost(host_scene_array(desc, 5, tc.NODE_DT)),
            "lights": tree_cost(host_scene_array(desc, 7, tc.NODE_DT)),
            "meshes": [tree_cost(asset[known[i][0]: known[i][0] + known[i][1]]) for i in ids]}


def assert_costs(r, desc, ids=None, label=""):
    want = host_costs(desc, ids)
    got = r.tree_costs(range(len(want["meshes"])) if ids is None else ids)
    assert got == want, (label, got, want)
    return got


def raw(r, ids=(), tlas=True, lights=True, meshes=True, stream=None, null_ids=False):
    """hk_tree_costs with any out left NULL: (return code, message, {name: TreeCost or [TreeCost]})."""
    from hikari_amd import TreeCost, _abi
    ids = np.ascontiguousarray(ids, np.uint32)
    fill = lambda: _abi.hk_tree_cost(11, 12, 13.0, 14)  # (what an untouched out still holds)
    t, l, m = fill(), fill(), (_abi.hk_tree_cost * max(len(ids), 1))(*[fill() for _ in range(max(len(ids), 1))])
    id_ptr = None if null_ids or not len(ids) else ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    code, msg = raw_call(r, "hk_tree_costs", id_ptr, len(ids), t if tlas else None, l if lights else None,
                         m if meshes else None, stream)
    out = {"tlas": TreeCost.from_c(t), "lights": TreeCost.from_c(l), "meshes": [TreeCost.from_c(m[j]) for j in range(len(ids))]}
    return code, msg, out


# ------------------------------------------------------------------ device equals host
@pytest.mark.parametrize("name", ic.ARRAY_CASES)
def test_instance_cases_after_upload_refit_and_rebuild(name):
    scene0, scene1 = ic.case(name)
    r = renderer(scene0)
    assert_costs(r, scene0.desc, label="upload")
    r.update_instances(scene1.instance_models(), scene1.instance_local_aabbs(), refit=True)
    kept = assert_costs(r, ic.refitted(name), label="hk_refit_instances")
    r.update_instances(scene1.instance_models(), scene1.instance_local_aabbs())
    built = assert_costs(r, ic.built1(name), label="hk_update_instances")
    n, m = ic.COUNTS[name]
    assert (built["tlas"].entries, built["lights"].entries) == (max(2 * n - 2, 0), max(2 * m - 2, 0))
    if name in ("swapped", "many_large", "over_lds", "deep"):  # (tests/test_tree_cost_cases.py, now from the device)
        assert kept["tlas"].total() > 2.0 * built["tlas"].total()
    r.close()


@pytest.mark.parametrize("name", rc.ARRAY_CASES)
def test_mesh_cases_after_upload_and_blas_refit(name):
    scene0, scene1 = rc.case(name)
    r = renderer(scene0)
    got = assert_costs(r, scene0.desc, label="upload")
    assert len(got["meshes"]) == len(_slices(scene0.desc))
    if name in BLAS_REFIT_CASES:
        source = rc.update_source(name, 1)
        r.update_meshes(source, rc.listed(name), local_aabbs=mc.local_aabbs(source), refit=True)
        after = assert_costs(r, rc.refitted(name), label="hk_refit_meshes")
        if name == "many_meshes":
            assert len(after["meshes"]) == len(mc.MANY_SIZES) + 1  # all 40 and the light's quad, in one launch
            assert sorted(c.entries for c in after["meshes"][:-1]) == sorted(2 * t - 2 for t in mc.MANY_SIZES)
        if name in ("folded", "tris_2600"):
            assert after["meshes"][0] != got["meshes"][0]
    r.close()


def _two_row_meshes():
    a, b = mc._row_soup(86), mc._row_soup(87)
    scene0, _ = mc._pair([(a, a), (b, b)], [(0, mc._centred()), (1, mc._centred(0.5))])
    scene0.build()
    return scene0


def test_a_slice_that_fills_a_workgroup_and_one_that_crosses_it():
    scene = _two_row_meshes()
    known = _slices(scene.desc)
    assert [n for _, n in known[:2]] == [256, 259]
    r = renderer(scene)
    want = host_costs(scene.desc, [0, 1])["meshes"]
    code, _, got = raw(r, [0, 1], tlas=False, lights=False)  # nothing in front: slice 0 is workgroup 0
    assert code == 0 and got["meshes"] == want and want[0].entries == 170 and want[1].entries == 172
    code, _, got = raw(r, [1, 0], tlas=False, lights=False)  # 259 first: slice 1 starts three threads into workgroup 1
    assert code == 0 and got["meshes"] == want[::-1]
    assert_costs(r, scene.desc)
    r.close()


# ------------------------------------------------------------------ call shapes
def test_mesh_ids_empty_repeated_and_reversed():
    name = "many_meshes"
    scene0, _ = rc.case(name)
    r = renderer(scene0)
    n = len(_slices(scene0.desc))
    assert_costs(r, scene0.desc, [])
    assert_costs(r, scene0.desc, list(range(n))[::-1])
    assert_costs(r, scene0.desc, [3, 3, 5, 3, 0, 5, n - 1, n - 1])
    assert_costs(r, scene0.desc, [17] * 9)
    r.close()


def test_each_out_may_be_null():
    from hikari_amd import TreeCost
    name = "lights_at_35"
    scene0, _ = ic.case(name)
    r = renderer(scene0)
    want = host_costs(scene0.desc, [0])
    untouched = TreeCost(11, 12, 13.0, 14)
    for skip in ("tlas", "lights", "meshes", None):
        code, _, got = raw(r, [0], **({skip: False} if skip else {}))
        assert code == 0
        for key in ("tlas", "lights", "meshes"):
            assert got[key] == ([untouched] if key == "meshes" else untouched) if key == skip else got[key] == want[key], (skip, key)
    code, _, got = raw(r, [0], tlas=False, lights=False, meshes=False)
    assert code == 0 and got["tlas"] == untouched
    r.close()


def test_a_scene_without_emitters_gives_zeros_for_the_lights():
    from hikari_amd import TreeCost
    for name in ("n1_m0", "deep"):
        scene0, _ = ic.case(name)
        r = renderer(scene0)
        assert r.scene_counts()[7] == 0
        got = assert_costs(r, scene0.desc)
        assert got["lights"] == TreeCost(0, 0, 0.0, 0)
        code, _, only = raw(r, tlas=False, meshes=False)  # nothing to launch at all
        assert code == 0 and only["lights"] == TreeCost()
        r.close()


# ------------------------------------------------------------------ state
def test_two_queries_in_a_row_give_the_same_words():
    """A stale accumulator would double the second."""
    scene0, _ = ic.case("many_large")
    r = renderer(scene0)
    first = assert_costs(r, scene0.desc)
    for _ in range(3):
        assert r.tree_costs(range(len(first["meshes"]))) == first
    assert r.tree_costs([0])["tlas"] == first["tlas"]  # and a smaller query on the larger one's scratch
    r.close()


def test_a_query_leaves_the_nine_arrays_and_the_capacities_alone():
    """All nine arrays byte for byte across a query between two frames; and a steady query allocates nothing: the scene's
    capacities and the device's free memory stand still from the second query on."""
    from hikari_amd import HikariSettings, Upscale, frame_inputs
    name = "moving"
    scene0, _ = ic.case(name)
    cam, lights = ic.camera_for(name)
    w, h = ic.FRAME_SIZE
    r = renderer(scene0, (w, h))
    s = HikariSettings(upscale=Upscale.SMAA_TU_1_0).to_c()
    passes(r, s, frame_inputs(0, cam, lights, w, h))
    before, capacity = device_arrays(r), r.scene_capacity()
    n = len(_slices(scene0.desc))
    assert_costs(r, scene0.desc)
    assert device_arrays(r) == before and r.scene_capacity() == capacity
    passes(r, s, frame_inputs(1, cam, lights, w, h))
    assert device_arrays(r) == before
    hip = hip_runtime()
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t)] * 2
    seen = []
    for _ in range(3):
        r.tree_costs(range(n))
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        seen.append(free.value)
        assert r.scene_capacity() == capacity
    assert seen[0] == seen[1] == seen[2]
    r.close()


def test_frames_with_a_query_before_each_equal_the_oracles():
    """moving at 64 x 48: two frames on scene0, the refit, two more, a query before every frame and one on a refitted
    context: the frames are the oracle's, which knows no query, and the ray counters too."""
    name = "moving"
    scene0, scene1 = ic.case(name)
    d1 = ic.refitted(name)
    with EditFrames(scene0, ic.camera_for(name), ic.FRAME_SIZE) as fr:
        for f in range(4):
            if f == 2:
                fr.r.update_instances(scene1.instance_models(), scene1.instance_local_aabbs(), refit=True)
                fr.set_scene(d1)
            assert_costs(fr.r, scene0.desc if f < 2 else d1, label=f"frame {f}")
            fi = fr.inputs()
            passes(fr.r, fr.s, fi)
            assert_costs(fr.r, scene0.desc if f < 2 else d1, [0], label=f"after frame {f}")  # before the readback
            passes(fr.o, fr.s, fi)
            fr.compare()


# ------------------------------------------------------------------ interface
def test_refusals_leave_the_context_as_it_was():
    from hikari_amd import HikariError, HikariRenderer, TreeCost, _abi
    scene0, _ = rc.case("one_of_three")
    empty = HikariRenderer(0)
    code, msg, _ = raw(empty)
    assert code == _abi.HK_ERR_STATE and "no scene" in msg
    with pytest.raises(HikariError, match="no scene"):
        empty.tree_costs()
    empty.close()
    assert _abi.lib().hk_tree_costs(None, None, 0, None, None, None, None) == _abi.HK_ERR_INVALID

    r = renderer(scene0)
    n = len(_slices(scene0.desc))
    before = device_arrays(r)
    untouched = TreeCost(11, 12, 13.0, 14)
    for ids in ([n], [0, 1, n + 7], [0xFFFFFFFF]):
        code, msg, got = raw(r, ids)
        assert code == _abi.HK_ERR_INVALID and "hk_tree_costs" in msg and str(ids[-1]) in msg, ids
        assert got["tlas"] == untouched and got["meshes"][0] == untouched  # nothing was written
    code, msg, _ = raw(r, [n], meshes=False)  # an id is checked whether its out is asked for or not
    assert code == _abi.HK_ERR_INVALID
    code, msg, _ = raw(r, [0, 1], null_ids=True)
    assert code == _abi.HK_ERR_INVALID and "hk_tree_costs" in msg
    with pytest.raises(HikariError, match="hk_tree_costs"):
        r.tree_costs([n])
    assert device_arrays(r) == before
    assert_costs(r, scene0.desc)
    r.close()


def test_a_query_on_a_caller_stream():
    scene0, scene1 = ic.case("many_large")
    r = renderer(scene0)
    with caller_stream() as (stream, _):
        want = host_costs(scene0.desc)
        assert r.tree_costs(range(len(want["meshes"])), stream=stream) == want
        r.update_instances(scene1.instance_models(), scene1.instance_local_aabbs(), stream, refit=True)
        want = host_costs(ic.refitted("many_large"))
        assert r.tree_costs(range(len(want["meshes"])), stream=stream) == want
        assert r.tree_costs(range(len(want["meshes"]))) == want  # and on the context's own again
        r.close()


def test_the_plugin_forwards_the_query():
    from hikari_amd import HikariPlugin
    scene0, _ = ic.case("moving")
    p = HikariPlugin(scene0)
    want = host_costs(scene0.desc)
    assert p.tree_costs(range(len(want["meshes"]))) == want
    assert p.tree_costs() == {**want, "meshes": []}
    p.renderer.close()


def test_the_timed_span_is_named():
    scene0, _ = ic.case("over_256")
    r = renderer(scene0)
    r.enable_kernel_timing(True)
    r.tree_costs([0])
    assert "tree_costs" in r.kernel_timing()
    r.close()


# ------------------------------------------------------------------ the policy
def test_refit_policy_rebuilds_the_stale_tree_and_keeps_the_good_one():
    """swapped: the kept TLAS costs 4.1 times its build: the policy rebuilds and the arrays are the host-built scene1's;
    moving (1.08): the refit stands.  The same trees by hks_tree_cost: tests/test_tree_cost_cases.py."""
    from hikari_amd import RefitPolicy
    from parity import assert_rebuild_bitwise
    for name, stale, desc in (("swapped", ["tlas"], ic.built1("swapped")), ("moving", [], ic.refitted("moving"))):
        scene0, scene1 = ic.case(name)
        r = renderer(scene0)
        policy = RefitPolicy(2.0)
        assert policy.update_instances(r, scene1.instance_models(), scene1.instance_local_aabbs()) == stale
        assert_rebuild_bitwise(r, desc)
        assert policy.at_build == policy.totals(host_costs(desc if stale else scene0.desc, []))
        assert policy.update_instances(r, scene1.instance_models(), scene1.instance_local_aabbs()) == []  # nothing moved since
        r.close()
