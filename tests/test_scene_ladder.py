"""The scene ladder (tests/scene_ladder.py) on the CPU: every rung's position on the LDS staging axis from the
library's own arithmetic (hk_scene_stage_bytes, hk_scene_gbuffer_stack), a Python sum over the desc counts as a
second opinion, and the emitter conditions from the oracle alone."""
import functools

import numpy as np
import pytest

import scene_ladder as sl

LIMIT = 32768  # LDS_SCENE_MAX
ROUND = 16384  # one round of stage_scene's copy loop: 4 x 256 chunks of 16 bytes
STACK_BUDGET = LIMIT + 16384  # launch_gbuffer: scene + levels * 2048 <= this, or the staged walk has no LDS stack


def _sizes(name):
    from hikari_amd import PLAN_GBUFFER, PLAN_LIGHT, scene_gbuffer_stack, scene_stage_bytes
    scene, _, _ = sl.built(name)
    (L, lim_l), (G, lim_g) = scene_stage_bytes(scene, PLAN_LIGHT), scene_stage_bytes(scene, PLAN_GBUFFER)
    assert lim_l == lim_g == LIMIT
    need, levels = scene_gbuffer_stack(scene)
    assert levels == 16
    return L, G, need


# rung -> (L, G, G-buffer stack bound): the committed positions
EXPECTED = {
    "no_emitters": (8480, 11552, 9),
    "odd_alias": (9856, 13216, 9),
    "emitters_3": (11760, 15200, 10),
    "one_triangle": (576, 448, 0),
    "round_edge": (16384, 21952, 12),
    "two_rounds": (16400, 21888, 11),
    "mid": (24016, 32224, 11),
    "light_at_limit": (32768, 44480, 11),
    "light_over_limit": (32784, 44576, 12),
    "gbuffer_at_limit": (32800, 32768, 14),
    "gbuffer_over_limit": (24400, 32784, 14),
    "gbuffer_no_stack_room": (21776, 29712, 13),
}


def test_every_rung_has_its_committed_size():
    assert list(EXPECTED) == list(sl.RUNGS)
    assert {n: _sizes(n) for n in sl.RUNGS} == EXPECTED


def test_rungs_sit_where_the_table_says():
    """The table's conditions, from hk_scene_stage_bytes / hk_scene_gbuffer_stack and the built arrays."""
    S = {n: _sizes(n) for n in sl.RUNGS}
    D = {n: sl.built(n)[0].desc for n in sl.RUNGS}
    d = D["no_emitters"]
    assert (d.alias_table.count, d.emissive_nodes.count, d.emissives.count) == (0, 0, 0) and S["no_emitters"][0] < ROUND
    d = D["odd_alias"]
    assert d.emissives.count == 1 and d.alias_table.count % 2 == 1 and (d.alias_table.count * 8) % 16 == 8
    assert S["odd_alias"][0] < ROUND
    d = D["emitters_3"]
    pairs = sorted((int(a), int(b)) for a, b in _alias_ranges(d))
    assert pairs == [(0, 3), (3, 5), (8, 7)], pairs
    assert d.emissive_nodes.count == 7 and S["emitters_3"][0] < ROUND  # 3n - 2 nodes: inner nodes
    d = D["one_triangle"]
    assert (d.instances.count, d.instance_nodes.count, d.asset_nodes.count, d.primitives.count, d.emissives.count) == \
        (1, 1, 1, 1, 1)
    assert S["round_edge"][0] == ROUND
    assert S["two_rounds"][0] == ROUND + 16
    L = S["mid"][0]
    assert ROUND < L < LIMIT and (L // 16) % 256 != 0 and D["mid"].emissives.count >= 3
    assert S["light_at_limit"][0] == LIMIT and D["light_at_limit"].emissives.count >= 3
    assert S["light_over_limit"][0] == LIMIT + 16
    assert sl.RUNGS["light_over_limit"]["emitters"] == sl.RUNGS["light_at_limit"]["emitters"]
    assert S["gbuffer_at_limit"][1] == LIMIT and S["gbuffer_at_limit"][0] > LIMIT      # stages the G-buffer plan only
    assert S["gbuffer_over_limit"][1] == LIMIT + 16 and S["gbuffer_over_limit"][0] <= LIMIT  # ... the light plan only
    L, G, need = S["gbuffer_no_stack_room"]
    assert G <= LIMIT and need <= 16 and G + need * 2048 > STACK_BUDGET
    # and a staged G-buffer walk whose LDS stack does follow the scene, ending past LDS_SCENE_MAX within the budget
    L, G, need = S["round_edge"]
    assert LIMIT < G + need * 2048 <= STACK_BUDGET


def _alias_ranges(desc):
    import ctypes as C
    raw = np.frombuffer(C.string_at(desc.emissives.data, desc.emissives.count * 64), np.uint32).reshape(-1, 16)
    k = _c_layout()["alias_words"]
    return [(r[k], r[k + 1]) for r in raw]


@functools.lru_cache(maxsize=None)
def _c_layout() -> dict:
    """include/hk_types.h as the C compiler sees it: the struct sizes, and the word offset of hk_emissive.alias_table
    (offset, count)."""
    import subprocess
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    names = ("hk_vertex", "hk_primitive", "hk_node", "hk_alias_entry", "hk_instance", "hk_material", "hk_emissive")
    with tempfile.TemporaryDirectory() as tmp:
        src = Path(tmp) / "layout.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hk_types.h"\nint main(void){'
                       'printf("alias_words %zu\\n", offsetof(hk_emissive, alias_table) / 4);' +
                       "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "return 0;}")
        exe = Path(tmp) / "layout"
        subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    return {k: int(v) for k, v in zip(out[::2], out[1::2])}


@pytest.mark.parametrize("name", list(sl.RUNGS))
def test_python_sum_of_struct_sizes_gives_the_same_bytes(name):
    """L and G again as a plain sum: desc counts x the hk_types.h struct sizes (as the C compiler sees them), each
    array rounded up to 16 bytes; the wide node layouts hold 64 bytes per node."""
    c = _c_layout()
    vertex, primitive, node, alias, instance, material, emissive = (
        c[n] for n in ("hk_vertex", "hk_primitive", "hk_node", "hk_alias_entry", "hk_instance", "hk_material",
                       "hk_emissive"))
    assert (vertex, primitive, node, alias, instance, material, emissive) == (32, 48, 32, 8, 176, 80, 64)
    d = sl.built(name)[0].desc

    def up(b):
        return (b + 15) // 16 * 16

    L = sum(up(a.count * size) for a, size in (
        (d.vertices, vertex), (d.primitives, primitive), (d.asset_nodes, node), (d.alias_table, alias),
        (d.instances, instance), (d.instance_nodes, node), (d.materials, material), (d.emissive_nodes, node),
        (d.emissives, emissive)))
    G = sum(up(a.count * size) for a, size in (
        (d.vertices, vertex), (d.primitives, primitive), (d.instances, instance), (d.asset_nodes, 64),
        (d.instance_nodes, 64)))
    assert (L, G) == _sizes(name)[:2]


def test_stage_bytes_rejects_bad_arguments():
    import ctypes as C

    from hikari_amd import _abi
    L = _abi.lib()
    d = sl.built("one_triangle")[0].desc
    b = C.c_uint32()
    assert L.hk_scene_stage_bytes(None, 0, C.byref(b), None) == _abi.HK_ERR_INVALID
    assert L.hk_scene_stage_bytes(C.byref(d), 2, C.byref(b), None) == _abi.HK_ERR_INVALID
    assert L.hk_scene_stage_bytes(C.byref(d), 0, None, None) == 0
    assert L.hk_scene_gbuffer_stack(None, C.byref(b), None) == _abi.HK_ERR_INVALID


@pytest.mark.parametrize("name", sl.LIT_RUNGS)
def test_emitters_light_the_rung(name):
    """From the oracle alone, at the GPU tests' size and settings: emitter walks happen, the tone-mapped frame
    differs from the same geometry without emission, and on the multi-emitter rungs every emitter is some
    pixel's visible surface in a reservoir sample (sample_position.w holds visible_instance)."""
    frames, counters = sl.reference(name)
    if name == "one_triangle":
        # its only surface is the emitter itself, and select_light_candidate skips the emitter a point lies on
        # (`instance != emissive.instance`, light.wgsl:638), so no point can walk an emitter: the rung has
        # a light and nothing to light.  Its emission is still in the frame (checked below).
        assert counters["traverse_emitter"] == 0 and counters["traverse_top"] > 0
    else:
        assert counters["traverse_emitter"] > 0
    dark, _ = sl.reference(name, emissive=False, frames=2)
    assert not np.array_equal(frames[1][0][10], dark[1][0][10])
    lit = frames[-1][0][10].view(np.float16).astype(np.float32)
    assert np.isfinite(lit).all()
    if name in sl.MULTI_EMITTER_RUNGS:
        seen = set()
        for res in frames[-1][1]:
            seen |= set(np.unique(res[:, 11].view(np.float32)).astype(np.int64).tolist())
        emitters = sl.emitter_instances(sl.built(name)[0])
        assert len(emitters) == len(sl.RUNGS[name]["emitters"])
        assert set(emitters) <= seen, (emitters, sorted(seen))


def test_no_emitters_renders_finite_frames_without_emitter_walks():
    frames, counters = sl.reference("no_emitters")
    assert counters["traverse_emitter"] == 0 and counters["traverse_top"] > 0
    assert np.isfinite(frames[-1][0][10].view(np.float16).astype(np.float32)).all()
