"""GPU parity for the traversal kernels' fixed costs: the wave counters summed by ballots and bit planes (wave_count)
and the closest-hit form of the bounce walk (traverse_top<false>), plus the indirect kernel with its LDS stash on the
scene-ladder rungs around the staging limit.  Everything is exact, so every case is bit for bit against the CPU oracle,
ray counters included.  tests/test_indirect_lds.py holds the device-free part (the LDS budget per scene).
"""
import numpy as np
import pytest

import scene_ladder as sl
from parity import renderer, run_frames, run_static

pytestmark = pytest.mark.gpu


def _settings(bounces=1):
    from hikari_amd import HikariSettings, Upscale
    return HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_bounces=bounces)


def _rung_against_reference(name, bounces=1, wavefront=False):
    """A renderer of the ladder rung over the ladder's frames against the stored oracle frames and counters."""
    from hikari_amd import frame_inputs
    scene, cam, lights = sl.built(name)
    r = renderer(scene, sl.SIZE, wavefront=wavefront)
    run_frames(r, sl.reference(name, bounces), sl.ladder_settings(bounces).to_c(),
               (frame_inputs(f, cam, lights, *sl.SIZE) for f in range(sl.FRAMES)))


# ------------------------------------------------------------------ counters
@pytest.mark.parametrize("size", [(63, 47), (64, 64), (256, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_counters_equal_oracle(size):
    """Cornell, frames 0-3: partial waves and an odd width (63 x 47), whole tiles (64 x 64) and many workgroups with
    all-background waves among them (256 x 256).  Every plane, reservoir and ray counter equals the oracle's."""
    run_static("cornell", *size, _settings(), 4)


def test_counters_equal_oracle_many_bounces():
    """Eight bounces on cornell 64 x 64, the largest per-lane counts a frame kernel reaches.  Measured on the oracle's
    statistics build (per-pixel traverse_top calls of the indirect pass, frames 0-3): the largest is 10, and it stays
    10 with 10, 12 or 32 bounces (12 with every surface whitened to 0.98), because the bounce loop ends once the path's
    throughput falls under 0.01.  So no bounce count takes a frame kernel's lane to 16; the reduction past 16 per
    lane is driven directly in test_wave_count_reduction below."""
    run_static("cornell", 64, 64, _settings(8), 4)


def test_wave_count_reduction():
    """wave_count itself (hk_selftest_count) on given per-thread counts: nothing counted, bit-plane sums of counts
    under 16, waves in which one lane or every lane has 16 or more (the shuffle-tree fallback), large counts, a
    partial last workgroup, and a mix over many workgroups (more than the counter's 1024 shards hold one each)."""
    from hikari_amd import examples
    scene, _, _ = examples.cornell()
    r = renderer(scene, (16, 16))
    rng = np.random.default_rng(16)
    cases = {
        "zeros": np.zeros(256, np.uint32),
        "ones": np.ones(256, np.uint32),
        "under_16": rng.integers(0, 16, 1000).astype(np.uint32),
        "all_15": np.full(300, 15, np.uint32),
        "one_lane_16": np.where(np.arange(512) == 77, 16, rng.integers(0, 16, 512)).astype(np.uint32),
        "all_16": np.full(256, 16, np.uint32),
        "large": rng.integers(0, 1 << 31, 777).astype(np.uint32),
        "max": np.full(64, 0xFFFFFFFF, np.uint32),
        "single": np.array([5], np.uint32),
        "mixed": np.where(rng.random(300_001) < 0.02, rng.integers(16, 5000, 300_001),
                          rng.integers(0, 16, 300_001) * (rng.random(300_001) < 0.4)).astype(np.uint32),
    }
    for name, v in cases.items():
        assert r.selftest_count(v) == int(v.astype(np.uint64).sum()), name
    assert r.selftest_count(np.zeros(0, np.uint32)) == 0


# ------------------------------------------------------------------ walk form
WALK_CASES = {"one_bounce": dict(bounces=1), "two_bounces": dict(bounces=2), "wavefront": dict(bounces=1, wavefront=True)}


@pytest.mark.parametrize("lds", [0, 1], ids=["lds_off", "lds_default"])
@pytest.mark.parametrize("case", list(WALK_CASES))
def test_closest_hit_walk_cornell_bit_exact(hk_options, case, lds):
    """The bounce walks in closest-hit form (indirect_begin, indirect_multi_bounces, the k_wf_trace stage) on cornell
    64 x 64, frames 0-3, staged and unstaged: all buffers and counters bit-exact."""
    hk_options["lds_scene"] = lds
    c = WALK_CASES[case]
    run_static("cornell", 64, 64, _settings(c["bounces"]), 4, wavefront=c.get("wavefront", False))


@pytest.mark.parametrize("case", list(WALK_CASES))
def test_closest_hit_walk_unstaged_rung_bit_exact(case):
    """The same on the ladder's first unstaged rung (light_over_limit: the light plan is one chunk past the staging
    limit, so every walk reads global memory) under the ladder's settings, frames 0-5."""
    c = WALK_CASES[case]
    _rung_against_reference("light_over_limit", c["bounces"], c.get("wavefront", False))


# ------------------------------------------------------------------ LDS budget
@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("name", ["round_edge", "light_at_limit", "light_over_limit"])
def test_indirect_stash_rungs_bit_exact(hk_options, name, bounces):
    """k_indirect on its own (no merged launch) on the rungs at the end of stage_scene's first round, at the staging
    limit (the stash next to 32768 staged bytes) and one chunk past it (unstaged), with the one-bounce and the
    multi-bounce kernel: bit-exact, counters included."""
    hk_options["merge"] = 0
    _rung_against_reference(name, bounces)
