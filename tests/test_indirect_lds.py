"""The indirect pass's LDS per workgroup, without a GPU: hk_scene_indirect_lds (the launcher's own sizes) against the
staged bytes of hk_scene_stage_bytes, for cornell and the scene-ladder rungs around the staging limit."""
import pytest

import scene_ladder as sl

STASH = 256 * 68  # IndStash: four float4 and one word per thread


def _sizes(scene):
    from hikari_amd import PLAN_LIGHT, scene_indirect_lds, scene_stage_bytes
    (L, lim), (stash, total, wg_max) = scene_stage_bytes(scene, PLAN_LIGHT), scene_indirect_lds(scene)
    return L, lim, stash, total, wg_max


@pytest.mark.parametrize("name", ["round_edge", "light_at_limit", "light_over_limit"])
def test_rung_stash_fits_the_launch(name):
    """Staged bytes plus stash stay within what one workgroup may allocate; the rung past the limit stages nothing."""
    scene, _, _ = sl.built(name)
    L, lim, stash, total, wg_max = _sizes(scene)
    staged = L <= lim
    assert staged == (name != "light_over_limit")
    assert stash == STASH and total == (L if staged else 0) + STASH
    assert total <= wg_max == 65536
    if name == "light_at_limit":
        assert (L, total) == (32768, 32768 + STASH)


def test_cornell_indirect_workgroup():
    """Cornell's staged indirect workgroup: 9456 bytes of scene and the stash, six to a CU's 160 KiB of LDS."""
    from hikari_amd import examples
    scene, _, _ = examples.cornell()
    L, lim, stash, total, _ = _sizes(scene)
    assert (L, stash, total) == (9456, STASH, 9456 + STASH) and L <= lim
    assert (160 * 1024) // total == 6


def test_indirect_lds_rejects_null():
    import ctypes as C

    from hikari_amd import _abi
    b = C.c_uint32()
    assert _abi.lib().hk_scene_indirect_lds(None, C.byref(b), None, None) == _abi.HK_ERR_INVALID
