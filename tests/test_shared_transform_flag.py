"""hks_shared_transform, the bitwise compare behind hk_scene_shared_transform, without a GPU: true only for one or
more matrices that all hold the same bits.  The walks reuse one instance's local ray for every instance where it is
true, so a value compare (0.0 == -0.0) would be wrong."""
import numpy as np
import pytest


def _models(name):
    from hikari_amd import examples
    return examples.SCENES[name]()[0].instance_models()


@pytest.fixture(scope="module")
def cornell():
    m = _models("cornell")
    assert m.shape == (8, 16) and m.dtype == np.float32
    return m


def _flag(models):
    from hikari_amd import shared_transform
    return shared_transform(models)


def test_true_for_cornell_and_for_one_matrix(cornell):
    assert _flag(cornell) is True
    assert _flag(cornell[:1]) is True
    assert _flag(np.eye(4, dtype=np.float32).reshape(1, 16)) is True


def test_false_without_a_matrix(cornell):
    import ctypes

    from hikari_amd import _abi
    assert _flag(np.zeros((0, 16), np.float32)) is False
    L = _abi.lib()
    assert L.hks_shared_transform(None, 0) == 0 and L.hks_shared_transform(None, 3) == 0
    assert L.hks_shared_transform(cornell.ctypes.data_as(ctypes.c_void_p), 0) == 0


@pytest.mark.parametrize("name", ["scene", "city"])
def test_false_for_scenes_with_several_transforms(name):
    assert _flag(_models(name)) is False


@pytest.mark.parametrize("k", [0, 3, 7])
def test_false_one_ulp_away(cornell, k):
    m = cornell.copy()
    e = int(np.flatnonzero(m[k] != 0)[0])
    m[k, e] = np.nextafter(m[k, e], np.float32(np.inf))
    assert m[k, e] != cornell[k, e]
    assert _flag(m) is False


@pytest.mark.parametrize("k", [0, 3, 7])
def test_false_for_a_zero_of_the_other_sign(cornell, k):
    m = cornell.copy()
    zeros = np.flatnonzero((m[k] == 0) & ~np.signbit(m[k]))
    assert len(zeros), "cornell's model has no +0.0 entry"
    m[k, zeros[0]] = np.float32(-0.0)
    assert np.array_equal(m, cornell)  # equal by value ...
    assert _flag(m) is False           # ... and not by bits


def test_false_when_only_the_first_or_the_last_matrix_differs(cornell):
    for k in (0, len(cornell) - 1):
        m = cornell.copy()
        m[k, 15 if k else 12] += np.float32(0.25)  # the last float of the last block, the translation of the first
        assert _flag(m) is False
    # NaN payloads count: the same payload everywhere is shared, another payload in one place is not
    m = cornell.copy()
    m.view(np.uint32)[:, 5] = 0x7FC00001
    assert _flag(m) is True
    m.view(np.uint32)[7, 5] = 0x7FC00002
    assert _flag(m) is False


def test_header_abi_and_renderer_expose_the_property():
    import re
    from pathlib import Path

    from hikari_amd import HikariRenderer, _abi
    root = Path(__file__).resolve().parents[1]
    header = (root / "include" / "hikari_amd.h").read_text()
    assert re.search(r"\bint\s+hk_scene_shared_transform\s*\(", header)
    assert re.search(r"\bshared_xform \(1\)", header)
    assert re.search(r"\bint\s+hks_shared_transform\s*\(", (root / "include" / "hikari_scene.h").read_text())
    for name in ("hk_scene_shared_transform", "hks_shared_transform"):
        assert name in _abi.EXPORTED_SYMBOLS and getattr(_abi.lib(), name).argtypes is not None
    assert callable(HikariRenderer.scene_shared_transform)
    keys, i = [], 0
    while _abi.lib().hk_option_name(i) is not None:
        keys.append(_abi.lib().hk_option_name(i).decode())
        i += 1
    assert "shared_xform" in keys
