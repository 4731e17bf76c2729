"""Every case of tests/texture_cases.py sits where its name says, shown with the CPU oracle alone (the G-buffer's
material and uv planes, and whole frames against each case's nearest neighbour)."""
import numpy as np
import pytest

import texture_cases as tc
from texture_numpy import INT_MAX, INT_MIN, to_int


@pytest.fixture(scope="module")
def case_frames():
    cache = {}

    def get(key, make):
        if key not in cache:
            cache[key] = tc.frames(make())
        return cache[key]
    return get


def _places_of(scene):
    """[(material, slot, texture id)] of every valid id of a scene."""
    n = len(scene.textures)
    return [(m, slot, getattr(mat, slot)) for m, mat in enumerate(scene.materials) for slot in tc.SLOTS
            if getattr(mat, slot) is not None and getattr(mat, slot) < n]


def test_wrap_all_leaves_the_unit_square_and_samples_every_texture():
    triple = tc.wrap_all()
    scene = triple[0]
    t = scene.textures
    assert len(t) == 18
    assert sorted((x.address_u, x.address_v, x.filter) for x in t) == sorted(tc.SAMPLERS)
    assert all(x.rgba8.shape[0] != x.rgba8.shape[1] for x in t) and {x.srgb for x in t} == {True, False}
    sizes = [x.rgba8.shape[0] * x.rgba8.shape[1] for x in t]
    offsets = np.cumsum([0] + sizes[:-1])
    assert np.any(offsets % 2 == 1) and np.any(offsets % 4 == 2) and np.any(offsets % 4 == 3)
    places = _places_of(scene)
    assert sorted(p[2] for p in places) == list(range(18)) and {p[1] for p in places} == set(tc.SLOTS)
    mat, uv = tc.gbuffer(triple)
    covered = mat >= 0
    outside = covered & ((uv < 0) | (uv > 1)).any(axis=-1)
    assert outside.sum() > 0.25 * covered.sum(), (int(outside.sum()), int(covered.sum()))
    assert uv[covered].min() < -2.0 and uv[covered].max() > 3.0
    for m, slot, tid in places:  # every texture belongs to a material that covers pixels: retreive_surface samples it
        assert (mat == m).sum() > 0, (m, slot, tid)


def test_one_texel_shapes_meet_every_mode_and_filter():
    triple = tc.one_texel()
    scene = triple[0]
    seen = {}
    for x in scene.textures:
        h, w = x.rgba8.shape[:2]
        assert min(w, h) == 1
        seen.setdefault((w, h), []).append((x.address_u, x.address_v, x.filter))
    assert sorted(seen) == [(1, 1), (1, 6), (5, 1)]
    for shape, samplers in seen.items():
        assert sorted(samplers) == sorted(tc.SAMPLERS), shape  # all nine address pairs under both filters
    mat, uv = tc.gbuffer(triple)
    places = _places_of(scene)
    assert len(places) == 54 and {p[1] for p in places} == set(tc.SLOTS)
    for m, slot, tid in places:
        assert (mat == m).sum() > 0, (m, slot, tid)
    assert (((uv < 0) | (uv > 1)).any(axis=-1) & (mat >= 0)).sum() > 0.25 * (mat >= 0).sum()


def test_huge_uv_saturates_and_stays_finite(case_frames):
    triple = tc.huge_uv()
    scene = triple[0]
    mat, uv = tc.gbuffer(triple)
    reach = {}
    for m in (tc.BOX0, tc.BOX1):
        px = uv[mat == m]
        assert len(px) > 20
        w = min(scene.textures[getattr(scene.materials[m], s)].rgba8.shape[1] for s in tc.SLOTS)
        reach[m] = px[:, 0] * np.float32(w)
    assert reach[tc.BOX0].max() >= 1e6 and reach[tc.BOX0].min() <= -1e6 and np.abs(reach[tc.BOX0]).max() < 2.0 ** 31
    sat = to_int(np.floor(reach[tc.BOX1]))
    assert np.any(sat == INT_MAX) and np.any(sat == INT_MIN)  # the saturated branch, from both sides
    for planes, reservoirs in case_frames("huge_uv", tc.huge_uv):
        for oid in (0, 4, 5, 6, 7, 8, 9, 10):
            assert np.isfinite(planes[oid].view(np.float16).astype(np.float32)).all(), oid


def test_emitters_textured_black_slab_is_still_a_light(case_frames):
    """The alias table and the light BVH come from the untextured constants, so the all-black slab is still picked:
    its candidates carry zero radiance.  Making it dark by its constant instead removes it from the lights, and the
    frames change although neither slab emits anything."""
    import scene_ladder as sl
    scene = tc.emitters_textured()[0]
    scene.build()
    assert scene.desc.emissives.count == 3
    dark = tc.emitters_textured(black_by_constant=True)[0]
    dark.build()
    assert dark.desc.emissives.count == 2
    lit = case_frames("emitters_textured", tc.emitters_textured)
    assert not tc.same_frames(lit, case_frames("emitters_dark", lambda: tc.emitters_textured(black_by_constant=True)))
    assert not tc.same_frames(lit, case_frames("rung", lambda: sl.build(tc.RUNG)))
    # all three slabs are in view, so their emissive images are also sampled at the primary surface
    mat, _ = tc.gbuffer(tc.emitters_textured(), size=(32, 24))
    assert all((mat == m).sum() > 0 for m in (tc.SLAB0, tc.SLAB1, tc.SLAB2))
    t = scene.textures
    assert not t[1].rgba8[..., :3].any() and t[0].rgba8[:, :3, :3].max() == 0 and t[0].rgba8[:, 3:, :3].min() >= 128
    assert t[2].rgba8[..., 3].max() < 255 and len(np.unique(t[2].rgba8[..., 3])) > 3


def test_ids_past_the_end_are_untextured_and_a_normal_map_changes_nothing(case_frames):
    scene = tc.ids()[0]
    n = len(scene.textures)
    used = sorted({getattr(m, s) for m in scene.materials for s in tc.SLOTS + ("normal_map_texture",)
                   if getattr(m, s) is not None})
    assert used == [0, 1, n, n + 7] and all(getattr(scene.materials[tc.FLOOR], s) == 0 for s in tc.SLOTS)
    assert scene.materials[tc.SLAB0].emissive_texture is None  # U32_MAX in the record
    full = case_frames("ids", tc.ids)
    assert tc.same_frames(full, case_frames("ids_none_past", lambda: tc.ids(past_the_end=False)))
    assert tc.same_frames(full, case_frames("ids_no_normal", lambda: tc.ids(normal_map=False)))


def test_base_colour_alpha_is_carried_but_changes_no_frame(case_frames):
    """What the oracle shows: retreive_surface multiplies base_color.a by the texel's alpha, and nothing downstream of
    it reads base_color.a (light.wgsl shades with base_color.rgb only), so frames with alpha in [20, 254] equal the
    frames of the same images made opaque."""
    scene = tc.alpha()[0]
    assert all(t.rgba8[..., 3].max() < 255 and t.rgba8[..., 3].min() >= 20 for t in scene.textures)
    assert tc.same_frames(case_frames("alpha", tc.alpha), case_frames("alpha_opaque", lambda: tc.alpha(opaque=True)))


@pytest.mark.parametrize("name", list(tc.CASES))
def test_case_differs_from_its_nearest_neighbour(case_frames, name):
    assert not tc.same_frames(case_frames(name, tc.CASES[name]), case_frames("n_" + name, tc.NEIGHBOURS[name]))


def test_swap_sequence_changes_count_and_sizes():
    triple, uploads = tc.swap_uploads()
    counts = [len(t) for t, _ in uploads]
    assert counts == [18, 5, 0, 18] and sum(n for _, n in uploads) == 8
    top = max(getattr(m, s) for m in triple[0].materials for s in tc.SLOTS if getattr(m, s) is not None)
    assert top == 17  # ids 5..17 are past the end under B, all of them under none
    a, b = uploads[0][0], uploads[1][0]
    assert {t.rgba8.shape[:2] for t in a}.isdisjoint({t.rgba8.shape[:2] for t in b})


def test_gains_texture_gives_and_takes():
    case, _, _ = tc.gains_texture()
    before, after = case.scenes[0].materials, case.scenes[1].materials
    assert before[tc.FLOOR].base_color_texture == 0 and after[tc.FLOOR].base_color_texture is None
    assert before[tc.BOX0].base_color_texture is None and after[tc.BOX0].base_color_texture == 1
    assert before[tc.SLAB0].emissive_texture is None and after[tc.SLAB0].emissive_texture == 1
    assert case.materials and case.previous[1] == list(range(len(case.scenes[0].instances)))
    assert len(case.scenes[0].textures) == 3
    f0 = tc.frames((case.scenes[0], *tc.wrap_all()[1:]))
    f1 = tc.frames((case.scenes[1], *tc.wrap_all()[1:]))
    assert not tc.same_frames(f0, f1)
