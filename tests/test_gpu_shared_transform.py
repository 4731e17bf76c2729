"""GPU parity for the walks' one local ray per walk (Scene::shared_xform): where every instance record carries the same
inverse_transpose_model bits, traverse_top computes the instance-local ray once before its loop instead of at every
instance entry (the G-buffer's closest_hit_ordered keeps the general walk: DESIGN section 4, round 9; its planes are
compared all the same).  Same visits, tests, hits and counters, so every case is bit for bit against
the CPU oracle on planes 0 to 16, the ten reservoir buffers and both ray counters, and every case asserts
hk_scene_shared_transform, so that none can pass by taking the general walk unnoticed (or the hoisted one wrongly)."""
import copy
import ctypes

import numpy as np
import pytest

from parity import RACY, compare_frame, orbit_camera, pair, passes, renderer, run_frames

pytestmark = pytest.mark.gpu

SIZES = [(63, 47), (64, 64)]


def _settings(**kw):
    from hikari_amd import HikariSettings, Upscale
    return HikariSettings(upscale=Upscale.SMAA_TU_1_0, **kw)


def _static(triple, size, st, frames, shared, options=None, wavefront=False, **run):
    """pair() and run_frames() under the scene's own camera, with the getter checked before and after."""
    from hikari_amd import frame_inputs
    w, h = size
    scene, cam, lights, r, o = pair(triple, w, h, st, options=options, wavefront=wavefront)
    assert r.scene_shared_transform() is shared
    run_frames(r, o, st.to_c(), (frame_inputs(f, cam, lights, w, h) for f in range(frames)), **run)
    assert r.scene_shared_transform() is shared
    return r, o


# the kernels a frame takes, forced by options: name -> (hk_set_option values, wavefront, indirect bounces)
PATHS = {
    "defaults": ({}, False, 1),
    "fused": ({"fuse_min_px": 0}, False, 1),
    "merged": ({"merge": 1}, False, 1),
    "lds_off": ({"lds_scene": 0}, False, 1),
    "lds_all": ({"lds_scene": 2}, False, 1),
    "wavefront": ({}, True, 1),
    "two_bounces": ({}, False, 2),
    "compact": ({"compact_emitter": 1, "compact_shadow": 1}, False, 1),
    "compact_fused": ({"compact_emitter": 1, "compact_shadow": 1, "fuse_min_px": 0, "merge": 0, "lds_scene": 0}, False, 1),
    "persistent": ({"persistent_indirect": 1}, False, 1),
}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("path", list(PATHS))
def test_cornell_every_kernel_path_bit_exact(hk_options, path, size):
    """Cornell (eight instances, one model matrix), frames 0-5 (both validation intervals), once per kernel path."""
    options, wavefront, bounces = PATHS[path]
    hk_options.update(options)
    _static("cornell", size, _settings(indirect_bounces=bounces), 6, True, wavefront=wavefront)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cornell_separate_direct_launches_bit_exact(hk_options, size):
    """An orbiting camera: the reprojection is no identity, so direct_lit and the emissive pass run as separate
    launches although the fused one is asked for.  Under motion the scatter into the previous spatial buffers is racy
    (parity.RACY at RACY_MIN_EXACT); with spatial reuse off nothing reads those records."""
    from hikari_amd import frame_inputs
    hk_options["fuse_min_px"] = 0
    w, h = size
    st = _settings(indirect_spatial_reuse=False)
    scene, cam, lights, r, o = pair("cornell", w, h, st)
    assert r.scene_shared_transform() is True
    errors, prev = [], None
    for f in range(6):
        c = orbit_camera(cam, f)
        fi = frame_inputs(f, c, lights, w, h, previous_camera=prev)
        prev = copy.deepcopy(c)
        for x in (r, o):
            passes(x, st.to_c(), fi)
        compare_frame(r, o, f, errors, racy=RACY if f >= 1 else ())
        if errors:
            break
    assert not errors, "\n".join(errors[:20])
    assert r.counters() == o.counters()


@pytest.mark.parametrize("path", ["defaults", "fused"])
def test_cornell_general_walk_with_the_option_off_bit_exact(hk_options, path):
    """shared_xform = 0 on a shared scene: the getter still reports the property, the walks take the general path."""
    hk_options.update(PATHS[path][0])
    hk_options["shared_xform"] = 0
    r, _ = _static("cornell", (63, 47), _settings(), 6, True)
    assert r.get_option("shared_xform") == 0.0


# ------------------------------------------------------------------ a shared transform that is no quarter turn
def _skewed_cornell():
    """Cornell with one extra transform on every instance (a rotation about a skew axis, a non-uniform scale, a
    translation) and the camera carried along, so the view is the box as before, seen through other numbers."""
    from hikari_amd import Camera, Transform, examples
    scene, cam, lights = examples.cornell()
    axis = np.array([0.3, 0.8, -0.52])
    axis /= np.linalg.norm(axis)
    a = 0.7
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)) @ np.diag([1.3, 0.8, 1.1])
    T[:3, 3] = [0.4, -0.3, 0.7]
    scene.instances = [(mesh, mat, T @ m) for mesh, mat, m in scene.instances]
    eye = T @ np.array([0.0, 1.0, 4.0, 1.0])
    target = T @ np.array([0.0, 1.0, 0.0, 1.0])
    return scene, Camera(Transform.from_xyz(*eye[:3]).looking_at(tuple(target[:3]))), lights


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_skewed_shared_transform_bit_exact(size):
    from hikari_amd import shared_transform
    triple = _skewed_cornell()
    models = triple[0].instance_models()
    assert shared_transform(models) and np.count_nonzero(models[0]) == 13  # nine linear entries, none zero
    r, o = _static(triple, size, _settings(), 4, True)
    covered = o.output(11).view(np.float32).reshape(-1, 4)[:, 3] > 0
    assert covered.mean() >= 0.2, covered.mean()  # (0.41 and 0.55 with the oracle when this was written)


# ------------------------------------------------------------------ transitions
def _with_models(models):
    """Cornell's (scene, camera, lights) with the given (n, 16) float32 column-major models, built."""
    from hikari_amd import examples
    scene, cam, lights = examples.cornell()
    scene.instances = [(mesh, mat, np.asarray(m, np.float64).reshape(4, 4).T)
                      for (mesh, mat, _), m in zip(scene.instances, models)]
    assert scene.instance_models().tobytes() == np.ascontiguousarray(models, np.float32).tobytes()
    scene.build()
    return scene, cam, lights


def _rotated_box(models, k, angle):
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    out = models.copy()
    out[k] = (rot @ models[k].astype(np.float64).reshape(4, 4).T).T.reshape(16).astype(np.float32)
    return out


def _one_ulp(models, k):
    out = models.copy()
    e = [i for i in (0, 1, 2, 4, 5, 6, 8, 9, 10) if out[k, i] != 0][0]  # a linear entry
    out[k, e] = np.nextafter(out[k, e], np.float32(np.inf))
    return out


def _zero_sign(models, k):
    out = models.copy()
    e = [i for i in (0, 1, 2, 4, 5, 6, 8, 9, 10) if out[k, i] == 0 and not np.signbit(out[k, i])][0]
    out[k, e] = np.float32(-0.0)
    return out


def _update_steps(steps, size=(63, 47), frames_each=2):
    """Upload cornell, then hk_update_instances with each later step's models: frames_each frames per step against the
    oracle on the host-built scene (one thread, spatial reuse off, the racy scatter targets within their tolerance:
    test_gpu_parity's instance update), the getter after every change, equal counters at the end."""
    from hikari_amd import frame_inputs, load_noise
    from oracle import Oracle
    w, h = size
    first = _with_models(steps[0][0])
    scene, cam, lights = first
    st = _settings(indirect_spatial_reuse=False)
    r = renderer(scene, size)
    o = Oracle(scene.desc, load_noise(), w, h, 1.0, threads=1)
    keep, errors, f = [first], [], 0
    for k, (models, shared) in enumerate(steps):
        if k:
            t = _with_models(models)
            keep.append(t)
            r.update_instances(t[0].instance_models(), t[0].instance_local_aabbs())
            o.set_scene(t[0].desc)
        assert r.scene_shared_transform() is shared, f"step {k}"
        for _ in range(frames_each):
            fi = frame_inputs(f, cam, lights, w, h)
            for x in (r, o):
                passes(x, st.to_c(), fi)
            compare_frame(r, o, f, errors, racy=RACY)
            f += 1
        assert not errors, f"step {k}\n" + "\n".join(errors[:10])
    assert r.counters() == o.counters()
    o.close()
    r.close()


def test_update_instances_on_off_on_bit_exact():
    """Frames 0-1 on cornell, 2-3 with the tall box turned by 0.2 rad, 4-5 with the first models again: a stale flag
    in either direction shows as a wrong getter, and a hoisted ray on the turned box as wrong frames."""
    from hikari_amd import examples
    m0 = examples.cornell()[0].instance_models()
    k = len(m0) - 2
    _update_steps([(m0, True), (_rotated_box(m0, k, 0.2), False), (m0, True)])


@pytest.mark.parametrize("near", ["one_ulp_first", "one_ulp_last", "zero_sign_first", "zero_sign_last"])
def test_near_misses_take_the_general_walk_bit_exact(near):
    """One instance's model one ulp away in one linear entry, or equal but for the sign of a zero: not shared."""
    from hikari_amd import examples, shared_transform
    m0 = examples.cornell()[0].instance_models()
    k = 0 if near.endswith("first") else len(m0) - 1
    m1 = (_one_ulp if near.startswith("one_ulp") else _zero_sign)(m0, k)
    assert (m1.view(np.uint32) != m0.view(np.uint32)).sum() == 1
    _update_steps([(m0, True), (m1, False)])
    # and uploaded as such, where the flag comes from what the walks read, the records' inverse_transpose_model: the
    # ulp survives the inversion, the sign of that zero does not (the eight inverses then hold the same bits, and one
    # local ray serves them exactly)
    triple = _with_models(m1)
    d = triple[0].desc
    itm = np.frombuffer(ctypes.string_at(d.instances.data, d.instances.count * 176), np.float32).reshape(-1, 44)[:, 24:40]
    assert shared_transform(itm) is near.startswith("zero_sign")
    _static(triple, (64, 64), _settings(), 2, shared_transform(itm))


def test_set_instances_despawn_on_spawn_off_bit_exact():
    """Cornell with one box turned (off); hk_set_instances despawns that box (on: the rest share the transform), then
    spawns it again, turned (off).  Frames against the oracle on the host-built scenes after each change."""
    from hikari_amd import examples, frame_inputs, load_noise
    from oracle import Oracle
    w, h = 64, 64
    base, cam, lights = examples.cornell()
    m0 = base.instance_models()
    n = len(m0)
    k = n - 2
    turned = _with_models(_rotated_box(m0, k, 0.2))[0]
    less = copy.copy(turned)
    less._h, less.desc = None, None
    less.instances = [x for i, x in enumerate(turned.instances) if i != k]
    less.build()
    again = copy.copy(turned)
    again._h, again.desc = None, None
    again.instances = list(less.instances) + [turned.instances[k]]
    again.build()
    st = _settings(indirect_spatial_reuse=False)
    r = renderer(turned, (w, h))
    o = Oracle(turned.desc, load_noise(), w, h, 1.0, threads=1)
    steps = [(turned, None, False), (less, [i for i in range(n) if i != k], True), (again, list(range(n - 1)) + [None], False)]
    errors, f = [], 0
    for step, (scene, previous, shared) in enumerate(steps):
        if step:
            r.set_instances(scene, previous=previous)
            o.set_scene(scene.desc)
        assert r.scene_shared_transform() is shared, f"step {step}"
        for _ in range(2):
            fi = frame_inputs(f, cam, lights, w, h)
            for x in (r, o):
                passes(x, st.to_c(), fi)
            compare_frame(r, o, f, errors, racy=RACY)
            f += 1
        assert not errors, f"step {step}\n" + "\n".join(errors[:10])
    assert r.counters() == o.counters()
    o.close()
    r.close()


# ------------------------------------------------------------------ an instance of an empty mesh
EMPTIED = 6  # cornell's short box: no emitter, in view


def test_empty_mesh_instance_is_not_entered_bit_exact():
    """Cornell with the short box's record given an empty BLAS range (mesh.node[1] = 0: the builder itself refuses an
    empty mesh, so the built record is patched).  Its TLAS leaf still passes box tests; the walks must not enter it,
    and the ray counters and frames say whether one did."""
    from hikari_amd import _abi, examples, frame_inputs, load_noise
    from oracle import Oracle
    scene, cam, lights = examples.cornell()
    d = scene.build()
    n = d.instances.count
    rec = np.frombuffer(ctypes.string_at(d.instances.data, n * 176), np.uint8).reshape(n, 176).copy()
    words = rec.view(np.uint32).reshape(n, 44)
    k = EMPTIED
    assert words[k, 43] > 0
    words[k, 43] = 0  # hk_instance::mesh.node[1]
    patched = _abi.hk_scene_desc()
    ctypes.memmove(ctypes.byref(patched), ctypes.byref(d), ctypes.sizeof(d))
    patched.instances = _abi.hk_array(rec.ctypes.data_as(ctypes.c_void_p), n)
    scene.desc = patched
    r, o = _static((scene, cam, lights), (63, 47), _settings(), 4, True)
    # the instance is in view: with the box in place the G-buffer differs
    scene2, _, _ = examples.cornell()
    o2 = Oracle(scene2.build(), load_noise(), 63, 47, 1.0)
    o2.render_gbuffer(frame_inputs(3, cam, lights, 63, 47))
    assert not np.array_equal(o2.output(11), o.output(11))
    assert rec is not None  # (the patched records stay alive up to here)


# ------------------------------------------------------------------ the stand-alone query
def test_trace_on_the_shared_scene_matches_oracle():
    """hk_trace (k_trace) against the oracle's query on cornell: closest-hit and any-hit early distances, excluded
    instances, direction components of 0.0 and -0.0 (reciprocals of +-inf), and a max_distance just short of and just
    past each ray's hit."""
    st = _settings()
    scene, cam, lights, r, o = pair("cornell", 16, 16, st)
    assert r.scene_shared_transform() is True
    rng = np.random.default_rng(11)
    n = 20000
    org = rng.uniform([-1.2, -0.2, -1.2], [1.2, 2.2, 1.2], (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:100, 0] = 0.0
    d[100:200, 1] = -0.0
    d[200:300, 2] = 0.0
    d[300:400, (0, 2)] = -0.0
    rays = np.concatenate([org, d], axis=1).astype(np.float32)
    assert np.signbit(rays[100:200, 4]).all() and (rays[100:200, 4] == 0).all()
    early = np.where(rng.random(n) < 0.5, 0.0, 65535.0).astype(np.float32)
    excl = rng.integers(0, len(scene.instances) + 1, n).astype(np.uint32)
    a, b = r.trace(rays, None, early, excl), o.trace(rays, None, early, excl)
    assert (a == b).all(), f"{int((a != b).any(axis=1).sum())} of {n} rays differ"
    assert (a[:, 3] != 0xFFFFFFFF).mean() > 0.5
    # closest hits, then the same rays limited to one ulp short of and one ulp past the hit distance
    none = np.full(n, 0xFFFFFFFF, np.uint32)
    zero = np.zeros(n, np.float32)
    full = o.trace(rays, None, zero, none)
    assert (r.trace(rays, None, zero, none) == full).all()
    hit = full[:, 3] != 0xFFFFFFFF
    assert hit.mean() > 0.5
    t = np.where(hit, full[:, 2].copy().view(np.float32), np.float32(1.0))
    for limit in (np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf))):
        limit = np.where(hit, limit, np.float32(65535.0)).astype(np.float32)
        a, b = r.trace(rays, limit, zero, none), o.trace(rays, limit, zero, none)
        assert (a == b).all(), f"{int((a != b).any(axis=1).sum())} of {n} rays differ"
    # the general walk answers the same
    r.set_option("shared_xform", 0)
    assert (r.trace(rays, None, early, excl) == o.trace(rays, None, early, excl)).all()
