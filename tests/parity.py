"""The parity tests' one harness: canonical forms (bit-exact comparison with NaN payloads canonicalised), renderer +
oracle pairs, the pass sequence, the frame comparison and the frame loop, decomposed (band / tile / stripe) contexts,
and the instance-update checks.  Importable with numpy alone: hikari_amd and oracle are imported inside functions."""
from __future__ import annotations

import ctypes

import numpy as np

F16_IDS = {0, 4, 5, 6, 7, 8, 9, 10, 17, 18, 19}   # RGBA16F planes (17..19: accumulated, upscaled, TAA)
F32_IDS = {1, 2, 3, 11, 13, 14, 15, 16}  # f32 planes

# Reprojection scatters rejected history into the previous *spatial* reservoir buffers at the reprojected pixel
# (light.wgsl:1092-1095): several pixels can hit one target, so under motion these four buffers depend on the write
# order.  A caller that lists them as `racy` asks for at least RACY_MIN_EXACT of their records bit-exact.
RACY = (4, 5, 8, 9)
RACY_MIN_EXACT = 0.97

NODE_DT = np.dtype([("min", "<f4", 3), ("entry", "<u4"), ("max", "<f4", 3), ("exit", "<u4")])
SCENE_ARRAYS = ("vertices", "primitives", "asset_nodes", "alias_table", "instances", "instance_nodes", "materials",
                "emissive_nodes", "emissives")  # hk_scene_desc order


def canon_f16(u16: np.ndarray) -> np.ndarray:
    u = u16.astype(np.uint16).copy()
    nan = ((u & 0x7C00) == 0x7C00) & ((u & 0x03FF) != 0)
    u[nan] = 0x7E00
    return u


def canon_f32(u32: np.ndarray) -> np.ndarray:
    u = u32.astype(np.uint32).copy()
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    u[nan] = 0x7FC00000
    return u


def canon_plane(output_id: int, raw: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(raw)
    if output_id in F16_IDS:
        return canon_f16(b.view(np.uint16))
    if output_id in F32_IDS:
        return canon_f32(b.view(np.uint32))
    return b


def canon_reservoirs(r: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(r).view(np.uint32).reshape(-1, 16).copy()
    f16_words = [0, 1, 14, 15]  # radiance, reservoir (random is unorm16: compared raw)
    halves = canon_f16(np.ascontiguousarray(u[:, f16_words]).view(np.uint16))
    u[:, f16_words] = halves.view(np.uint32).reshape(len(u), len(f16_words))
    u[:, 4:12] = canon_f32(u[:, 4:12])
    return u


def canon_frame(src):
    """(planes 0..16, reservoir buffers 0..9) of `src` in canonical form: a stored frame for compare_frame."""
    return ([canon_plane(oid, src.output(oid)) for oid in range(17)],
            [canon_reservoirs(src.reservoirs(rid)) for rid in range(10)])


def mismatch_report(a: np.ndarray, b: np.ndarray, label: str) -> str:
    if a.shape != b.shape:
        return f"{label}: shape {a.shape} != {b.shape}"
    diff = a != b
    n = int(diff.sum())
    if n == 0:
        return ""
    where = np.argwhere(diff)[:5]
    return f"{label}: {n}/{a.size} words differ, first at {where.tolist()}"


# ------------------------------------------------------------------ contexts
def renderer(scene, size=None, ratio=1.0, options=None, wavefront=False):
    """A HikariRenderer with the noise and the scene, resized to `size` = (w, h) (None: left to the caller)."""
    from hikari_amd import HikariRenderer
    r = HikariRenderer(0, options=options)
    r.set_noise()
    r.upload_scene(scene)
    if size is not None:
        r.resize(*size, ratio)
    if wavefront:
        r.set_wavefront(True)
    return r


def pair(scene, w, h, settings, *, threads=None, options=None, wavefront=False):
    """(scene, camera, lights, renderer, oracle) at w x h and the settings' upscale ratio.  `scene`: an
    examples.SCENES name or a (scene, camera, lights) triple; threads=None: the oracle's own default."""
    from hikari_amd import examples, load_noise
    from oracle import Oracle
    scene, cam, lights = examples.SCENES[scene]() if isinstance(scene, str) else scene
    desc = scene.desc if scene.desc is not None else scene.build()
    ratio = settings.upscale.ratio()
    r = renderer(scene, (w, h), ratio, options, wavefront)
    o = Oracle(desc, load_noise(), w, h, ratio, textures=scene.textures,
               **({} if threads is None else {"threads": threads}))
    return scene, cam, lights, r, o


def decomposed(scene, world, W, H, kind, halo=0, bounds=None):
    """One context per part of a W x H frame, as the ranks of a multi-GPU run hold them: [(rect, renderer)] for
    `kind` "bands" (row bands of bands.band_of, `bounds`: uneven band edges), "tiles" (bands.tile_of) or "stripes"
    (interleaved 8-row stripes; rect is the rank), the first two with `halo` rows and columns around them."""
    from hikari_amd.bands import band_of, tile_of
    out = []
    for k in range(world):
        r = renderer(scene)
        if kind == "stripes":
            rect = k
            r.resize_striped(W, H, k, world)
        elif kind == "tiles":
            rect = tile_of(k, world, W, H)
            r.set_band_halo(halo)
            r.resize_tile(W, H, rect.x0, rect.cols, rect.y0, rect.rows)
        else:
            rect = band_of(k, world, H, bounds)
            r.set_band_halo(halo)
            r.resize(W, H, 1.0, rect.y0, rect.rows)
        out.append((rect, r))
    return out


def orbit_camera(cam, f, radius_step=0.05, angle_step=0.04):
    """The camera moved along an orbit around the Cornell box's centre: frame f's camera."""
    from hikari_amd import Camera, Transform
    t = cam.transform.translation
    a = angle_step * f
    c, s = np.cos(a), np.sin(a)
    eye = (float(c * t[0] + s * t[2]), float(t[1] + 0.02 * f), float(-s * t[0] + c * t[2]) + radius_step * f)
    return Camera(Transform.from_xyz(*eye).looking_at((0.0, 1.0, 0.0)))


def hip_runtime():
    """ctypes handle to the HIP runtime libhikari_amd.so itself uses (torch may bring a second copy into the
    process), for tests that act as a reader with a stream and device buffers of its own."""
    maps = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
    path = next((m for m in maps if m.startswith("/opt/rocm")), maps[0] if maps else "libamdhip64.so")
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpyAsync.argtypes = hip.hipMemcpy.argtypes + [ctypes.c_void_p]
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    return hip


# ------------------------------------------------------------------ frames
def passes(x, s, fi, post=False):
    """One frame on a renderer or an oracle: G-buffer, light passes, denoiser, tone-sum (and the post-process)."""
    x.render_gbuffer(fi)
    x.render_frame(s, fi)
    x.denoise(s, fi)
    x.tone_sum(s)
    if post:
        x.post_process(s, fi)


def compare_frame(r, ref, frame, errors, outputs=range(17), rids=range(10), racy=(), stats=None):
    """Append to `errors` one line per output plane in `outputs` and reservoir buffer in `rids` of `r` that is not
    bit-exact (canonical form) against `ref`: a live oracle (or a second renderer), or a stored canon_frame.
    Buffers listed in `racy` need RACY_MIN_EXACT of their records exact instead, their share appended to `stats` as
    (frame, rid, share)."""
    stored = isinstance(ref, tuple)
    for oid in outputs:
        want = ref[0][oid] if stored else canon_plane(oid, ref.output(oid))
        m = mismatch_report(canon_plane(oid, r.output(oid)), want, f"frame {frame} output {oid}")
        if m:
            errors.append(m)
    for rid in rids:
        # the reference allocates S.x*S.y records but indexes them with the s stride
        # (light.rs:344,352 vs light.wgsl:1061): compare the indexed prefix
        g = canon_reservoirs(r.reservoirs(rid))
        c = ref[1][rid][: len(g)] if stored else canon_reservoirs(ref.reservoirs(rid)[: len(g)])
        if rid in racy:
            exact = float((g == c).all(axis=1).mean())
            if stats is not None:
                stats.append((frame, rid, exact))
            if exact < RACY_MIN_EXACT:
                errors.append(f"frame {frame} reservoir {rid}: only {exact:.4f} of records exact")
        else:
            m = mismatch_report(g, c, f"frame {frame} reservoir {rid}")
            if m:
                errors.append(m)


def run_frames(r, ref, s, inputs, post=False, counters=True, label="", **compare):
    """The common loop: frame f = 0, 1, ... with inputs[f] on `r` and on `ref` (a live oracle, or the stored
    (frames, counters) of scene_ladder.reference), compare_frame(**compare) after each, stopping at the first
    frame that differs; then no errors and, unless counters=False, equal ray counters."""
    stored = isinstance(ref, tuple)
    errors = []
    for f, fi in enumerate(inputs):
        for x in (r,) if stored else (r, ref):
            passes(x, s, fi, post)
        compare_frame(r, ref[0][f] if stored else ref, f, errors, **compare)
        if errors:
            break
    assert not errors, label + "\n".join(errors[:20])
    if counters:
        assert r.counters() == (ref[1] if stored else ref.counters())


def run_static(scene, w, h, settings, frames, *, threads=None, options=None, wavefront=False, **run):
    """pair() and run_frames() over frames 0..frames-1 under the scene's own static camera."""
    from hikari_amd import frame_inputs
    scene, cam, lights, r, o = pair(scene, w, h, settings, threads=threads, options=options, wavefront=wavefront)
    run_frames(r, o, settings.to_c(), (frame_inputs(f, cam, lights, w, h) for f in range(frames)), **run)


def summed_counters(ranks):
    """The ray counters of decomposed()'s contexts added up."""
    return {k: sum(r.counters()[k] for _, r in ranks) for k in ("traverse_top", "traverse_emitter", "primary")}


def plane_agreement(a, b):
    """(share of pixels bit-exact, mean relative difference of rgb) of two canonical RGBA16F planes (.., 4) u16;
    the difference is inf or NaN when a value is not finite."""
    exact = float((a == b).all(axis=-1).mean())
    fa = a.view(np.float16).astype(np.float32)[..., :3]
    fb = b.view(np.float16).astype(np.float32)[..., :3]
    return exact, float(np.abs(fa - fb).sum() / max(np.abs(fb).sum(), 1e-6))


def core_agreement(r, rect, whole):
    """plane_agreement of a band context's core rows of the tone-mapped plane with rows rect.y0.. of `whole`,
    the whole frame's canonical plane as (H, W, 4)."""
    row0, rows, core0, core_rows = r.band_info()
    a = canon_plane(10, r.output(10)[core0: core0 + core_rows]).reshape(core_rows, -1, 4)
    return plane_agreement(a, whole[rect.y0: rect.y0 + rect.rows])


# ------------------------------------------------------------------ instance updates
def moved(triple, seed):
    """The (scene, camera, lights) triple with every instance moved / rotated / scaled by a seeded transform."""
    scene, cam, lights = triple
    rng = np.random.default_rng(seed)
    for k, (mesh, mat, m) in enumerate(scene.instances):
        a = rng.uniform(-0.4, 0.4)
        c, s_ = np.cos(a), np.sin(a)
        rot = np.array([[c, 0, s_, 0], [0, 1, 0, 0], [-s_, 0, c, 0], [0, 0, 0, 1]])
        sc = np.diag([rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2), 1.0])
        t = np.eye(4)
        t[:3, 3] = rng.uniform(-0.2, 0.2, 3)
        scene.instances[k] = (mesh, mat, t @ rot @ sc @ m)
    return scene, cam, lights


def host_scene_array(desc, idx, dt):
    """Array `idx` (SCENE_ARRAYS order) of a host-built hk_scene_desc as records of dtype `dt`."""
    a = getattr(desc, SCENE_ARRAYS[idx])
    return np.frombuffer(ctypes.string_at(a.data, a.count * dt.itemsize) if a.count else b"", dt)


def assert_instance_update_matches_host(r, desc, skip_empty=False):
    """The device scene arrays hk_update_instances rebuilt on `r` (instance records, alias table, emissive records,
    light BVH, TLAS) equal those of `desc`, the host builder's scene for the same transforms.  skip_empty: an empty
    host array is not read back."""
    inst_dt = np.dtype((np.void, 176))
    for idx, dt in ((4, inst_dt), (3, np.dtype((np.void, 8))), (8, np.dtype((np.void, 64))), (7, NODE_DT)):
        h = host_scene_array(desc, idx, dt)
        if skip_empty and len(h) == 0:
            continue
        g = r.scene_array(idx, dt, len(h))
        assert h.tobytes() == g.tobytes(), f"array {idx} differs"
    # TLAS: identical except that the device copy carries the instance box in each leaf
    h = host_scene_array(desc, 5, NODE_DT)
    g = r.scene_array(5, NODE_DT, len(h))
    assert np.array_equal(h["entry"], g["entry"]) and np.array_equal(h["exit"], g["exit"]), "array 5: links differ"
    inner = h["entry"] < 0x80000000
    assert h[inner].tobytes() == g[inner].tobytes(), "array 5: inner nodes differ"
    inst = np.frombuffer(host_scene_array(desc, 4, inst_dt).tobytes(), np.float32).reshape(-1, 44)
    leaf_ids = h["entry"][~inner] - 0x80000000
    assert (np.array_equal(g["min"][~inner], inst[leaf_ids, 0:3])
            and np.array_equal(g["max"][~inner], inst[leaf_ids, 4:7])), "array 5: leaf boxes differ"


def assert_rebuild_bitwise(r, desc):
    """assert_instance_update_matches_host (empty host arrays not read back), and the device TLAS's leaf boxes byte for
    byte the host instance boxes, so that a zero of the other sign counts as a difference there too."""
    assert_instance_update_matches_host(r, desc, skip_empty=True)
    h = host_scene_array(desc, 5, NODE_DT)
    g = r.scene_array(5, NODE_DT, len(h))
    leaf = h["entry"] >= 0x80000000
    inst = np.frombuffer(host_scene_array(desc, 4, np.dtype((np.void, 176))).tobytes(), np.float32).reshape(-1, 44)
    ids = h["entry"][leaf] - 0x80000000
    assert (g["min"][leaf].tobytes() == inst[ids, 0:3].tobytes()
            and g["max"][leaf].tobytes() == inst[ids, 4:7].tobytes()), "array 5: leaf boxes differ"
