"""The scene-edit GPU tests' one harness (hk_update_instances, hk_update_meshes, hk_add_meshes, hk_set_meshes,
hk_set_instances, the skins, the two refits and hk_tree_costs): the record dtypes, the arrays a context has to hold after
an edit, frames across an edit against the one-thread oracle, G-buffer planes, seeded rays against a fresh context, a
caller's stream and raw calls of the C entry points.  It builds on parity.py and, like it, is importable with numpy
alone: hikari_amd and oracle are imported inside functions.  Pinned on the CPU by tests/test_scene_edits_harness.py."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

import mesh_cases as mc
from instance_set_cases import desc_counts
from parity import (NODE_DT, RACY, assert_rebuild_bitwise, canon_plane, compare_frame, hip_runtime, host_scene_array,
                    mismatch_report, passes, renderer)

DEPTH_SIZE = (64, 48)  # the frame of the stack-bound tests
VERTEX_DT, PRIM_DT = np.dtype((np.void, 32)), np.dtype((np.void, 48))
MATERIAL_DT, INST_DT = np.dtype((np.void, 80)), np.dtype((np.void, 176))
ELEM_DT = [VERTEX_DT, PRIM_DT, NODE_DT, np.dtype((np.void, 8)), INST_DT, NODE_DT, MATERIAL_DT, NODE_DT,
           np.dtype((np.void, 64))]  # parity.SCENE_ARRAYS order


# ------------------------------------------------------------------ expected arrays
# The leaf boxes of the device's asset nodes, restated: k_fill_blas_leaves takes vmin(a, vmin(b, c)) and
# vmax(a, vmax(b, c)) of the triangle's corners with the device's fminf / fmaxf, which order -0 below +0.
def device_min(p):
    m = p.min(axis=1)
    zero, neg = m == 0.0, (p.view(np.uint32) == 0x80000000).any(axis=1)
    m[zero & neg], m[zero & ~neg] = -0.0, 0.0
    return m


def device_max(p):
    m = p.max(axis=1)
    zero, pos = m == 0.0, (p.view(np.uint32) == 0).any(axis=1)
    m[zero & pos], m[zero & ~pos] = 0.0, -0.0
    return m


def expected_asset_nodes(desc, registered=()):
    """The host's asset nodes with the leaves of every instanced mesh and of every slice in `registered` (added or
    listed, instanced or not) carrying their triangle's box; the leaves of a pooled mesh nobody registered stay
    empty."""
    nodes = host_scene_array(desc, 2, NODE_DT).copy()
    corners = np.ascontiguousarray(
        np.frombuffer(host_scene_array(desc, 1, PRIM_DT).tobytes(), np.float32).reshape(-1, 3, 4)[:, :, :3])
    for _, prim, n0, nc in set(mc.mesh_slices(desc)) | set(registered):
        part = nodes[n0: n0 + nc]
        leaf = part["entry"] >= 0x80000000
        tri = corners[prim + (part["entry"][leaf] - 0x80000000)]
        part["min"][leaf], part["max"][leaf] = device_min(tri), device_max(tri)
    return nodes


def assert_mesh_arrays(r, desc, registered=(), longer=False):
    """Counts 0-2 the host's; arrays 0 and 1 byte for byte the host's; array 2: entry / exit everywhere, inner nodes
    whole, every leaf of an instanced or registered mesh the byte image of its triangle's box.  longer: arrays 0-2
    hold an appended mesh behind the host scene's, so their counts are larger and their heads are compared."""
    counts, want = r.scene_counts()[:3], desc_counts(desc)[:3]
    assert (all(g > w for g, w in zip(counts, want)) if longer else counts == want), \
        f"counts of arrays 0-2: {counts}, host {want}"
    for idx in (0, 1):
        h = host_scene_array(desc, idx, ELEM_DT[idx])
        assert h.tobytes() == r.scene_array(idx, ELEM_DT[idx], counts[idx])[:len(h)].tobytes(), f"array {idx} differs"
    want = expected_asset_nodes(desc, registered)
    got = r.scene_array(2, NODE_DT, counts[2])[:len(want)]
    assert np.array_equal(want["entry"], got["entry"]) and np.array_equal(want["exit"], got["exit"]), "array 2: links"
    inner = want["entry"] < 0x80000000
    assert want[inner].tobytes() == got[inner].tobytes(), "array 2: inner nodes differ"
    assert want.tobytes() == got.tobytes(), "array 2: leaf boxes differ"


def assert_mesh_rebuild_bitwise(r, desc, registered=(), longer=False):
    """assert_mesh_arrays, and parity.assert_rebuild_bitwise for what the instance rebuild derives (instances, alias
    table, emissives, light BVH, TLAS)."""
    assert_mesh_arrays(r, desc, registered, longer)
    assert_rebuild_bitwise(r, desc)


def assert_scene_is(r, desc, registered=(), meshes=True, materials=True):
    """All nine counts and arrays the host build's: 0-2 by assert_mesh_arrays, 3, 4, 7, 8 and the TLAS (entries, exits
    and inner nodes the host's, the instance boxes in its leaves) by parity.assert_rebuild_bitwise, the materials here.
    meshes=False leaves arrays 0-2 to their counts, materials=False the materials: for hk_set_instances, which writes
    neither (a despawned mesh's leaves keep their boxes, and the materials are the host's only where they were sent)."""
    got, want = r.scene_counts(), desc_counts(desc)
    assert got == want, f"counts of arrays {[i for i in range(9) if got[i] != want[i]]}: {got}, host {want}"
    if meshes:
        assert_mesh_arrays(r, desc, registered)
    assert_rebuild_bitwise(r, desc)
    if materials:
        h = host_scene_array(desc, 6, MATERIAL_DT)
        assert h.tobytes() == r.scene_array(6, MATERIAL_DT, len(h)).tobytes(), "array 6 differs"


def assert_slices_kept(r, scene, mesh_ids):
    """The vertex, primitive and node slices of the meshes `mesh_ids` are byte for byte those of `scene`, the built
    scene that was uploaded (its nodes with the device's leaf boxes)."""
    nodes = expected_asset_nodes(scene.desc)
    for i in mesh_ids:
        v, p, n0, nc = scene.mesh_index(i)
        nv, k = len(scene.meshes[i].positions), (nc + 2) // 3
        for idx, a, n in ((0, v, nv), (1, p, k), (2, n0, nc)):
            h = nodes if idx == 2 else host_scene_array(scene.desc, idx, ELEM_DT[idx])
            g = r.scene_array(idx, ELEM_DT[idx], len(h))
            assert h[a: a + n].tobytes() == g[a: a + n].tobytes(), (i, idx)


def device_arrays(r, which=range(9)) -> list:
    """The bytes of the device's arrays `which`, each at its count."""
    counts = r.scene_counts()
    return [r.scene_array(i, ELEM_DT[i], counts[i]).tobytes() if counts[i] else b"" for i in which]


# ------------------------------------------------------------------ frames across an edit
class EditFrames:
    """A renderer `r` on `scene` and a one-thread oracle `o` on its desc at `size`, under SMAA_TU_1_0 without spatial
    reuse of the indirect reservoirs (`s`); view = (camera, lights).  Inside the `with` block the test applies its edits
    to `r` and checks the arrays; set_scene() gives the oracle the host-built desc, frames() renders on both and
    compares.  Leaving the block without an error asserts equal ray counters, that more than `floor` of the last frame's
    pixels see the scene (None: not asked) and, with `finite`, that the tone-mapped plane 10 holds finite values only;
    both sides are closed either way."""

    def __init__(self, scene, view, size, floor=None, finite=False, options=None, wavefront=False):
        from hikari_amd import HikariSettings, Upscale, load_noise
        from oracle import Oracle
        (self.cam, self.lights), (self.w, self.h), self.floor, self.finite = view, size, floor, finite
        self.r = renderer(scene, size, options=options, wavefront=wavefront)
        self.o = Oracle(scene.desc, load_noise(), self.w, self.h, 1.0, threads=1, textures=scene.textures)
        self.s = HikariSettings(upscale=Upscale.SMAA_TU_1_0, indirect_spatial_reuse=False).to_c()
        self.f = 0  # the next frame's index

    def set_scene(self, desc):
        self.o.set_scene(desc)

    def inputs(self):
        """The next frame's hk_frame_inputs."""
        from hikari_amd import frame_inputs
        return frame_inputs(self.f, self.cam, self.lights, self.w, self.h)

    def compare(self, label=""):
        """The frame both sides have just rendered, bit for bit (parity.compare_frame, the racy scatter targets within
        their tolerance): no errors, `label` in front of at most ten lines of them; then the frame index moves on."""
        errors = []
        compare_frame(self.r, self.o, self.f, errors, racy=RACY)
        self.f += 1
        assert not errors, (label + "\n" if label else "") + "\n".join(errors[:10])

    def frames(self, n=2, label=""):
        """The next n frames on both sides, each compared."""
        for _ in range(n):
            fi = self.inputs()
            for x in (self.r, self.o):
                passes(x, self.s, fi)
            self.compare(label)

    def oracle_plane(self, oid, dtype=np.float32):
        """The oracle's output plane `oid` as (h, w, 4) values of `dtype`."""
        return canon_plane(oid, self.o.output(oid)).view(dtype).reshape(self.h, self.w, 4)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                assert self.r.counters() == self.o.counters()
                if self.floor is not None:
                    assert (self.oracle_plane(11)[..., 3] > 0).mean() > self.floor  # the view covers the scene
                if self.finite:
                    assert np.isfinite(self.oracle_plane(10, np.float16).astype(np.float32)).all()
        finally:
            self.o.close()
            self.r.close()


# ------------------------------------------------------------------ G-buffer planes
MOTION_PLANES = (11, 12, 13, 14, 15)  # the G-buffer's planes and the velocity plane


def gbuffer_planes(x, fi, outputs=(11, 12, 13, 14)):
    """The canonical planes `outputs` of one G-buffer pass on a renderer or an oracle."""
    x.render_gbuffer(fi)
    return [canon_plane(oid, x.output(oid)) for oid in outputs]


def assert_planes(got, want, label):
    """Two lists of gbuffer_planes (plane 11 first) are equal, word for word."""
    for k, (a, b) in enumerate(zip(got, want)):
        m = mismatch_report(a, b, f"{label}: output {11 + k}")
        assert not m, m


# ------------------------------------------------------------------ rays
def seeded_rays(seed, n_instances, n=256, top=2.0):
    """(rays (n, 6) f32, early (n,) f32, excl (n,) u32) for hk_trace: origins in front of the scene, unit directions
    towards targets inside it (up to height `top`), half of them any-hit, each excluding one instance or none.  The
    draws from default_rng(seed) come in this order: origins, targets, early, excl."""
    rng = np.random.default_rng(seed)
    org = rng.uniform([-1.5, 0.0, 1.0], [1.5, 2.0, 4.0], (n, 3))
    d = rng.uniform([-1.5, 0.0, -0.5], [1.5, top, 0.2], (n, 3)) - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d], axis=1).astype(np.float32)
    early = np.where(rng.random(n) < 0.5, 0.0, 65535.0).astype(np.float32)
    excl = rng.integers(0, n_instances + 1, n).astype(np.uint32)
    return rays, early, excl


def assert_traces_equal_fresh(r, fresh, seed, n_instances, top=2.0):
    """seeded_rays(seed, n_instances, top=top) through hk_trace on the edited context `r` and on `fresh`, which
    uploaded the same scene: equal, and more than 0.3 of them hit.  Returns the hits."""
    rays, early, excl = seeded_rays(seed, n_instances, top=top)
    a, b = r.trace(rays, None, early, excl), fresh.trace(rays, None, early, excl)
    assert np.array_equal(a, b)
    assert (b[:, 3] < n_instances).mean() > 0.3  # many of them hit
    return b


def raw_renderer(desc, size=None):
    """A context that uploaded a desc as it is."""
    from hikari_amd import HikariRenderer
    r = HikariRenderer(0)
    r.set_noise()
    assert r._L.hk_scene_upload(r.ctx, ctypes.byref(desc)) == 0
    if size is not None:
        r.resize(*size, 1.0)
    return r


# ------------------------------------------------------------------ caller stream
@contextlib.contextmanager
def caller_stream():
    """(stream, sync): a stream of the caller's for edit calls, created in the HIP runtime the library loads
    (parity.hip_runtime: a stream of another runtime copy in the process is not a handle the library can take), and
    sync(), which asserts hipStreamSynchronize on it.  The edit calls wait for their stream once, so the arrays are
    complete when they return; a test calls sync() all the same, then asserts, and closes its renderer as the last
    thing inside the block: leaving the block destroys the stream, which has to outlive the context that used it.
    Nothing is synchronised on the way out, so that a test synchronises exactly where it says."""
    hip = hip_runtime()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0

    def sync():
        assert hip.hipStreamSynchronize(s) == 0

    try:
        yield s, sync
    finally:
        assert hip.hipStreamDestroy(s) == 0


# ------------------------------------------------------------------ raw calls
def raw_call(r, entry, *args):
    """C entry point `entry` called on r's context with hand-made arguments: (return code, last error text)."""
    rc = getattr(r._L, entry)(r.ctx, *args)
    return rc, r._L.hk_last_error(r.ctx).decode()


def models_and_aabbs(scene, local_aabbs=None):
    """The contiguous f32 `models` and `local_aabbs` arrays of a scene, as the edit calls take them (local_aabbs=None:
    mesh_cases.local_aabbs, the host builder's fold)."""
    return (np.ascontiguousarray(scene.instance_models(), np.float32),
            np.ascontiguousarray(mc.local_aabbs(scene) if local_aabbs is None else local_aabbs, np.float32))


def ptr(a, given=True):
    """The address of array `a` for a raw call; NULL for None or where it is not given."""
    return a.ctypes.data if given and a is not None else None
