"""`HikariPlugin` host mirror: one `HikariRenderer` per camera, driving libhikari_amd.so.

The reference's per-frame render-graph work for a `hikari` camera is
    PrepassNode::run (raster G-buffer)                 -> render_gbuffer()  (primary rays, f1)
    LightNode::run (light.rs:590-702)                  -> render_frame()
    PostProcessNode::run denoise block (post_process.rs:1190-1224) -> denoise()
    tone_mapping dispatch (post_process.rs:1226-1234)  -> tone_sum()
`HikariPlugin.frame()` runs them in that order, like the `hikari` sub-graph (lib.rs:238-367).  After the renderer's
post_process(), `present()` is the `Overlay` phase item's draw into the view target (overlay.rs, overlay.wgsl).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _abi
from .cost import TreeCost
from .scene import Mesh, Scene, load_noise, texture_array
from .settings import HikariSettings, HikariUniversalSettings, PresentFormat

RESERVOIR_DTYPE = np.dtype([("radiance", "<u4", 2), ("random", "<u4", 2), ("visible_position", "<f4", 4),
                            ("sample_position", "<f4", 4), ("visible_normal", "<u4"), ("sample_normal", "<u4"),
                            ("reservoir", "<u4", 2)])
assert RESERVOIR_DTYPE.itemsize == 64


def _stream(stream):
    """A hipStream_t handle for the C ABI: None (the context's own stream), an integer address (e.g.
    torch.cuda.Stream.cuda_stream) or a ctypes.c_void_p; anything else is refused here, before it
    reaches HIP."""
    if stream is None or isinstance(stream, (int, C.c_void_p)):
        return stream
    raise TypeError(f"stream must be None or an integer hipStream_t handle, not {type(stream).__name__}")


def _check(ctx, rc: int, what: str) -> None:
    if rc != 0:
        msg = _abi.lib().hk_last_error(ctx).decode() if ctx else ""
        raise _abi.HikariError(f"{what} failed ({rc}): {msg}")


PLAN_LIGHT, PLAN_GBUFFER = 0, 1


def scene_stage_bytes(scene, plan: int):
    """(bytes, limit) of hk_scene_stage_bytes: what the traversal kernels of `plan` (PLAN_LIGHT, PLAN_GBUFFER)
    stage into LDS for this scene (a Scene or its hk_scene_desc), and the size up to which they stage at all.
    Host arithmetic only: needs no device."""
    desc = scene if isinstance(scene, _abi.hk_scene_desc) else (scene.desc if scene.desc is not None else scene.build())
    b, lim = C.c_uint32(), C.c_uint32()
    _check(None, _abi.lib().hk_scene_stage_bytes(C.byref(desc), int(plan), C.byref(b), C.byref(lim)),
           "hk_scene_stage_bytes")
    return b.value, lim.value


def scene_indirect_lds(scene):
    """(stash, total, limit) of hk_scene_indirect_lds: the indirect pass's stash bytes per workgroup, stash plus the
    scene's staged bytes (none past the staging limit), and what one workgroup may allocate.  Host arithmetic only."""
    desc = scene if isinstance(scene, _abi.hk_scene_desc) else (scene.desc if scene.desc is not None else scene.build())
    s, t, lim = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(None, _abi.lib().hk_scene_indirect_lds(C.byref(desc), C.byref(s), C.byref(t), C.byref(lim)),
           "hk_scene_indirect_lds")
    return s.value, t.value, lim.value


def scene_gbuffer_stack(scene):
    """(need, lds_levels) of hk_scene_gbuffer_stack: the G-buffer walk's stack bound for this scene as
    hk_scene_upload computes it, and the levels the shallow walk keeps in LDS."""
    desc = scene if isinstance(scene, _abi.hk_scene_desc) else (scene.desc if scene.desc is not None else scene.build())
    n, lv = C.c_uint32(), C.c_uint32()
    _check(None, _abi.lib().hk_scene_gbuffer_stack(C.byref(desc), C.byref(n), C.byref(lv)), "hk_scene_gbuffer_stack")
    return n.value, lv.value


def shared_transform(models) -> bool:
    """hks_shared_transform: True when there is at least one matrix and all the column-major 4x4 float32 matrices
    of `models` (n x 16) hold the same bits (-0.0 differs from 0.0).  Host only: needs no device."""
    m = np.ascontiguousarray(models, np.float32).reshape(-1, 16)
    return bool(_abi.lib().hks_shared_transform(m.ctypes.data if len(m) else None, len(m)))


def instance_descs(scene: Scene, previous=None):
    """ctypes array of hk_instance_desc for the instance list of `scene`: each instance's mesh slice
    (Scene.mesh_index), its material and its index in the set before (`previous`: one entry per instance, None or
    HK_INSTANCE_NEW for a new entity; previous=None: every entity is new)."""
    n = len(scene.instances)
    if previous is not None and len(previous) != n:
        raise ValueError("previous needs one entry per instance")
    out = (_abi.hk_instance_desc * max(1, n))()
    slices = {}
    for k, (mesh, mat, _) in enumerate(scene.instances):
        if mesh not in slices:
            v, pr, n0, nc = scene.mesh_index(mesh)
            slices[mesh] = _abi.hk_mesh_index(v, pr, (C.c_uint32 * 2)(n0, nc))
        p = None if previous is None else previous[k]
        out[k] = _abi.hk_instance_desc(slices[mesh], int(mat), _abi.HK_INSTANCE_NEW if p is None else int(p))
    return out


def material_records(scene: Scene):
    """The scene's GpuStandardMaterial records as one ctypes buffer (hk_material x len(scene.materials))."""
    return C.create_string_buffer(b"".join(m.record() for m in scene.materials), 80 * max(1, len(scene.materials)))


def instance_set_counts(uploaded, scene: Scene, materials: bool = False):
    """The nine element counts (hk_scene_desc order) hk_instance_set_counts gives for the instance list of `scene`
    set on the host-built `uploaded` scene (a Scene or its hk_scene_desc); materials=True: with the scene's material
    records instead of the uploaded ones.  Host arithmetic only: needs no device."""
    desc = uploaded if isinstance(uploaded, _abi.hk_scene_desc) else (
        uploaded.desc if uploaded.desc is not None else uploaded.build())
    out = (C.c_uint32 * 9)()
    mats = material_records(scene) if materials else None
    _check(None, _abi.lib().hk_instance_set_counts(C.byref(desc), instance_descs(scene), len(scene.instances), mats, out),
           "hk_instance_set_counts")
    return list(out)


def _mesh_descs(meshes):
    """(ctypes array of hk_mesh_desc, the numpy arrays it points into) for a list of Mesh objects, as Scene.build hands
    them to hks_add_mesh.  A mesh without an attribute gets a NULL there (hk_add_meshes refuses it)."""
    out = (_abi.hk_mesh_desc * max(1, len(meshes)))()
    keep = []
    for d, m in zip(out, meshes):
        p, n, u = (None if a is None else np.ascontiguousarray(a, np.float32) for a in (m.positions, m.normals, m.uvs))
        ix = None if m.indices is None else np.ascontiguousarray(m.indices, np.uint32).reshape(-1)
        keep += [p, n, u, ix]
        d.positions, d.normals, d.uvs = (None if a is None else a.ctypes.data for a in (p, n, u))
        d.vertex_count = 0 if p is None else len(p.reshape(-1, 3))
        d.indices = None if ix is None else ix.ctypes.data
        d.index_count = 0 if ix is None else len(ix)
        d.topology = int(m.topology)
    return out, keep


def add_meshes_counts(before, meshes):
    """(slices, counts after) of hk_add_meshes_counts: the (vertex, primitive, node0, node_count) slices `meshes` (Mesh
    objects) take when appended to arrays of the nine element counts `before`, and the nine counts after.  Host
    arithmetic only: needs no device."""
    L = _abi.lib()
    descs, keep = _mesh_descs(meshes)
    slices = (_abi.hk_mesh_index * max(1, len(meshes)))()
    after = (C.c_uint32 * 9)()
    rc = L.hk_add_meshes_counts((C.c_uint32 * 9)(*before), descs, len(meshes), slices, after)
    if rc != 0:
        raise _abi.HikariError(f"hk_add_meshes_counts failed ({rc}): {L.hk_add_meshes_counts_error().decode()}")
    return [(s.vertex, s.primitive, s.node[0], s.node[1]) for s in slices[:len(meshes)]], list(after)


def _mesh_entries(entries):
    """(ctypes array of hk_mesh_entry, what it points into) for the list of set_meshes: an item is a Mesh (a new mesh),
    or ((vertex, primitive, node0, node_count), vertex_count): a slice of the current arrays, kept."""
    new = [e for e in entries if isinstance(e, Mesh)]
    descs, keep = _mesh_descs(new)
    out = (_abi.hk_mesh_entry * max(1, len(entries)))()
    k = 0
    for d, e in zip(out, entries):
        if isinstance(e, Mesh):
            d.source = C.pointer(descs[k])
            k += 1
        else:
            (v, pr, n0, nc), count = e
            d.keep = _abi.hk_mesh_index(int(v), int(pr), (C.c_uint32 * 2)(int(n0), int(nc)))
            d.vertex_count = int(count)
    return out, (descs, keep)


def set_meshes_counts(before, entries):
    """(slices, counts after) of hk_set_meshes_counts: the (vertex, primitive, node0, node_count) slice of every entry
    of `entries` (HikariRenderer.set_meshes) in the new layout, and the nine counts after ([3:] are `before`'s: they
    follow the instance set).  Host arithmetic only: needs no device."""
    L = _abi.lib()
    arr, keep = _mesh_entries(entries)
    slices = (_abi.hk_mesh_index * max(1, len(entries)))()
    after = (C.c_uint32 * 9)()
    rc = L.hk_set_meshes_counts((C.c_uint32 * 9)(*before), arr, len(entries), slices, after)
    if rc != 0:
        raise _abi.HikariError(f"hk_set_meshes_counts failed ({rc}): {L.hk_set_meshes_counts_error().decode()}")
    return [(s.vertex, s.primitive, s.node[0], s.node[1]) for s in slices[:len(entries)]], list(after)


class HikariRenderer:
    """A camera's integrator context (hk_ctx)."""

    # options (hk_set_option) applied to every context this class creates; tests use it to force kernel
    # variants and schedules for all the contexts of a test (tests/conftest.py `hk_options`)
    defaults: dict = {}

    def __init__(self, device: int = 0, options: Optional[dict] = None):
        L = _abi.lib()
        h = C.c_void_p()
        rc = L.hk_create(device, C.byref(h))
        if rc != 0:
            raise _abi.HikariError(f"hk_create({device}) failed ({rc}): no usable gfx950 device")
        self._L = L
        self.ctx = h.value
        self.width = self.height = 0
        for k, v in {**self.defaults, **(options or {})}.items():
            self.set_option(k, v)

    def close(self):
        if getattr(self, "ctx", None):
            self._L.hk_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        self.close()

    # ---- runtime options (hk_set_option): schedule / kernel-variant choices, results unchanged
    def set_option(self, key: str, value: float) -> None:
        _check(self.ctx, self._L.hk_set_option(self.ctx, key.encode(), float(value)), f"hk_set_option({key})")

    def get_option(self, key: str) -> float:
        v = C.c_double()
        _check(self.ctx, self._L.hk_get_option(self.ctx, key.encode(), C.byref(v)), f"hk_get_option({key})")
        return v.value

    def options(self) -> dict:
        """{key: value} of every option of this context."""
        out, i = {}, 0
        while True:
            k = self._L.hk_option_name(i)
            if k is None:
                return out
            out[k.decode()] = self.get_option(k.decode())
            i += 1

    def set_options(self, opts: dict) -> dict:
        """Set several options; returns their previous values (for restoring)."""
        old = {k: self.get_option(k) for k in opts}
        for k, v in opts.items():
            self.set_option(k, v)
        return old

    # ---- resources
    def upload_scene(self, scene: Scene) -> None:
        desc = scene.desc if scene.desc is not None else scene.build()
        _check(self.ctx, self._L.hk_scene_upload(self.ctx, C.byref(desc)), "hk_scene_upload")
        tex = texture_array(scene.textures)
        _check(self.ctx, self._L.hk_texture_upload(self.ctx, tex, len(scene.textures)), "hk_texture_upload")

    def upload_textures(self, textures) -> None:
        """Replace the material textures alone (hk_texture_upload; an empty list: the NO_TEXTURE pipeline)."""
        textures = list(textures)
        tex = texture_array(textures)
        _check(self.ctx, self._L.hk_texture_upload(self.ctx, tex, len(textures)), "hk_texture_upload")

    def set_noise(self, noise: Optional[np.ndarray] = None) -> None:
        n = np.ascontiguousarray(load_noise() if noise is None else noise, np.uint8)
        _check(self.ctx, self._L.hk_set_noise(self.ctx, n.ctypes.data, 16, 64), "hk_set_noise")

    def resize(self, width: int, height: int, ratio: float = 1.0, band_y0: int = 0, band_rows: int = 0) -> None:
        _check(self.ctx, self._L.hk_resize(self.ctx, width, height, ratio, band_y0, band_rows), "hk_resize")
        self.width, self.height = width, height

    def resize_striped(self, width: int, height: int, rank: int, world: int) -> None:
        """Interleaved 8-row stripes rank, rank + world, ... of the frame (bands.stripes_of)."""
        _check(self.ctx, self._L.hk_resize_striped(self.ctx, width, height, rank, world), "hk_resize_striped")
        self.width, self.height = width, height

    def resize_tile(self, width: int, height: int, x0: int, cols: int, y0: int, rows: int) -> None:
        """A 2-D tile of the frame: columns [x0, x0 + cols) of rows [y0, y0 + rows) plus halo (hk_resize_tile)."""
        _check(self.ctx, self._L.hk_resize_tile(self.ctx, width, height, x0, cols, y0, rows), "hk_resize_tile")
        self.width, self.height = width, height

    def tile_info(self):
        v = [C.c_int32(), C.c_int32()]
        _check(self.ctx, self._L.hk_tile_info(self.ctx, C.byref(v[0]), C.byref(v[1])), "hk_tile_info")
        return v[0].value, v[1].value

    def copy_output_rect(self, output_id: int, row0: int, rows: int, col0: int, cols: int, dst_ptr: int,
                         dst_pitch: int = 0, to_host: bool = False, stream=None) -> None:
        _check(self.ctx, self._L.hk_copy_output_rect(self.ctx, output_id, row0, rows, col0, cols, dst_ptr, dst_pitch,
                                                     int(to_host), _stream(stream)), "hk_copy_output_rect")

    def set_band_halo(self, rows: int) -> None:
        _check(self.ctx, self._L.hk_set_band_halo(self.ctx, rows), "hk_set_band_halo")

    def copy_output_rows(self, output_id: int, row0: int, rows: int, dst_ptr: int, to_host: bool = False,
                         stream=None) -> None:
        _check(self.ctx, self._L.hk_copy_output_rows(self.ctx, output_id, row0, rows, dst_ptr, int(to_host), _stream(stream)),
               "hk_copy_output_rows")

    def band_info(self):
        v = [C.c_int32() for _ in range(4)]
        _check(self.ctx, self._L.hk_band_info(self.ctx, *[C.byref(x) for x in v]), "hk_band_info")
        return tuple(x.value for x in v)

    def band_window_grow(self, settings: _abi.hk_settings, commit: bool = False) -> np.ndarray:
        """(10, 4) int32: per reservoir buffer the (frame row, rows) above and below the band's core whose records
        the next hk_render_frame with `settings` needs from their owner bands (hk_band_window_grow); commit widens
        the band's windows without zero-filling (after the rows were loaded)."""
        ranges = np.zeros((_abi.RESERVOIR_BUFFERS, 4), np.int32)
        rc = self._L.hk_band_window_grow(self.ctx, C.byref(settings), ranges.ctypes.data, int(commit))
        _check(self.ctx, min(rc, 0), "hk_band_window_grow")
        return ranges

    def reservoir_rows_bytes(self, rows: int) -> int:
        return 4 * rows * self.width * 16

    def reservoir_rows(self, buffer_id: int, frame_row0: int, rows: int, data=None, store: bool = False,
                       stream=None):
        """Records of frame rows [frame_row0, frame_row0 + rows) of a reservoir buffer in the row-exchange layout
        (hk_reservoir_rows): store False copies them out (into `data`: a uint8 array, or a device address; a new
        array when None, returned), store True copies `data` in."""
        if data is None:
            data = np.empty(self.reservoir_rows_bytes(rows), np.uint8)
        if isinstance(data, np.ndarray):
            if not data.flags.c_contiguous or data.nbytes != self.reservoir_rows_bytes(rows):
                raise ValueError("reservoir row data must be a contiguous array of reservoir_rows_bytes(rows) bytes")
            ptr = data.ctypes.data
        else:
            ptr = int(data)
        _check(self.ctx, self._L.hk_reservoir_rows(self.ctx, buffer_id, frame_row0, rows, ptr, int(store),
                                                   _stream(stream)), "hk_reservoir_rows")
        return data

    # ---- per frame
    def render_gbuffer(self, inputs: _abi.hk_frame_inputs, stream=None) -> None:
        _check(self.ctx, self._L.hk_render_gbuffer(self.ctx, C.byref(inputs), _stream(stream)), "hk_render_gbuffer")

    def render_frame(self, settings: _abi.hk_settings, inputs: _abi.hk_frame_inputs, stream=None) -> None:
        _check(self.ctx, self._L.hk_render_frame(self.ctx, C.byref(settings), C.byref(inputs), _stream(stream)),
               "hk_render_frame")

    def denoise(self, settings: _abi.hk_settings, inputs: _abi.hk_frame_inputs, stream=None) -> None:
        _check(self.ctx, self._L.hk_denoise(self.ctx, C.byref(settings), C.byref(inputs), _stream(stream)), "hk_denoise")

    def tone_sum(self, settings: _abi.hk_settings, stream=None) -> None:
        _check(self.ctx, self._L.hk_tone_sum(self.ctx, C.byref(settings), _stream(stream)), "hk_tone_sum")

    def update_instances(self, models: np.ndarray, local_aabbs: np.ndarray, stream=None, refit: bool = False) -> None:
        """New transforms of every instance (hk_update_instances): (n, 16) column-major models and
        (n, 6) local AABBs (center, half extents); the GPU rebuilds instances, TLAS, emissives and
        the light BVH.  refit=True (hk_refit_instances): the TLAS and the light BVH keep their trees and get new
        boxes (include/hk_refit.h) instead of a rebuild: cheaper, and trees that cost more to walk the further the
        instances are from where the trees were built; call without refit to rebuild."""
        m = np.ascontiguousarray(models, np.float32).reshape(-1, 16)
        a = np.ascontiguousarray(local_aabbs, np.float32).reshape(-1, 6)
        if len(m) != len(a):
            raise ValueError("models and local_aabbs differ in length")
        name = "hk_refit_instances" if refit else "hk_update_instances"
        _check(self.ctx, getattr(self._L, name)(self.ctx, m.ctypes.data, a.ctypes.data, len(m), _stream(stream)), name)

    def update_meshes(self, scene: Scene, mesh_ids, models=None, local_aabbs=None, stream=None,
                      refit=False) -> None:
        """Deformed meshes of an uploaded scene (hk_update_meshes): the positions and normals of `scene.meshes[i]` for
        each i in `mesh_ids` (same topology as uploaded) replace the uploaded ones on the GPU, which rebuilds those
        meshes' primitives and BLAS and then everything update_instances rebuilds.  models / local_aabbs: as for
        update_instances (default: the scene's instance_models() / instance_local_aabbs()).  refit=True
        (hk_refit_meshes): each listed BLAS keeps its tree and gets new boxes (include/hk_refit.h) instead of a rebuild:
        much cheaper, and a tree that walks more nodes the further the mesh is from the pose it was built for.
        refit="all" (hk_refit_meshes_all): the TLAS and the light BVH are refit as well, as by
        update_instances(refit=True)."""
        m = np.ascontiguousarray(scene.instance_models() if models is None else models, np.float32).reshape(-1, 16)
        a = np.ascontiguousarray(scene.instance_local_aabbs() if local_aabbs is None else local_aabbs,
                                 np.float32).reshape(-1, 6)
        if len(m) != len(a):
            raise ValueError("models and local_aabbs differ in length")
        ups = (_abi.hk_mesh_update * max(1, len(mesh_ids)))()
        keep = []
        for u, i in zip(ups, mesh_ids):
            mesh = scene.meshes[i]
            p = np.ascontiguousarray(mesh.positions, np.float32).reshape(-1, 3)
            n = None if mesh.normals is None else np.ascontiguousarray(mesh.normals, np.float32).reshape(-1, 3)
            if n is not None and len(n) != len(p):
                raise ValueError("positions and normals differ in length")
            keep += [p, n]
            v, pr, n0, nc = scene.mesh_index(i)
            u.mesh = _abi.hk_mesh_index(v, pr, (C.c_uint32 * 2)(n0, nc))
            u.vertex_count = len(p)
            u.positions = p.ctypes.data
            u.normals = None if n is None else n.ctypes.data
        name = "hk_refit_meshes_all" if refit == "all" else "hk_refit_meshes" if refit else "hk_update_meshes"
        _check(self.ctx, getattr(self._L, name)(self.ctx, ups, len(mesh_ids), m.ctypes.data, a.ctypes.data, len(m),
                                                _stream(stream)), name)

    def set_mesh_skins(self, scene: Scene, mesh_ids, keep_normals=(), stream=None) -> None:
        """Register the skins of `scene.meshes[i]` for each i in `mesh_ids` (hk_set_mesh_skins): the mesh's positions and
        normals as the bind pose and its `skin` (joint indices, weights, joint count) are copied to the device, where
        skin_meshes reads them.  The call replaces the whole set (an empty list drops it).  keep_normals: mesh ids
        registered without normals, whose uploaded normals a pose leaves alone."""
        arr = (_abi.hk_mesh_skin * max(1, len(mesh_ids)))()
        keep = []
        for s, i in zip(arr, mesh_ids):
            mesh = scene.meshes[i]
            if mesh.skin is None:
                raise ValueError(f"mesh {i} has no skin")
            p = np.ascontiguousarray(mesh.positions, np.float32).reshape(-1, 3)
            n = None if mesh.normals is None or i in keep_normals else \
                np.ascontiguousarray(mesh.normals, np.float32).reshape(-1, 3)
            ix = np.ascontiguousarray(mesh.skin.joint_indices, np.uint16).reshape(-1, 4)
            w = np.ascontiguousarray(mesh.skin.joint_weights, np.float32).reshape(-1, 4)
            if not (len(ix) == len(w) == len(p)) or (n is not None and len(n) != len(p)):
                raise ValueError("positions, normals, joint_indices and joint_weights differ in length")
            keep += [p, n, ix, w]
            v, pr, n0, nc = scene.mesh_index(i)
            s.mesh = _abi.hk_mesh_index(v, pr, (C.c_uint32 * 2)(n0, nc))
            s.vertex_count = len(p)
            s.positions = p.ctypes.data
            s.normals = None if n is None else n.ctypes.data
            s.joint_indices = ix.ctypes.data
            s.joint_weights = w.ctypes.data
            s.joint_count = int(mesh.skin.joint_count)
        _check(self.ctx, self._L.hk_set_mesh_skins(self.ctx, arr, len(mesh_ids), _stream(stream)), "hk_set_mesh_skins")

    def skin_meshes(self, scene: Scene, poses: dict, models=None, local_aabbs=None, stream=None,
                    refit=False) -> None:
        """Pose skinned meshes on the GPU (hk_skin_meshes): poses = {mesh id: (joint_count, 16) column-major joint
        matrices} for meshes registered by set_mesh_skins; the GPU skins their vertices, rebuilds their primitives and
        BLAS and then everything update_instances rebuilds, with the posed meshes' boxes derived on the device.
        `scene` gives the slices (scene.mesh_index) and, by default, models and local_aabbs (instance_models() /
        instance_local_aabbs(); the rows of a posed mesh's instances are ignored).  refit=True (hk_skin_meshes_refit):
        the posed meshes' BLAS are refit, not rebuilt, as in update_meshes; refit="all" (hk_skin_meshes_refit_all): the
        TLAS and the light BVH too."""
        m = np.ascontiguousarray(scene.instance_models() if models is None else models, np.float32).reshape(-1, 16)
        a = np.ascontiguousarray(scene.instance_local_aabbs() if local_aabbs is None else local_aabbs,
                                 np.float32).reshape(-1, 6)
        if len(m) != len(a):
            raise ValueError("models and local_aabbs differ in length")
        arr = (_abi.hk_skin_pose * max(1, len(poses)))()
        keep = []
        for p, (i, joints) in zip(arr, poses.items()):
            j = np.ascontiguousarray(joints, np.float32).reshape(-1, 16)
            keep.append(j)
            v, pr, n0, nc = scene.mesh_index(i)
            p.mesh = _abi.hk_mesh_index(v, pr, (C.c_uint32 * 2)(n0, nc))
            p.joints = j.ctypes.data
            p.joint_count = len(j)
        name = "hk_skin_meshes_refit_all" if refit == "all" else "hk_skin_meshes_refit" if refit else "hk_skin_meshes"
        _check(self.ctx, getattr(self._L, name)(self.ctx, arr, len(poses), m.ctypes.data, a.ctypes.data, len(m),
                                                _stream(stream)), name)

    def set_mesh_morphs(self, scene: Scene, mesh_ids, keep_normals=(), stream=None) -> None:
        """Register the morph targets of `scene.meshes[i]` for each i in `mesh_ids` (hk_set_mesh_morphs): the mesh's
        positions and normals as the base and its `morph` (target-major position and normal deltas) are copied to the
        device, where morph_meshes reads them.  The call replaces the whole set (an empty list drops it); the skin set
        is another.  keep_normals: mesh ids registered without normals (and without normal deltas), whose uploaded
        normals a pose leaves alone."""
        arr = (_abi.hk_mesh_morph * max(1, len(mesh_ids)))()
        keep = []
        for s, i in zip(arr, mesh_ids):
            mesh = scene.meshes[i]
            if mesh.morph is None:
                raise ValueError(f"mesh {i} has no morph")
            p = np.ascontiguousarray(mesh.positions, np.float32).reshape(-1, 3)
            n = None if mesh.normals is None or i in keep_normals else \
                np.ascontiguousarray(mesh.normals, np.float32).reshape(-1, 3)
            dp = np.ascontiguousarray(mesh.morph.position_deltas, np.float32).reshape(-1, len(p), 3)
            dn = None if mesh.morph.normal_deltas is None or n is None else \
                np.ascontiguousarray(mesh.morph.normal_deltas, np.float32).reshape(-1, len(p), 3)
            if (n is not None and len(n) != len(p)) or (dn is not None and dn.shape != dp.shape):
                raise ValueError("positions, normals, position_deltas and normal_deltas differ in length")
            keep += [p, n, dp, dn]
            v, pr, n0, nc = scene.mesh_index(i)
            s.mesh = _abi.hk_mesh_index(v, pr, (C.c_uint32 * 2)(n0, nc))
            s.vertex_count = len(p)
            s.positions = p.ctypes.data
            s.normals = None if n is None else n.ctypes.data
            s.target_count = len(dp)
            s.position_deltas = dp.ctypes.data
            s.normal_deltas = None if dn is None else dn.ctypes.data
        _check(self.ctx, self._L.hk_set_mesh_morphs(self.ctx, arr, len(mesh_ids), _stream(stream)), "hk_set_mesh_morphs")

    def morph_meshes(self, scene: Scene, poses: dict, models=None, local_aabbs=None, stream=None,
                     refit=False) -> None:
        """Morph meshes on the GPU (hk_morph_meshes): poses = {mesh id: weights} or {mesh id: (weights, joints)} for
        meshes registered by set_mesh_morphs (and, with joints, by set_mesh_skins); the GPU folds the targets whose
        weight is not zero over the resident base, skins the result where joints are given, rebuilds the meshes'
        primitives and BLAS and then everything update_instances rebuilds, with the posed meshes' boxes derived on the
        device.  `scene` gives the slices and, by default, models and local_aabbs, as for skin_meshes.  refit=True
        (hk_morph_meshes_refit): the posed meshes' BLAS are refit, not rebuilt; refit="all" (hk_morph_meshes_refit_all):
        the TLAS and the light BVH too."""
        m = np.ascontiguousarray(scene.instance_models() if models is None else models, np.float32).reshape(-1, 16)
        a = np.ascontiguousarray(scene.instance_local_aabbs() if local_aabbs is None else local_aabbs,
                                 np.float32).reshape(-1, 6)
        if len(m) != len(a):
            raise ValueError("models and local_aabbs differ in length")
        arr = (_abi.hk_morph_pose * max(1, len(poses)))()
        keep = []
        for p, (i, pose) in zip(arr, poses.items()):
            weights, joints = pose if isinstance(pose, tuple) else (pose, None)
            w = np.ascontiguousarray(weights, np.float32).reshape(-1)
            j = None if joints is None else np.ascontiguousarray(joints, np.float32).reshape(-1, 16)
            keep += [w, j]
            v, pr, n0, nc = scene.mesh_index(i)
            p.mesh = _abi.hk_mesh_index(v, pr, (C.c_uint32 * 2)(n0, nc))
            p.weights = w.ctypes.data
            p.target_count = len(w)
            p.joints = None if j is None else j.ctypes.data
            p.joint_count = 0 if j is None else len(j)
        name = "hk_morph_meshes_refit_all" if refit == "all" else "hk_morph_meshes_refit" if refit else "hk_morph_meshes"
        _check(self.ctx, getattr(self._L, name)(self.ctx, arr, len(poses), m.ctypes.data, a.ctypes.data, len(m),
                                                _stream(stream)), name)

    def set_instances(self, scene: Scene, previous=None, materials: bool = False, stream=None, models=None,
                      local_aabbs=None) -> None:
        """A new instance set for the uploaded scene (hk_set_instances): entities spawned, despawned, hidden or given
        another material.  `scene` has the uploaded scene's meshes and materials in the same order and any instance
        list; the GPU rebuilds instances, TLAS, emissives, alias tables and the light BVH for it.  previous: per
        instance its index in the set before this call (None for a new entity; previous=None: all new), for the motion
        vectors.  materials=True also sends the scene's material records.  models / local_aabbs: default
        the scene's instance_models() / instance_local_aabbs()."""
        m = np.ascontiguousarray(scene.instance_models() if models is None else models, np.float32).reshape(-1, 16)
        a = np.ascontiguousarray(scene.instance_local_aabbs() if local_aabbs is None else local_aabbs,
                                 np.float32).reshape(-1, 6)
        if len(m) != len(a) or len(m) != len(scene.instances):
            raise ValueError("models and local_aabbs need one record per instance")
        mats = material_records(scene) if materials else None
        _check(self.ctx, self._L.hk_set_instances(self.ctx, instance_descs(scene, previous), m.ctypes.data, a.ctypes.data,
                                                  len(m), mats, _stream(stream)), "hk_set_instances")

    def scene_counts(self) -> list:
        """The current element counts of the nine scene arrays, hk_scene_desc order (hk_scene_counts)."""
        out = (C.c_uint32 * 9)()
        _check(self.ctx, self._L.hk_scene_counts(self.ctx, out), "hk_scene_counts")
        return list(out)

    def add_meshes(self, meshes, stream=None) -> list:
        """Mesh assets that arrive after the upload (hk_add_meshes): the GPU appends the vertices and primitives of
        each hikari_amd.Mesh in `meshes` to the scene's arrays and builds its BLAS; the instance set and the picture
        stay.  Returns each mesh's slice (vertex, primitive, node0, node_count), which set_instances then spawns: a
        Scene whose mesh list is the uploaded one followed by these gives the same slices (Scene.mesh_index)."""
        descs, keep = _mesh_descs(meshes)
        slices = (_abi.hk_mesh_index * max(1, len(meshes)))()
        _check(self.ctx, self._L.hk_add_meshes(self.ctx, descs, len(meshes), slices, _stream(stream)), "hk_add_meshes")
        return [(s.vertex, s.primitive, s.node[0], s.node[1]) for s in slices[:len(meshes)]]

    def set_meshes(self, scene: Scene, entries, previous=None, materials: bool = False, models=None, local_aabbs=None,
                   stream=None) -> list:
        """A new mesh asset list and instance set (hk_set_meshes): meshes removed, replaced by ones of another
        topology, inserted or reordered, without a host rebuild.  entries: the new list, an item a hikari_amd.Mesh (a
        new mesh, built on the GPU) or ((vertex, primitive, node0, node_count), vertex_count) (a slice of the current
        arrays, kept and moved to its place).  `scene` is the host scene of the new list and set: scene.meshes[k] is
        the mesh entry k stands for, and its instances, models and local boxes are used as in set_instances (previous,
        materials, models, local_aabbs: as there).  Returns the slices of the new layout, which equal
        scene.mesh_index(k)."""
        m = np.ascontiguousarray(scene.instance_models() if models is None else models, np.float32).reshape(-1, 16)
        a = np.ascontiguousarray(scene.instance_local_aabbs() if local_aabbs is None else local_aabbs,
                                 np.float32).reshape(-1, 6)
        if len(m) != len(a) or len(m) != len(scene.instances):
            raise ValueError("models and local_aabbs need one record per instance")
        if len(entries) != len(scene.meshes):
            raise ValueError("entries needs one item per mesh of the scene")
        arr, keep = _mesh_entries(entries)
        slices = (_abi.hk_mesh_index * max(1, len(entries)))()
        mats = material_records(scene) if materials else None
        _check(self.ctx, self._L.hk_set_meshes(self.ctx, arr, len(entries), slices, instance_descs(scene, previous),
                                               m.ctypes.data, a.ctypes.data, len(m), mats, _stream(stream)),
               "hk_set_meshes")
        return [(s.vertex, s.primitive, s.node[0], s.node[1]) for s in slices[:len(entries)]]

    def scene_capacity(self) -> list:
        """The element capacities of the nine scene arrays, hk_scene_desc order (hk_scene_capacity): what each holds
        before set_instances or add_meshes has to allocate."""
        out = (C.c_uint32 * 9)()
        _check(self.ctx, self._L.hk_scene_capacity(self.ctx, out), "hk_scene_capacity")
        return list(out)

    def tree_costs(self, mesh_ids=(), stream=None) -> dict:
        """How expensive the resident trees are to walk (hk_tree_costs; the rule: include/hk_cost.h), computed on the
        GPU in one launch: {"tlas": TreeCost, "lights": TreeCost (zeros without emitters), "meshes": [TreeCost of the
        BLAS of each id in `mesh_ids`]}.  A mesh id indexes the context's known slices in the order they became known:
        after upload_scene the distinct meshes in the order the instances first carry them.  Reads the scene, changes
        nothing; what a caller that refits decides a rebuild with (hikari_amd.RefitPolicy)."""
        ids = np.ascontiguousarray(mesh_ids, np.uint32).reshape(-1)
        tlas, lights = _abi.hk_tree_cost(), _abi.hk_tree_cost()
        meshes = (_abi.hk_tree_cost * max(len(ids), 1))()
        _check(self.ctx, self._L.hk_tree_costs(self.ctx, ids.ctypes.data_as(C.POINTER(C.c_uint32)) if len(ids) else None,
                                               len(ids), tlas, lights, meshes, _stream(stream)), "hk_tree_costs")
        return {"tlas": TreeCost.from_c(tlas), "lights": TreeCost.from_c(lights),
                "meshes": [TreeCost.from_c(meshes[j]) for j in range(len(ids))]}

    def scene_shared_transform(self) -> bool:
        """Every instance of the current scene carries one bit-identical transform (hk_scene_shared_transform): the
        walks then compute one local ray per walk while option shared_xform is on."""
        out = C.c_int32()
        _check(self.ctx, self._L.hk_scene_shared_transform(self.ctx, C.byref(out)), "hk_scene_shared_transform")
        return bool(out.value)

    def tile_skip_info(self) -> dict:
        """The last frame's background tile skip (hk_tile_skip_info, option bg_tile_skip): workgroups skipped in the
        G-buffer, direct / emissive and indirect launches, and the current G-buffer's screen bound (x0, y0, x1, y1),
        None while there is none."""
        skipped, bound, bounded = (C.c_uint32 * 3)(), (C.c_int32 * 4)(), C.c_int32()
        _check(self.ctx, self._L.hk_tile_skip_info(self.ctx, skipped, bound, C.byref(bounded)), "hk_tile_skip_info")
        return {"gbuffer": skipped[0], "direct": skipped[1], "indirect": skipped[2],
                "bound": tuple(bound) if bounded.value else None}

    def tone_skip_info(self) -> dict:
        """The last tone_sum's launch (hk_tone_skip_info): the pixels of its window it left out because they already
        held the clear colour's texel, and the frame rectangle (x0, y0, x1, y1) it ran over, None when it launched
        nothing."""
        skipped, rect = C.c_uint64(), (C.c_int32 * 4)()
        _check(self.ctx, self._L.hk_tone_skip_info(self.ctx, C.byref(skipped), rect), "hk_tone_skip_info")
        return {"skipped": int(skipped.value), "rect": tuple(rect) if any(rect) else None}

    def scene_array(self, array: int, dtype, count: int) -> np.ndarray:
        """Device copy of group-2 scene array `array` (hk_scene_desc order) as `count` records."""
        out = np.empty(count, dtype)
        _check(self.ctx, self._L.hk_read_scene_array(self.ctx, array, out.ctypes.data, out.nbytes),
               "hk_read_scene_array")
        return out

    def post_process(self, settings: _abi.hk_settings, inputs: _abi.hk_frame_inputs, stream=None) -> None:
        """SMAA TU4x or FSR1 (settings.upscale) and TAA Jasmine after tone mapping (hk_post_process); FSR1 leaves the
        display-size frame in OUT_FSR_RCAS."""
        _check(self.ctx, self._L.hk_post_process(self.ctx, C.byref(settings), C.byref(inputs), _stream(stream)),
               "hk_post_process")

    def set_fsr1_sharpness(self, sharpness: float) -> None:
        """`Upscale::Fsr1 { sharpness }` for the following post_process calls (hk_set_fsr1_sharpness)."""
        _check(self.ctx, self._L.hk_set_fsr1_sharpness(self.ctx, float(sharpness)), "hk_set_fsr1_sharpness")

    def present(self, settings, width: int, height: int, format="rgba8_srgb", viewport=None, input: int = -1,
                dst_ptr: Optional[int] = None, pitch: int = 0, stream=None):
        """The overlay's draw (hk_present): the displayed plane (input -1: chosen from `settings` as overlay.rs:227-231
        does; else an RGBA16F output id) into `viewport` = (x, y, w, h) (None: all) of a width x height target of
        `format` (a PresentFormat, its number or its lower-case name).  dst_ptr None: the context's own present plane,
        returned as an (height, width, 4) array, uint8 for the 8-bit formats and uint16 (f16 bits) for RGBA16F;
        otherwise device memory of the caller's with row pitch `pitch` bytes (0: packed), and None is returned.
        `settings`: an hk_settings record, or None with an explicit input."""
        t = _abi.hk_present_target()
        t.data, t.width, t.height, t.pitch = dst_ptr, int(width), int(height), int(pitch)
        t.format = int(PresentFormat.of(format))
        t.vp_x, t.vp_y, t.vp_w, t.vp_h = (0, 0, 0, 0) if viewport is None else [int(v) for v in viewport]
        t.input = int(input)
        _check(self.ctx, self._L.hk_present(self.ctx, None if settings is None else C.byref(settings), C.byref(t),
                                            _stream(stream)), "hk_present")
        return self.get_present(stream) if dst_ptr is None else None

    def present_info(self):
        """(width, height, bytes per texel, PresentFormat) of the context's own present plane."""
        v = [C.c_uint32() for _ in range(4)]
        _check(self.ctx, self._L.hk_present_info(self.ctx, *[C.byref(x) for x in v]), "hk_present_info")
        return v[0].value, v[1].value, v[2].value, PresentFormat(v[3].value)

    def get_present(self, stream=None) -> np.ndarray:
        """The context's own present plane as (height, width, 4) uint8, or uint16 for RGBA16F (hk_get_present)."""
        w, h, b, _ = self.present_info()
        out = np.empty((h, w, 4), np.uint8 if b == 4 else np.uint16)
        _check(self.ctx, self._L.hk_get_present(self.ctx, out.ctypes.data, out.nbytes, 1, _stream(stream)),
               "hk_get_present")
        return out

    def accumulate(self, reset: bool = False, stream=None) -> None:
        """Add the tone-mapped output to the sub-frame accumulator (hk_accumulate)."""
        _check(self.ctx, self._L.hk_accumulate(self.ctx, int(reset), _stream(stream)), "hk_accumulate")

    def resolve_accumulation(self, stream=None) -> None:
        """Accumulator / sub-frame count -> OUT_ACCUMULATED (RGBA16F)."""
        _check(self.ctx, self._L.hk_resolve_accumulation(self.ctx, _stream(stream)), "hk_resolve_accumulation")

    # ---- readback
    def output_info(self, output_id: int):
        w, h, b = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self.ctx, self._L.hk_output_info(self.ctx, output_id, C.byref(w), C.byref(h), C.byref(b)),
               "hk_output_info")
        return w.value, h.value, b.value

    def output(self, output_id: int) -> np.ndarray:
        """Raw bytes of an output plane as (rows, width, bytes_per_pixel) uint8."""
        w, h, b = self.output_info(output_id)
        out = np.empty((h, w, b), np.uint8)
        _check(self.ctx, self._L.hk_get_output(self.ctx, output_id, out.ctypes.data, out.nbytes, 1, None),
               "hk_get_output")
        return out

    def output_device_ptr(self, output_id: int) -> int:
        """Device address of the plane for this frame (call sync(stream) before reading it there)."""
        return self._L.hk_output_device_ptr(self.ctx, output_id)

    def set_wavefront(self, enable: bool = True) -> None:
        """Indirect pass as a wavefront with material-sorted shading (hk_set_wavefront)."""
        _check(self.ctx, self._L.hk_set_wavefront(self.ctx, int(enable)), "hk_set_wavefront")

    def sync(self, stream=None) -> None:
        """`stream` waits for the context's own streams (hk_sync)."""
        _check(self.ctx, self._L.hk_sync(self.ctx, _stream(stream)), "hk_sync")

    def set_gbuffer_plane(self, plane: int, data: np.ndarray, stream=None) -> None:
        """A host G-buffer plane (hk_set_gbuffer_plane; 0..4 = position, normal, depth gradient,
        instance/material, velocity/uv), the route that keeps the reference's raster prepass."""
        d = np.ascontiguousarray(data)
        _check(self.ctx, self._L.hk_set_gbuffer_plane(self.ctx, plane, d.ctypes.data, d.nbytes, 0, _stream(stream)),
               "hk_set_gbuffer_plane")

    def reservoirs(self, buffer_id: int) -> np.ndarray:
        w, h, _ = self.output_info(_abi.OUT_VARIANCE[0])
        out = np.empty(w * h, RESERVOIR_DTYPE)
        _check(self.ctx, self._L.hk_dump_reservoirs(self.ctx, buffer_id, out.ctypes.data, w * h, None),
               "hk_dump_reservoirs")
        return out

    def load_reservoirs(self, buffer_id: int, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data, RESERVOIR_DTYPE)
        _check(self.ctx, self._L.hk_load_reservoirs(self.ctx, buffer_id, data.ctypes.data, len(data), None),
               "hk_load_reservoirs")

    def reset_counters(self) -> None:
        _check(self.ctx, self._L.hk_reset_counters(self.ctx, None), "hk_reset_counters")

    def counters(self) -> dict:
        c = _abi.hk_counters()
        _check(self.ctx, self._L.hk_read_counters(self.ctx, C.byref(c), None), "hk_read_counters")
        return {"traverse_top": c.traverse_top, "traverse_emitter": c.traverse_emitter, "primary": c.primary}

    def primary_reused(self) -> int:
        """Primary rays (included in counters()["primary"]) of frames whose G-buffer planes were reused
        rather than traced (option gbuffer_reuse)."""
        c = _abi.hk_counters()
        _check(self.ctx, self._L.hk_read_counters(self.ctx, C.byref(c), None), "hk_read_counters")
        return c.primary_reused

    def enable_kernel_timing(self, enable: bool = True) -> None:
        _check(self.ctx, self._L.hk_enable_kernel_timing(self.ctx, int(enable)), "hk_enable_kernel_timing")

    def set_kernel_timing_interval(self, every: int) -> None:
        """Time only frames whose frame_number % every == 0 (hk_set_kernel_timing_interval)."""
        _check(self.ctx, self._L.hk_set_kernel_timing_interval(self.ctx, int(every)), "hk_set_kernel_timing_interval")

    def lane_stats(self) -> dict:
        """{kernel: (active lanes, walk iterations)} of traverse_top (instrumented builds only)."""
        names = (C.c_char_p * 64)()
        act = (C.c_uint64 * 64)()
        its = (C.c_uint64 * 64)()
        n = self._L.hk_lane_stats(self.ctx, names, act, its, 64)
        return {names[i].decode(): (int(act[i]), int(its[i])) for i in range(min(n, 64))}

    def kernel_timing(self) -> dict:
        names = (C.c_char_p * 64)()
        ms = (C.c_float * 64)()
        n = self._L.hk_kernel_timing(self.ctx, names, ms, 64)
        return {names[i].decode(): float(ms[i]) for i in range(min(n, 64))}

    def trace(self, rays: np.ndarray, max_distance=None, early_distance=None, exclude=None) -> np.ndarray:
        """Stand-alone traverse_top over n rays (n, 6) -> (n, 5) uint32 {u, v, t bits, instance, primitive}."""
        rays = np.ascontiguousarray(rays, np.float32)
        n = len(rays)
        hits = np.empty((n, 5), np.uint32)
        keep = [None if a is None else np.ascontiguousarray(a, dt)
                for a, dt in ((max_distance, np.float32), (early_distance, np.float32), (exclude, np.uint32))]
        ptr = [None if a is None else a.ctypes.data for a in keep]
        _check(self.ctx, self._L.hk_trace(self.ctx, rays.ctypes.data, ptr[0], ptr[1], ptr[2], n, hits.ctypes.data, 0,
                                          None), "hk_trace")
        return hits

    def selftest_rcp(self, lo: int, hi: int) -> int:
        """f32 bit patterns in [lo, hi) (both signs) where the kernels' rcp_exact(x) != 1 / x."""
        n = C.c_uint64()
        _check(self.ctx, self._L.hk_selftest_rcp(self.ctx, lo, hi, C.byref(n)), "hk_selftest_rcp")
        return n.value

    def selftest_count(self, values: np.ndarray) -> int:
        """The kernels' ray-counter reduction (wave_count) over per-thread counts `values` (uint32): their total."""
        v = np.ascontiguousarray(values, np.uint32)
        n = C.c_uint64()
        _check(self.ctx, self._L.hk_selftest_count(self.ctx, v.ctypes.data, len(v), C.byref(n)), "hk_selftest_count")
        return n.value

    def selftest_div(self, divisor: float, lo: int, hi: int) -> int:
        """Mismatches of the kernels' division by a frame dimension against IEEE x / divisor."""
        n = C.c_uint64()
        _check(self.ctx, self._L.hk_selftest_div(self.ctx, divisor, lo, hi, C.byref(n)), "hk_selftest_div")
        return n.value

    def selftest_texture(self, texture: int, uv: np.ndarray) -> np.ndarray:
        """The kernels' own texture sampler on uploaded texture `texture` at (n, 2) uv -> (n, 4) float32."""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.empty((len(uv), 4), np.float32)
        _check(self.ctx, self._L.hk_selftest_texture(self.ctx, texture, uv.ctypes.data, len(uv), out.ctypes.data),
               "hk_selftest_texture")
        return out

    def selftest_math(self, fn, a: np.ndarray, b: np.ndarray = None):
        """The kernels' own scalar function `fn` (an hk_math_fn id or its name in _abi.MATH_FN) on the uint32 words
        `a` (and `b` for the two-operand ids): the result words, a pair (out0, out1) for sincos and unpack_f16."""
        from . import _abi
        name = fn if isinstance(fn, str) else _abi.MATH_FN_NAMES[fn]
        a = np.ascontiguousarray(a, np.uint32).ravel()
        if b is not None:
            b = np.ascontiguousarray(b, np.uint32).ravel()
            if len(b) != len(a):
                raise ValueError("a and b differ in length")
        out0 = np.empty(len(a), np.uint32)
        out1 = np.empty(len(a), np.uint32) if name in _abi.MATH_FN_TWO_RESULTS else None
        _check(self.ctx, self._L.hk_selftest_math(self.ctx, _abi.MATH_FN[name], a.ctypes.data,
                                                  None if b is None else b.ctypes.data, len(a), out0.ctypes.data,
                                                  None if out1 is None else out1.ctypes.data), "hk_selftest_math")
        return out0 if out1 is None else (out0, out1)

    def selftest_f16(self, values: np.ndarray) -> np.ndarray:
        """The kernels' own f32 -> f16 conversion applied to `values` (uint16 bit patterns)."""
        v = np.ascontiguousarray(values, np.float32)
        out = np.empty(len(v), np.uint16)
        _check(self.ctx, self._L.hk_selftest_f16(self.ctx, v.ctypes.data, len(v), out.ctypes.data), "hk_selftest_f16")
        return out


class HikariPlugin:
    """`app.add_plugin(HikariPlugin)` for one camera: owns the renderer and the frame counter
    (`FrameCounter`, view.rs:75-103; frame numbers 0, 1, 2, ...)."""

    def __init__(self, scene: Scene, settings: HikariSettings = None, device: int = 0,
                 universal: HikariUniversalSettings = None):
        self.settings = settings or HikariSettings()
        self.universal = universal or HikariUniversalSettings()
        self.renderer = HikariRenderer(device)
        self.renderer.set_noise()
        if self.universal.build_mesh_acceleration_structure and self.universal.build_instance_acceleration_structure:
            self.renderer.upload_scene(scene)
        self.frame_number = 0
        self._previous_camera = None

    def resize(self, width: int, height: int, band_y0: int = 0, band_rows: int = 0):
        self.renderer.resize(width, height, self.settings.upscale.ratio(), band_y0, band_rows)
        self.renderer.set_fsr1_sharpness(self.settings.upscale.sharpness())

    def frame(self, camera, lights, gbuffer: bool = True, stream=None) -> None:
        """One frame.  The previous frame's camera is the PreviousViewUniform of the motion vectors
        (view.rs:47-73; the first frame has none: static) and the prepass jitters the primary rays
        when TAA is on (prepass.rs:194-199)."""
        import copy

        from .scene import frame_inputs, jitter_mode
        r = self.renderer
        s = self.settings.to_c()
        fi = frame_inputs(self.frame_number, camera, lights, r.width, r.height,
                          previous_camera=self._previous_camera, jitter=jitter_mode(self.settings))
        self._previous_camera = copy.deepcopy(camera)
        if gbuffer:
            r.render_gbuffer(fi, stream)
        r.render_frame(s, fi, stream)
        if self.settings.denoise:
            r.denoise(s, fi, stream)
        r.tone_sum(s, stream)
        self.frame_number += 1

    def update_instances(self, models, local_aabbs, stream=None, refit: bool = False) -> None:
        """`prepare_instances` for moved instances (HikariRenderer.update_instances; refit=True keeps both trees)."""
        self.renderer.update_instances(models, local_aabbs, stream, refit=refit)

    def tree_costs(self, mesh_ids=(), stream=None) -> dict:
        """The resident trees' costs (HikariRenderer.tree_costs): what decides between a refit and a rebuild."""
        return self.renderer.tree_costs(mesh_ids, stream)

    def update_meshes(self, scene: Scene, mesh_ids, models=None, local_aabbs=None, stream=None,
                      refit=False) -> None:
        """`prepare_mesh_assets` for modified meshes of unchanged topology (HikariRenderer.update_meshes)."""
        self.renderer.update_meshes(scene, mesh_ids, models, local_aabbs, stream, refit=refit)

    def set_mesh_skins(self, scene: Scene, mesh_ids, keep_normals=(), stream=None) -> None:
        """HikariRenderer.set_mesh_skins: the `SkinnedMesh` entities' bind poses and rigs, resident on the device."""
        self.renderer.set_mesh_skins(scene, mesh_ids, keep_normals, stream)

    def skin_meshes(self, scene: Scene, poses: dict, models=None, local_aabbs=None, stream=None,
                    refit=False) -> None:
        """HikariRenderer.skin_meshes: this frame's joint palettes (`SkinnedMeshJoints` x inverse bind poses)."""
        self.renderer.skin_meshes(scene, poses, models, local_aabbs, stream, refit=refit)

    def set_mesh_morphs(self, scene: Scene, mesh_ids, keep_normals=(), stream=None) -> None:
        """HikariRenderer.set_mesh_morphs: the meshes' morph targets (glTF blend shapes), resident on the device."""
        self.renderer.set_mesh_morphs(scene, mesh_ids, keep_normals, stream)

    def morph_meshes(self, scene: Scene, poses: dict, models=None, local_aabbs=None, stream=None,
                     refit=False) -> None:
        """HikariRenderer.morph_meshes: this frame's target weights (`MorphWeights`), and joint palettes under a skin."""
        self.renderer.morph_meshes(scene, poses, models, local_aabbs, stream, refit=refit)

    def add_meshes(self, meshes, stream=None) -> list:
        """HikariRenderer.add_meshes: mesh assets created after the scene was uploaded (AssetEvent::Created)."""
        return self.renderer.add_meshes(meshes, stream=stream)

    def set_meshes(self, scene: Scene, entries, previous=None, materials: bool = False, models=None, local_aabbs=None,
                   stream=None) -> list:
        """HikariRenderer.set_meshes: mesh assets removed, replaced or reordered (AssetEvent::Removed / Modified with
        another topology, the BTreeMap's order) together with the instance set."""
        return self.renderer.set_meshes(scene, entries, previous, materials, models, local_aabbs, stream)

    def set_instances(self, scene: Scene, previous=None, materials: bool = False, stream=None) -> None:
        """`prepare_instances` for spawned, despawned, hidden or re-materialed entities (HikariRenderer.set_instances)."""
        self.renderer.set_instances(scene, previous, materials, stream)

    def present(self, width: int = None, height: int = None, hdr: bool = False, viewport=None, stream=None):
        """The `Overlay` draw into a window-sized view target (overlay.rs:333-395): the plane the settings display,
        into `viewport` (camera.viewport; None: the whole target) of a target of width x height (default: the
        physical size, as a window's) — Rgba8UnormSrgb, or Rgba16Float when the view is `hdr`.  Returns the target as
        an (height, width, 4) array (HikariRenderer.present)."""
        r = self.renderer
        return r.present(self.settings.to_c(), r.width if width is None else width, r.height if height is None else height,
                         PresentFormat.RGBA16F if hdr else PresentFormat.RGBA8_SRGB, viewport, stream=stream)
