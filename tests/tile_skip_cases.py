"""Scenes, cameras and helpers of the background tile skip's tests (option bg_tile_skip): the screen bound of a
scene's world box (hks_instance_bounds, hks_screen_bounds) on the host, and the skipped workgroups on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

GUARD = 4  # the runtime's guard band (TILE_SKIP_GUARD), in pixels


def world_box(scene) -> np.ndarray:
    """hks_instance_bounds of the scene's instances: (min xyz, max xyz) as 6 doubles."""
    from hikari_amd import _abi
    models = np.ascontiguousarray(scene.instance_models(), np.float32)
    boxes = np.ascontiguousarray(scene.instance_local_aabbs(), np.float32)
    out = (C.c_double * 6)()
    assert _abi.lib().hks_instance_bounds(models.ctypes.data, boxes.ctypes.data, len(models), out) == 1
    return np.array(out, np.float64)


def screen_bounds(box, view, w, h, guard=GUARD):
    """hks_screen_bounds: (x0, y0, x1, y1), or None without a rectangle."""
    from hikari_amd import _abi
    b = (C.c_double * 6)(*[float(v) for v in box])
    rect = (C.c_int32 * 4)()
    rc = _abi.lib().hks_screen_bounds(b, C.byref(view), w, h, guard, rect)
    return tuple(rect) if rc == 1 else None


def quad_scene(half_w=1.0, half_h=0.6, centre=(0.0, 1.0, 0.0)):
    """One emissive-free quad in the plane z = centre.z, facing +z, with a lamp-less material."""
    from hikari_amd import Mesh, Scene, StandardMaterial
    s = Scene()
    p = np.array([[-half_w, -half_h, 0], [half_w, -half_h, 0], [half_w, half_h, 0], [-half_w, half_h, 0]], np.float32)
    n = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    mesh = s.add_mesh(Mesh(p, n, uv, np.array([0, 1, 2, 0, 2, 3], np.uint32)))
    mat = s.add_material(StandardMaterial(base_color=(0.8, 0.7, 0.6, 1.0)))
    m = np.eye(4)
    m[:3, 3] = centre
    s.add_instance(mesh, mat, m)
    return s


def covered(oracle) -> np.ndarray:
    """(H, W) bool: the pixels of the oracle's current G-buffer with depth > 0."""
    pos = np.ascontiguousarray(oracle.output(11)).view(np.float32)
    return pos.reshape(-1, 4)[:, 3] > 0


def pan_camera(cam, dx):
    """The camera and its target moved sideways by dx: the view slides over the scene."""
    from hikari_amd import Camera, Transform
    t = np.asarray(cam.transform.translation, np.float64)
    return Camera(Transform.from_xyz(t[0] + dx, t[1], t[2]).looking_at((dx, 1.0, 0.0)))
