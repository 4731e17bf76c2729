"""The conservative screen bound behind option bg_tile_skip (hks_instance_bounds, hks_screen_bounds), on the host against
the CPU oracle's G-buffer: for seeded cameras over cornell, a single quad and a quad whose silhouette lies on a 16-pixel
tile edge +- 1 px, every pixel the oracle's primary rays cover (depth > 0) lies inside the bound taken with a guard of
1 px, which is the runtime's rectangle (guard 4) shrunk by guard - 1 before it is clipped to the frame.  A camera inside
the box has no rectangle.  A condition, not a tolerance: no camera is left out."""
import numpy as np
import pytest

from tile_skip_cases import GUARD, covered, quad_scene, screen_bounds, world_box


def _check(o, box, fi, w, h, label):
    """The oracle's G-buffer of `fi` against the bound; returns (has rectangle, covered pixels)."""
    o.render_gbuffer(fi)
    c = covered(o).reshape(h, w)
    inner, outer = screen_bounds(box, fi.view, w, h, 1), screen_bounds(box, fi.view, w, h, GUARD)
    assert (inner is None) == (outer is None), label
    if inner is None:
        return False, int(c.sum())
    x0, y0, x1, y1 = inner
    out = c.copy()
    out[y0:y1, x0:x1] = False
    assert not out.any(), f"{label}: covered pixels {np.argwhere(out)[:4].tolist()} outside {inner}"
    X0, Y0, X1, Y1 = outer
    if x1 > x0:  # the guard band only grows the rectangle
        assert X0 <= x0 and Y0 <= y0 and X1 >= x1 and Y1 >= y1, label
        assert X0 == max(0, x0 - (GUARD - 1)) and X1 == min(w, x1 + (GUARD - 1)), label
    return True, int(c.sum())


def _cameras(rng, n, centre, ortho_every=4):
    """Seeded cameras around `centre`: eyes 2.5 to 9 units away, looking at points up to 5 units off the centre (the
    scene partly or wholly off screen), every ortho_every-th one orthographic."""
    from hikari_amd import Camera, Transform
    out = []
    for k in range(n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        eye = centre + d * rng.uniform(2.5, 9.0)
        target = centre + rng.uniform(-1.0, 1.0, 3) * rng.choice([0.3, 2.0, 5.0])
        t = Transform.from_xyz(*eye).looking_at(tuple(target))
        out.append(Camera.orthographic(t, float(rng.uniform(1.5, 8.0))) if k % ortho_every == 3 else Camera(t))
    return out


SIZES = [(192, 96), (96, 64), (80, 48)]


@pytest.mark.parametrize("name", ["cornell", "quad"])
def test_covered_pixels_lie_inside_the_bound(name):
    from hikari_amd import examples, frame_inputs, load_noise
    from oracle import Oracle
    if name == "cornell":
        scene, cam, lights = examples.cornell()
    else:
        scene, (_, cam, lights) = quad_scene(), examples.cornell()
    desc = scene.build()
    box = world_box(scene)
    rng = np.random.default_rng(20 if name == "cornell" else 21)
    centre = 0.5 * (box[:3] + box[3:])
    total = with_rect = hit = partly = empty = 0
    for w, h in SIZES:
        for ratio, jitter in ((1.0, 0), (1.5, 1), (2.0, 2)):
            o = Oracle(desc, load_noise(), w, h, ratio)
            # the scene's own camera and an orbit around it, then the seeded ones
            from parity import orbit_camera
            cams = [cam] + [orbit_camera(cam, f) for f in range(1, 5)] + _cameras(rng, 12, centre)
            for k, c in enumerate(cams):
                fi = frame_inputs(k, c, lights, w, h, jitter=jitter)
                ok, n = _check(o, box, fi, w, h, f"{name} {w}x{h} ratio {ratio} camera {k}")
                total += 1
                with_rect += ok
                hit += n > 0
                if ok:
                    r = screen_bounds(box, fi.view, w, h, 1)
                    empty += r[2] <= r[0]
                    partly += r[2] > r[0] and (r[0] == 0 or r[1] == 0 or r[2] == w or r[3] == h)
    assert total >= 150
    # the cases are not vacuous: most cameras have a rectangle and see the scene, some see it cut by the frame's
    # edge, some not at all
    assert with_rect >= total // 2 and hit >= total // 3 and partly >= 5 and empty >= 1, (total, with_rect, hit, partly, empty)


def test_silhouette_on_a_tile_edge():
    """An orthographic view maps the quad's edges to exact pixel columns and rows: its right edge on column 64 (a tile
    edge of every 16-pixel grid) and 1 px to either side, its top edge likewise on row 16, with every prepass jitter."""
    from hikari_amd import Camera, Transform, examples, frame_inputs, load_noise
    from oracle import Oracle
    _, _, lights = examples.cornell()
    w, h = 128, 64
    height = 4.0                     # world units over h pixels: 16 px per unit
    px = height / h
    n = 0
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            # quad from column 32 to 64 + dx and from row 16 + dy to 48: x = (col - w / 2) px, y = (h / 2 - row) px
            x0, x1 = (32 - w / 2) * px, (64 + dx - w / 2) * px
            y1, y0 = (h / 2 - (16 + dy)) * px, (h / 2 - 48) * px
            scene = quad_scene(0.5 * (x1 - x0), 0.5 * (y1 - y0), (0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.0))
            desc = scene.build()
            box = world_box(scene)
            o = Oracle(desc, load_noise(), w, h, 1.0)
            cam = Camera.orthographic(Transform.from_xyz(0.0, 0.0, 5.0).looking_at((0.0, 0.0, 0.0)), height)
            for f, jitter in ((0, 0), (1, 1), (2, 1), (3, 2), (6, 2)):
                fi = frame_inputs(f, cam, lights, w, h, jitter=jitter)
                ok, hit = _check(o, box, fi, w, h, f"edge {dx} {dy} frame {f} jitter {jitter}")
                assert ok and hit > 0
                r = screen_bounds(box, fi.view, w, h, GUARD)
                # the runtime's rectangle reaches past the edge by the guard, no further than guard + 2 px
                assert 64 + dx + GUARD <= r[2] <= 64 + dx + GUARD + 2, (dx, r)
                assert 16 + dy - GUARD - 2 <= r[1] <= 16 + dy - GUARD, (dy, r)
                n += 1
    assert n == 45


def test_camera_inside_the_box_has_no_rectangle():
    from hikari_amd import Camera, Transform, examples, frame_inputs
    scene, cam, lights = examples.cornell()
    scene.build()
    box = world_box(scene)
    rng = np.random.default_rng(22)
    for k in range(24):
        eye = box[:3] + rng.uniform(0.02, 0.98, 3) * (box[3:] - box[:3])
        t = Transform.from_xyz(*eye).looking_at(tuple(eye + rng.normal(size=3)))
        for c in (Camera(t), Camera.orthographic(t, 3.0)):
            assert screen_bounds(box, frame_inputs(k, c, lights, 96, 64).view, 96, 64) is None
    # ... and a box behind the eye, or an eye that is not the projection's centre
    away = Camera(Transform.from_xyz(0.0, 1.0, 4.0).looking_at((0.0, 1.0, 9.0)))
    assert screen_bounds(box, frame_inputs(0, away, lights, 96, 64).view, 96, 64) is None
    v = frame_inputs(0, cam, lights, 96, 64).view
    assert screen_bounds(box, v, 96, 64) is not None
    v.world_position[0] += 0.5
    assert screen_bounds(box, v, 96, 64) is None


def test_instance_bounds_hold_the_records_boxes():
    """hks_instance_bounds over the models and local boxes holds every instance record's f32 box, within 1e-4 of it."""
    from hikari_amd import examples
    from parity import moved
    for seed in range(4):
        scene, _, _ = moved(examples.cornell(), seed)
        scene.build()
        box = world_box(scene)
        inst = np.frombuffer(scene.arrays()["instances"].tobytes(), np.float32).reshape(-1, 44)
        lo, hi = inst[:, 0:3].min(axis=0).astype(np.float64), inst[:, 4:7].max(axis=0).astype(np.float64)
        assert (box[:3] <= lo).all() and (box[3:] >= hi).all()
        assert np.abs(box[:3] - lo).max() < 1e-3 and np.abs(box[3:] - hi).max() < 1e-3
