"""The host arithmetic behind the tone pass over the kept rectangle and the background tile skip's kept tiles
(hikari_scene.h hks_tone_rect, hks_keep_tiles) against a plain Python restatement: a pixel rectangle in frame
coordinates -> the tone kernel's run range in a plane's own coordinates (columns outward to whole runs), and -> the
tiles of a launch's own 16x16 grid that meet it (the size and tile offset of a grid over them alone).  Rectangles on each frame edge, the empty one, the whole frame,
widths that are no multiple of 16 and an odd width, whole frames, row bands and column tiles."""
import ctypes as C

import pytest

ALL = 2**31 - 1  # the runtime's "no bound" edge


def _vec(values, ctype=C.c_int32):
    return (ctype * len(values))(*values)


def tone_rect(keep, window, row0, run):
    from hikari_amd import _abi
    out = (C.c_int32 * 4)()
    rc = _abi.lib().hks_tone_rect(_vec(keep), _vec(window), row0, run, out)
    assert rc in (0, 1)
    assert rc == 1 or tuple(out) == (0, 0, 0, 0)
    return tuple(out) if rc else None


def keep_tiles(keep, window, row0, tile=16):
    from hikari_amd import _abi
    out = (C.c_uint32 * 4)()
    rc = _abi.lib().hks_keep_tiles(_vec(keep), _vec(window), row0, tile, out)
    assert rc in (0, 1)
    assert rc == 1 or tuple(out) == (0, 0, 0, 0)
    return tuple(out) if rc else None


def py_tone_rect(keep, window, row0, run):
    """The pixels of `keep` (frame coordinates) inside the window (plane coordinates, plane row r = frame row row0 + r),
    by enumeration of the window's columns and rows; the columns then outward to multiples of run."""
    xs = [x for x in range(window[0], window[2]) if keep[0] <= x < keep[2]]
    ys = [y for y in range(window[1], window[3]) if keep[1] <= y + row0 < keep[3]]
    if not xs or not ys:
        return None
    return (min(xs) // run * run, min(ys), -(-(max(xs) + 1) // run) * run, max(ys) + 1)


def py_keep_tiles(keep, window, row0, tile=16):
    """The tiles of the window's own grid (tile (0, 0) at the window's first column and row) holding a pixel of keep."""
    gx, gy = -(-(window[2] - window[0]) // tile), -(-(window[3] - window[1]) // tile)
    tx = [t for t in range(gx) if any(keep[0] <= window[0] + tile * t + i < keep[2] for i in range(tile))]
    ty = [t for t in range(gy) if any(keep[1] <= row0 + window[1] + tile * t + i < keep[3] for i in range(tile))]
    if not tx or not ty:
        return None
    return (min(tx), min(ty), max(tx) + 1, max(ty) + 1)


def _rects(w, h):
    """Rectangles of a w x h frame: on each edge, in each corner, in the middle (odd and even edges), one pixel, the
    whole frame, the runtime's unbounded one, empty ones."""
    return [
        (0, 0, w, h), (0, 0, ALL, ALL), (0, 5, 9, h - 3), (w - 7, 4, w, 20), (3, 0, w - 3, 6), (11, h - 5, 30, h),
        (0, 0, 1, 1), (w - 1, h - 1, w, h), (17, 9, 46, 31), (16, 16, 48, 32), (15, 15, 49, 33), (33, 7, 34, 8),
        (0, 0, 0, 0), (20, 10, 20, 30), (20, 10, 40, 10), (w, 0, w + 8, h),
    ]


FRAMES = [(96, 64), (176, 112), (100, 70), (161, 96)]  # 100 and 161: no multiples of 16; 161: odd


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tone_rect_whole_frame_window(size):
    w, h = size
    run = 2
    window = (0, 0, w - w % run, h)  # (an odd plane takes the per-texel kernel: the arithmetic on its even part)
    for keep in _rects(w, h):
        got, want = tone_rect(keep, window, 0, run), py_tone_rect(keep, window, 0, run)
        assert got == want, (keep, got, want)
        if got:
            assert window[0] <= got[0] < got[2] <= window[2] and window[1] <= got[1] < got[3] <= window[3]
            assert got[0] % run == 0 and got[2] % run == 0


@pytest.mark.parametrize("run", [1, 2, 4, 8])
def test_tone_rect_bands_tiles_and_runs(run):
    """A row band with halo rows (plane row 0 is frame row 22, the window rows 3..35 of the plane) and a column tile
    (window columns 48..112), each run length."""
    w, h = 176, 112
    for window, row0 in (((0, 3, w, 35), 22), ((48, 0, 112, h), 0), ((48, 2, 112, 40), 50)):
        for keep in _rects(w, h):
            got, want = tone_rect(keep, window, row0, run), py_tone_rect(keep, window, row0, run)
            assert got == want, (window, row0, keep, got, want)


def test_tone_rect_refuses_unusable_arguments():
    assert tone_rect((0, 0, 10, 10), (0, 0, 16, 16), 0, 0) is None       # no run
    assert tone_rect((0, 0, 10, 10), (1, 0, 17, 16), 0, 2) is None       # window off the runs
    assert tone_rect((0, 0, 10, 10), (0, 0, 15, 16), 0, 2) is None
    assert tone_rect((0, 0, 10, 10), (0, 0, 0, 16), 0, 2) is None        # empty window
    from hikari_amd import _abi
    assert _abi.lib().hks_tone_rect(None, None, 0, 2, None) == 0


@pytest.mark.parametrize("size", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_keep_tiles(size):
    w, h = size
    windows = [((0, 0, w, h), 0), ((0, 3, w, 35), 22), ((48, 0, 96, h), 0), ((32, 2, 90, 40), 17)]
    for window, row0 in windows:
        gx, gy = -(-(window[2] - window[0]) // 16), -(-(window[3] - window[1]) // 16)
        for keep in _rects(w, h):
            got, want = keep_tiles(keep, window, row0), py_keep_tiles(keep, window, row0)
            assert got == want, (window, row0, keep, got, want)
            if got:  # the launch grid and its tile offset
                assert 0 <= got[0] < got[2] <= gx and 0 <= got[1] < got[3] <= gy
    assert keep_tiles((0, 0, ALL, ALL), (0, 0, w, h), 0) == (0, 0, -(-w // 16), -(-h // 16))
    assert keep_tiles((0, 0, 8, 8), (0, 0, w, h), 0, tile=0) is None
