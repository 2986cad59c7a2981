"""The label maps that the grouping tests share (tests/test_cpu_groups.py pins what the reference makes of them,
tests/test_gpu_groups.py holds the device to the reference on them).  numpy only.  Four classes: 1, 2, 3 and background;
4, 200 and 255 are background too.

layout_a (h >= 33, w >= 65): what a grouping kernel with 32 x 32 tiles can get wrong at gaps 2 and 5.
layout_b (h >= 22, w >= 65): the pairs exactly at and just past the largest gap, 32.
"""
import functools

import numpy as np

C = 4
GAPS = (1, 2, 5, 32)
SHAPES = ((1, 1, 1), (1, 1, 70), (1, 70, 1), (2, 33, 65), (3, 40, 100))      # (n, h, w)


def layout_a(h, w):
    assert h >= 33 and w >= 65
    m = np.zeros((h, w), np.uint8)
    for c, y in ((1, 5), (2, 8)):                      # a chain of three, 4 apart: one group from gap 4, in two classes
        m[y, 2:7] = c; m[y, 10:15] = c; m[y, 18:23] = c
    m[14:16, 2:4] = 3; m[14, 7] = 3; m[14:16, 11:13] = 3      # two blocks 8 apart and one pixel 4 from each: the bridge
    m[30:33, 28:37] = 1                                # across the tile borders x = 32 and y = 32
    m[30:33, 62:65] = 1                                # across x = 64, 26 from the last: one group at gap 32 only
    m[0, 0] = 2; m[0, w - 1] = 2; m[h - 1, 0] = 2      # the frame's corners
    m[20, w - 1] = 3; m[21, 0] = 3                     # neighbours in memory, w - 1 apart in the frame
    m[24, 40] = 3; m[27, 44] = 3                       # d^2 = 25
    m[24, 52] = 3; m[25, 57] = 3                       # d^2 = 26
    m[24, 20] = 2; m[24, 22] = 2                       # d^2 = 4
    m[28, 20] = 2; m[29, 22] = 2                       # d^2 = 5
    m[18, 30:34] = 200; m[19, 30:34] = 4               # background whatever it says
    return m


def layout_b(h, w):
    assert h >= 22 and w >= 65
    m = np.zeros((h, w), np.uint8)
    m[2, 3] = 1; m[2, 35] = 1                          # d^2 = 1024
    m[20, 3] = 2; m[21, 35] = 2                        # d^2 = 1025
    m[10, w - 1] = 3; m[11, 0] = 3
    return m


def _line(k):
    v = np.zeros(k, np.uint8)
    for at in (0, 2, 7, 39, 69):                       # 2, 5 and 32 apart, and the last pixel of the frame
        if at < k:
            v[at] = 1
    if k > 50:
        v[45:48] = 2; v[50] = 2                        # a run and a pixel 3 from its end
    return v


def speckle(n, h, w, density, seed):
    rng = np.random.default_rng(seed)
    on = rng.random((n, h, w)) < density
    return np.where(on, rng.choice(np.array([1, 2, 3, 1, 2, 3, 4, 255], np.uint8), (n, h, w)), 0).astype(np.uint8)


KINDS = ("layout", "speckle02", "speckle30")


@functools.lru_cache(maxsize=None)
def maps_of(shape, kind):
    """uint8 [n, h, w], built once and read-only"""
    n, h, w = shape
    if kind == "layout":
        if (h, w) == (1, 1):
            m = np.full((1, 1, 1), 3, np.uint8)
        elif h == 1:
            m = _line(w)[None, None, :]
        elif w == 1:
            m = _line(h)[None, :, None]
        else:
            a = layout_a(h, w)
            images = [a, layout_b(h, w)]
            if n == 3:
                images.insert(1, np.where((a >= 1) & (a < C), a % 3 + 1, a).astype(np.uint8))     # the classes rotated
            m = np.stack(images)
    else:
        m = speckle(n, h, w, {"speckle02": 0.02, "speckle30": 0.3}[kind], 11 * h + w)
    m = np.ascontiguousarray(m, np.uint8)
    assert m.shape == shape
    m.setflags(write=False)
    return m
