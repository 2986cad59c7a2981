"""Exact restatement of what ops.measure_class_regions computes on the device: numpy only on top of the region
reference (tests/_seg_regions_ref.class_regions64), no GPU and no project code.  Brute force per region.

One record of 11 + 2 D int64 per class region with size >= min_pixels, sorted by (image, root index):
image_base + image, root index y * w + x (the region's smallest), size, sum_xx, sum_yy, sum_xy (sums of x x, y y, x y
over the region's pixels), q1, q2, qd, q3, q4 (bit quads: the (h + 1)(w + 1) 2 x 2 windows of the region's own mask,
padded with one ring of zeros, that hold one member, two edge-adjacent members, two diagonal members, three, four),
pmin_0 .. pmin_{D-1}, pmax_0 .. pmax_{D-1} (extremes of x c_k + y s_k over the region's pixels).
(c_k, s_k) = (rint(cos(pi k / D) 2^14), rint(sin(pi k / D) 2^14)).
"""
import numpy as np

from _seg_regions_ref import class_regions64

HEAD = 11


def directions(D):
    a = np.pi * np.arange(D, dtype=np.float64) / D
    return np.stack([np.rint(np.cos(a) * 16384), np.rint(np.sin(a) * 16384)], axis=1).astype(np.int64)


def quads(mask):
    """(q1, q2, qd, q3, q4) of a boolean mask, window by window"""
    p = np.pad(np.asarray(mask, bool), 1).astype(np.int64)
    tl, tr, bl, br = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    s = tl + tr + bl + br
    diagonal = (s == 2) & (tl == br)
    return (int((s == 1).sum()), int(((s == 2) & ~diagonal).sum()), int(diagonal.sum()), int((s == 3).sum()),
            int((s == 4).sum()))


def shape_records(maps, C, min_pixels=1, image_base=0, D=32):
    maps = np.asarray(maps)
    assert maps.ndim == 3 and min_pixels >= 1
    region, sizes, _ = class_regions64(maps, C)
    n, h, w = region.shape
    table = directions(D)
    out = []
    for i in range(n):
        for number in np.unique(region[i][region[i] > 0]).tolist():
            mask = region[i] == number
            ys, xs = np.nonzero(mask)
            if len(xs) < min_pixels:
                continue
            assert sizes[i].ravel()[number - 1] == len(xs) and number - 1 == ys[0] * w + xs[0]
            p = xs[:, None] * table[None, :, 0] + ys[:, None] * table[None, :, 1]
            out.append([image_base + i, number - 1, len(xs), int((xs * xs).sum()), int((ys * ys).sum()), int((xs * ys).sum()),
                        *quads(mask), *p.min(axis=0).tolist(), *p.max(axis=0).tolist()])
    a = np.array(out, np.int64).reshape(-1, HEAD + 2 * D)
    return a[np.lexsort((a[:, 1], a[:, 0]))]
