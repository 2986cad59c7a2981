"""Exact restatement of what ops.describe_class_regions computes on the device: numpy only on top of the region
reference (tests/_seg_regions_ref.class_regions64), no GPU and no project code.

One record of 12 int64 per class region with size >= min_pixels, sorted by (image, root index):
image_base + image, class, root index y * w + x (the region's smallest), size, x0, y0, x1, y1 (inclusive box), sum_x,
sum_y (sums of the pixels' coordinates), conf_sum_q, conf_max_q (sum and maximum over the region's pixels of q(v)).
q(v) = rint(clip(v, 0, 1) * 65536) on float32 (np.rint: ties to even); without conf both are 0.
"""
import numpy as np

from _seg_regions_ref import class_regions64, classes_of

FIELDS = 12


def q16(conf):
    c = np.clip(np.asarray(conf, np.float32), np.float32(0), np.float32(1))
    return np.rint(c * np.float32(65536)).astype(np.int64)


def describe_records(maps, C, conf=None, min_pixels=1, image_base=0):
    maps = np.asarray(maps)
    assert maps.ndim == 3 and min_pixels >= 1
    cls = classes_of(maps, C)
    region, sizes, _ = class_regions64(maps, C)
    n, h, w = cls.shape
    q = np.zeros(cls.shape, np.int64) if conf is None else q16(conf)
    assert q.shape == cls.shape
    out = []
    for i in range(n):
        on = np.flatnonzero((region[i] > 0) & (sizes[i] >= min_pixels))
        if on.size == 0:
            continue
        numbers, inv = np.unique(region[i].ravel()[on], return_inverse=True)
        ys, xs = np.divmod(on, w)
        qs = q[i].ravel()[on]
        k = len(numbers)
        lo_x, lo_y = np.full(k, w, np.int64), np.full(k, h, np.int64)
        hi_x, hi_y, hi_q = np.full(k, -1, np.int64), np.full(k, -1, np.int64), np.zeros(k, np.int64)
        np.minimum.at(lo_x, inv, xs); np.minimum.at(lo_y, inv, ys)
        np.maximum.at(hi_x, inv, xs); np.maximum.at(hi_y, inv, ys); np.maximum.at(hi_q, inv, qs)
        rec = np.zeros((k, FIELDS), np.int64)
        roots = numbers - 1
        rec[:, 0] = image_base + i
        rec[:, 1] = cls[i].ravel()[roots]
        rec[:, 2] = roots
        rec[:, 3] = np.bincount(inv, minlength=k)
        rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = lo_x, lo_y, hi_x, hi_y
        rec[:, 8] = np.bincount(inv, weights=xs, minlength=k).astype(np.int64)       # exact: far below 2^53
        rec[:, 9] = np.bincount(inv, weights=ys, minlength=k).astype(np.int64)
        rec[:, 10] = np.bincount(inv, weights=qs, minlength=k).astype(np.int64)
        rec[:, 11] = hi_q
        assert np.array_equal(rec[:, 3], sizes[i].ravel()[roots])
        out.append(rec)
    if not out:
        return np.zeros((0, FIELDS), np.int64)
    a = np.concatenate(out)
    return a[np.lexsort((a[:, 2], a[:, 0]))]
