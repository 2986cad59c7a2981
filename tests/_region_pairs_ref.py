"""Exact restatement of what ops.pair_class_regions computes on the device: numpy only, no GPU and no project code.

The two inputs are region maps [n, h, w] as tests/_seg_regions_ref.class_regions64 numbers them: 1 + the smallest linear
index y * w + x of the pixel's region, 0 on background.  A pixel carries the pair (truth id, pred id) iff both are
non-zero.  pairs(): one record (image_base + image, truth id - 1, pred id - 1, number of pixels that carry the pair) per
distinct pair of every image, int64 [K, 4], sorted by (image, truth root, pred root): np.unique with counts.
pair_starts(): per image, the pixels that carry a pair and have x == 0 or another pair (or none) to their left: what
unet_region_pair_bound counts, an upper bound on the image's distinct pairs.
"""
import numpy as np

import _seg_regions_ref as R


def pairs(truth_region, pred_region, image_base=0):
    t, p = np.asarray(truth_region, np.int64), np.asarray(pred_region, np.int64)
    assert t.shape == p.shape and t.ndim == 3
    image = np.broadcast_to(np.arange(t.shape[0])[:, None, None], t.shape)
    on = (t > 0) & (p > 0)
    rows = np.stack([image[on] + image_base, t[on] - 1, p[on] - 1], axis=1).reshape(-1, 3)
    if not len(rows):
        return np.zeros((0, 4), np.int64)
    keys, counts = np.unique(rows, axis=0, return_counts=True)          # sorted lexicographically by row
    return np.concatenate([keys, counts[:, None]], axis=1).astype(np.int64)


def pair_starts(truth_region, pred_region):
    t, p = np.asarray(truth_region, np.int64), np.asarray(pred_region, np.int64)
    on = (t > 0) & (p > 0)
    key = np.where(on, t * (1 << 32) + p, 0)
    left = np.zeros_like(key)
    left[:, :, 1:] = key[:, :, :-1]
    first = np.zeros(key.shape, bool)
    first[:, :, 0] = True
    return (on & (first | (key != left))).sum(axis=(1, 2)).astype(np.int64)


def pairs_of_labels(truth, pred, C, image_base=0):
    """pairs() of the class regions of two uint8 label maps [n, h, w] of C classes"""
    return pairs(R.class_regions64(truth, C)[0], R.class_regions64(pred, C)[0], image_base)
