"""Exact restatement of what ops.label_class_regions and ops.ClassRegionMatcher compute on the device: scipy and
numpy only, no GPU and no project code.

A pixel of a uint8 label map has class c iff its value is c with 1 <= c < C; 0 and every value >= C are background.  A
class region is an 8-connected component of pixels of one class in one image.

class_regions64(maps, C): per image and class scipy.ndimage.label(map == c, np.ones((3, 3))), renumbered canonically
as tests/_region_auc_ref.regions64 does: region = 1 + the smallest linear index y * w + x of the region, sizes = the
region's pixel count at each of its pixels, both 0 on background; counts [n, C] = regions per image and class.

match_records(truth, pred, C, min_pixels): a predicted region is kept iff its size >= min_pixels.  hit of a truth region
= its pixels whose predicted class is the region's and whose predicted region is kept; hit of a kept predicted region =
its pixels whose truth class is its class.  One record (image, class, root index, size, hit) per truth region and per
kept predicted region, each array sorted by (image, root index).
"""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), int)


def classes_of(maps, C):
    m = np.asarray(maps).astype(np.int64)
    return np.where((m >= 1) & (m < C), m, 0)


def _canonical(mask):
    """(region, sizes, number of regions) of one 2-D boolean mask"""
    lab, n = ndimage.label(mask, structure=EIGHT)
    flat = lab.ravel()
    first = np.full(n + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))             # smallest linear index per label
    canon = first + 1
    canon[0] = 0
    count = np.bincount(flat, minlength=n + 1).astype(np.int64)
    count[0] = 0
    return canon[lab], count[lab], n


def class_regions64(maps, C):
    cls = classes_of(maps, C)
    assert cls.ndim == 3
    region, sizes = np.zeros(cls.shape, np.int64), np.zeros(cls.shape, np.int64)
    counts = np.zeros((cls.shape[0], C), np.int64)
    for i in range(cls.shape[0]):
        for c in range(1, C):
            r, s, k = _canonical(cls[i] == c)
            region[i] += r                                       # the classes' regions are disjoint
            sizes[i] += s
            counts[i, c] = k
    return region, sizes, counts


def _sorted(records):
    a = np.array(records, np.int64).reshape(-1, 5)
    return a[np.lexsort((a[:, 2], a[:, 0]))]


def match_records(truth, pred, C, min_pixels=1, image_base=0):
    tc, pc = classes_of(truth, C), classes_of(pred, C)
    assert tc.shape == pc.shape and min_pixels >= 1
    treg, tsz, _ = class_regions64(truth, C)
    preg, psz, _ = class_regions64(pred, C)
    kept = psz >= min_pixels
    agree = (tc > 0) & (tc == pc) & kept
    trec, prec = [], []
    per = tc.shape[1] * tc.shape[2]
    for i in range(tc.shape[0]):
        on = agree[i].ravel()
        for out, cls, reg, sz, keep in ((trec, tc[i].ravel(), treg[i].ravel(), tsz[i].ravel(), None),
                                        (prec, pc[i].ravel(), preg[i].ravel(), psz[i].ravel(), kept[i].ravel())):
            hits = np.bincount(reg[on], minlength=per + 1)       # agreeing pixels per region, by region number
            mine = reg > 0 if keep is None else (reg > 0) & keep
            for number in np.unique(reg[mine]):
                root = number - 1
                out.append((image_base + i, cls[root], root, sz[root], hits[number]))
    return _sorted(trec), _sorted(prec)
