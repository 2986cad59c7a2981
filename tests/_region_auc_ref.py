"""Exact restatement of what ops.label_regions and ops.RegionOverlapAUC compute on the device.

regions64(mask): the 8-connected components of one 2-D boolean mask (scipy.ndimage.label with the 3x3 structure),
renumbered canonically: label = 1 + the smallest linear index y * w + x of the region, 0 elsewhere; sizes = the region's
pixel count at each of its pixels.

aupro64(scores, masks, limit): AUPRO of the MVTec AD evaluation.  With R regions and N ok pixels over all images, walk
the distinct scores v downwards from (0, 0): fpr = #{ok >= v} / N, pro = sum over defective pixels >= v of 1 / (R size);
the area below the piecewise-linear curve over fpr in [0, L], the crossing segment cut at L, divided by L.  Evaluated
in exact rational arithmetic (the limit is the double's exact value) and rounded once: by linearity the area is the sum
over the defective pixels (value v, region size s, [x0, x1] = [#ok > v, #ok >= v] / N) of
    1 / (s R) * (L - (x0 + x1) / 2)  if x1 <= L,   1 / (s R) * (L - x0)^2 / (2 (x1 - x0))  if x0 < L < x1,   else 0,
grouped by region size so that only a few fractions are ever formed.  test_cpu_region_auc.py pins it against the walk
itself and against a cumsum / argsort formulation.  No region, no ok pixel or any NaN / inf score: 0.0.
"""
from fractions import Fraction

import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), int)


def regions64(mask):
    m = np.asarray(mask, bool)
    assert m.ndim == 2
    lab, n = ndimage.label(m, structure=EIGHT)
    flat = lab.ravel()
    _, first = np.unique(flat, return_index=True)            # first occurrence = smallest linear index, per label
    if not (flat == 0).any():
        first = np.r_[0, first]
    canon = np.r_[0, first[1:] + 1].astype(np.int64)
    count = np.bincount(flat, minlength=n + 1).astype(np.int64)
    count[0] = 0
    return canon[lab], count[lab], n


def _planes(a):
    a = np.asarray(a)
    n, w = a.shape[0], a.shape[-1]
    h = a.shape[-2] if a.ndim >= 3 else 1
    return a.reshape(n, h, w)


def aupro64(scores, masks, limit=0.3):
    s = _planes(np.asarray(scores, np.float32))
    m = _planes(np.asarray(masks, bool))
    assert s.shape == m.shape
    L = Fraction(float(limit))
    assert 0 < L <= 1
    sizes = np.zeros(m.shape, np.int64)
    R = 0
    for i in range(m.shape[0]):
        _, sizes[i], k = regions64(m[i])
        R += k
    s, sizes = s.ravel(), sizes.ravel()
    finite = np.isfinite(s)
    defect = sizes > 0
    res = {"aupro": 0.0, "pro_at_limit": 0.0, "fpr_limit": float(limit), "regions": R, "defective": int(defect.sum()),
           "ok": int((~defect).sum()), "nonfinite": int((~finite).sum())}
    if res["nonfinite"] or R == 0 or res["ok"] == 0:
        return res
    v = s.astype(np.float64) + 0.0                           # + 0.0: -0.0 becomes +0.0
    neg = np.sort(v[~defect])
    pos, size = v[defect], sizes[defect]
    N = int(neg.size)
    c1 = N - np.searchsorted(neg, pos, "left").astype(np.int64)      # ok pixels at or above the value
    c0 = N - np.searchsorted(neg, pos, "right").astype(np.int64)     # ok pixels above it
    LN = L * N
    kfloor, kceil = LN.numerator // LN.denominator, -((-LN.numerator) // LN.denominator)
    full = c1 <= kfloor
    cross = ~full & (c0 < kceil)
    assert int(pos.size) * 2 * N < 2 ** 63
    area, pro = Fraction(0), Fraction(0)
    order = np.argsort(size[full], kind="stable")
    if order.size:
        ss, cc = size[full][order], (c0 + c1)[full][order]
        heads = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1]])
        sums = np.add.reduceat(cc, heads)
        counts = np.diff(np.r_[heads, ss.size])
        for sz, cnt, tot in zip(ss[heads].tolist(), counts.tolist(), sums.tolist()):
            area += (cnt * L - Fraction(tot, 2 * N)) / sz
            pro += Fraction(cnt, sz)
    if cross.any():                                          # the pixels of the one value whose segment crosses L
        a, b = int(c0[cross][0]), int(c1[cross][0])
        assert (c0[cross] == a).all() and (c1[cross] == b).all()
        t = LN - a
        for sz, cnt in zip(*(x.tolist() for x in np.unique(size[cross], return_counts=True))):
            area += cnt * t * t / (2 * N * (b - a)) / sz
            pro += cnt * t / (b - a) / sz
    res["aupro"] = float(area / (R * L))
    res["pro_at_limit"] = float(pro / R)
    return res
