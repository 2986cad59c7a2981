"""Numpy restatement of csrc/distance.hip for the tests: class boundaries by shifted comparison, the exact squared
distance separably (a column pass, then per row the minimum over x' by broadcasting), the (image, class) records and the
pooled histogram by plain loops over the boundary pixels with math.isqrt.  Pinned to scipy's distance transform and a
brute-force minimum by test_cpu_boundaries.py."""
import math

import numpy as np

NONE = 1 << 30
FIELDS = (("image", "class", "t_pixels", "p_pixels", "t_boundary", "p_boundary")
          + tuple(f"p_near{k}" for k in range(4)) + tuple(f"t_near{k}" for k in range(4))
          + ("band_inter", "band_union", "p_dist_sum_q8", "t_dist_sum_q8", "p_dist_max_sq", "t_dist_max_sq"))
F = {name: i for i, name in enumerate(FIELDS)}
BINS = 1025


def class_mask(labels, c):
    return np.asarray(labels) == c


def boundary_mask(mask):
    """bool [h, w]: pixels of the mask with a 4-neighbour inside the frame that is not of it"""
    m = np.asarray(mask, bool)
    other = np.zeros_like(m)
    other[1:, :] |= ~m[:-1, :]
    other[:-1, :] |= ~m[1:, :]
    other[:, 1:] |= ~m[:, :-1]
    other[:, :-1] |= ~m[:, 1:]
    return m & other


def distance_sq(boundary):
    """int64 [h, w]: the exact squared distance to the nearest True pixel, NONE without one"""
    b = np.asarray(boundary, bool)
    h, w = b.shape
    if not b.any():
        return np.full((h, w), NONE, np.int64)
    big = 1 << 40
    g = np.full((h, w), big, np.int64)                 # vertical distance: down the columns, then up
    last = np.full(w, -1, np.int64)
    for y in range(h):
        last[b[y]] = y
        g[y] = np.where(last >= 0, y - last, big)
    nxt = np.full(w, -1, np.int64)
    for y in range(h - 1, -1, -1):
        nxt[b[y]] = y
        g[y] = np.minimum(g[y], np.where(nxt >= 0, nxt - y, big))
    g2 = np.where(g >= big, big, g * g)
    xs = np.arange(w, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2             # [x, x']
    out = np.empty((h, w), np.int64)
    for y in range(h):
        out[y] = (g2[y][None, :] + dx2).min(axis=1)
    return out


def distance_sq_brute(boundary):
    b = np.asarray(boundary, bool)
    h, w = b.shape
    ys, xs = np.nonzero(b)
    if len(ys) == 0:
        return np.full((h, w), NONE, np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
    return d.min(axis=-1).astype(np.int64)


def boundary_distance_sq(labels, num_classes):
    """int64 [n, num_classes - 1, h, w] of label maps [n, h, w]"""
    labels = np.asarray(labels)
    n, h, w = labels.shape
    out = np.empty((n, num_classes - 1, h, w), np.int64)
    for i in range(n):
        for c in range(1, num_classes):
            out[i, c - 1] = distance_sq(boundary_mask(class_mask(labels[i], c)))
    return out


def band_width(h, w):
    return max(1, round(0.02 * math.sqrt(h * h + w * w)))


def stats(truth, pred, num_classes, tolerances, band, image_base=0, hist=None):
    """(records int64 [n * (num_classes - 1), 20] sorted by (image, class), hist int64 [num_classes - 1, 2, 1025]);
    ``hist`` is added to when it is given"""
    truth, pred = np.asarray(truth), np.asarray(pred)
    n = truth.shape[0]
    if hist is None:
        hist = np.zeros((num_classes - 1, 2, BINS), np.int64)
    rows = []
    for i in range(n):
        for c in range(1, num_classes):
            tm, pm = class_mask(truth[i], c), class_mask(pred[i], c)
            tb, pb = boundary_mask(tm), boundary_mask(pm)
            dt, dp = distance_sq(tb), distance_sq(pb)
            r = [0] * len(FIELDS)
            r[F["image"]], r[F["class"]] = image_base + i, c
            r[F["t_pixels"]], r[F["p_pixels"]] = int(tm.sum()), int(pm.sum())
            r[F["t_boundary"]], r[F["p_boundary"]] = int(tb.sum()), int(pb.sum())
            in_t, in_p = tm & (dt <= band * band), pm & (dp <= band * band)
            r[F["band_inter"]], r[F["band_union"]] = int((in_t & in_p).sum()), int((in_t | in_p).sum())
            for side, mine, other, direction in (("p", pb, dt, 0), ("t", tb, dp, 1)):
                for y, x in zip(*np.nonzero(mine)):
                    d2 = int(other[y, x])
                    if d2 == NONE:
                        continue
                    for k, tol in enumerate(tolerances):
                        if d2 <= tol * tol:
                            r[F[f"{side}_near{k}"]] += 1
                    r[F[f"{side}_dist_sum_q8"]] += math.isqrt(d2 << 16)
                    r[F[f"{side}_dist_max_sq"]] = max(r[F[f"{side}_dist_max_sq"]], d2)
                    hist[c - 1, direction, min(math.isqrt(d2), BINS - 1)] += 1
            rows.append(r)
    return np.array(rows, np.int64).reshape(-1, len(FIELDS)), hist
