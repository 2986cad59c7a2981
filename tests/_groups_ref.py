"""Exact restatement of what ops.group_class_regions computes on the device: numpy only on top of the region reference
(tests/_seg_regions_ref.class_regions64), no GPU and no project code.

A fragment is a class region with size >= min_pixels; smaller regions are dropped before grouping.  Two fragments of one
image and one class are linked iff they hold pixels p, q with (py - qy)^2 + (px - qx)^2 <= gap^2; a group is a connected
component of the link graph.  group = 1 + the smallest fragment root of the pixel's group, group_sizes = the group's
pixel count at each of its pixels, both 0 on background and on dropped regions; counts [n, C] = groups per image and
class; fragments = one row (image_base + image, class, fragment root, group root, fragment size) per fragment, sorted
by (image, group root, fragment root).

group_regions64: for every offset (dy, dx) of the half-disc (dy > 0, or dy == 0 and dx > 0) the class and region maps
are compared with themselves shifted by the offset, without wrapping; the pairs of region numbers found are joined by a
host union-find that keeps the smallest root.
brute_groups64: the same outputs from the all-pairs distances of the fragments' pixels, for small maps.
"""
import numpy as np

from _seg_regions_ref import class_regions64, classes_of

FIELDS = 5


def half_disc(gap):
    return [(dy, dx) for dy in range(gap + 1) for dx in range(-gap, gap + 1)
            if (dy > 0 or dx > 0) and dy * dy + dx * dx <= gap * gap]


def _find(parent, a):
    while parent[a] != a:
        a = parent[a]
    return a


def _outputs(cls, region, sizes, kept, links, C, image_base):
    """links: per image an iterable of (region number, region number) pairs of linked fragments"""
    n, h, w = cls.shape
    group, gsizes = np.zeros(cls.shape, np.int64), np.zeros(cls.shape, np.int64)
    counts = np.zeros((n, C), np.int64)
    rows = []
    for i in range(n):
        numbers = np.unique(region[i][kept[i]])
        parent = {int(v): int(v) for v in numbers}
        for a, b in links[i]:
            a, b = _find(parent, int(a)), _find(parent, int(b))
            if a != b:
                parent[max(a, b)] = min(a, b)                    # the smallest root stays the root
        top = {v: _find(parent, v) for v in parent}
        total = {}
        flat_c, flat_s = cls[i].ravel(), sizes[i].ravel()
        for v, g in top.items():
            total[g] = total.get(g, 0) + int(flat_s[v - 1])
        lut_g, lut_s = np.zeros(h * w + 1, np.int64), np.zeros(h * w + 1, np.int64)
        for v, g in top.items():
            lut_g[v], lut_s[v] = g, total[g]
            rows.append((image_base + i, int(flat_c[v - 1]), v - 1, g - 1, int(flat_s[v - 1])))
            if v == g:
                counts[i, flat_c[v - 1]] += 1
        ids = np.where(kept[i], region[i], 0)
        group[i], gsizes[i] = lut_g[ids], lut_s[ids]
    frag = np.array(rows, np.int64).reshape(-1, FIELDS)
    frag = frag[np.lexsort((frag[:, 2], frag[:, 3], frag[:, 0]))]
    return group, gsizes, counts, frag


def _labelled(maps, C, min_pixels):
    maps = np.asarray(maps)
    assert maps.ndim == 3 and min_pixels >= 1
    cls = classes_of(maps, C)
    region, sizes, _ = class_regions64(maps, C)
    return cls, region, sizes, (region > 0) & (sizes >= min_pixels)


def group_regions64(maps, C, gap, min_pixels=1, image_base=0):
    assert 1 <= gap <= 32
    cls, region, sizes, kept = _labelled(maps, C, min_pixels)
    n, h, w = cls.shape
    ids = np.where(kept, region, 0)
    links = []
    for i in range(n):
        found = set()
        for dy, dx in half_disc(gap):
            if dy >= h or abs(dx) >= w:
                continue
            # p = (y, x) against q = (y + dy, x + dx), both inside the frame: a row never wraps
            ys, xs = slice(0, h - dy), slice(max(0, -dx), min(w, w - dx))
            yq, xq = slice(dy, h), slice(max(0, -dx) + dx, min(w, w - dx) + dx)
            a, b = ids[i][ys, xs], ids[i][yq, xq]
            on = (a > 0) & (b > 0) & (a != b) & (cls[i][ys, xs] == cls[i][yq, xq])
            if on.any():
                found.update(zip(a[on].tolist(), b[on].tolist()))
        links.append(found)
    return _outputs(cls, region, sizes, kept, links, C, image_base)


def brute_groups64(maps, C, gap, min_pixels=1, image_base=0):
    cls, region, sizes, kept = _labelled(maps, C, min_pixels)
    n, h, w = cls.shape
    links = []
    for i in range(n):
        ys, xs = np.nonzero(kept[i])
        rid, kl = region[i][ys, xs], cls[i][ys, xs]
        d2 = (ys[:, None] - ys[None, :]) ** 2 + (xs[:, None] - xs[None, :]) ** 2
        on = (d2 <= gap * gap) & (rid[:, None] != rid[None, :]) & (kl[:, None] == kl[None, :])
        a, b = np.nonzero(on)
        links.append(set(zip(rid[a].tolist(), rid[b].tolist())))
    return _outputs(cls, region, sizes, kept, links, C, image_base)


def describe_groups(maps, C, gap, conf=None, min_pixels=1, image_base=0):
    """(one record of tests/_defects_ref.describe_records' 12 fields per group, sorted by (image, group root): the class
    of its fragments, the root of the group, the sums of the fragments' sizes, coordinate sums and conf_sum_q, the hull
    of their boxes and the largest conf_max_q; the fragment table)"""
    from _defects_ref import describe_records
    parts = describe_records(maps, C, conf, min_pixels, image_base)
    frag = group_regions64(maps, C, gap, min_pixels, image_base)[3]
    by_root = frag[np.lexsort((frag[:, 2], frag[:, 0]))]
    assert np.array_equal(by_root[:, [0, 1, 2, 4]], parts[:, :4])
    out = {}
    for f, p in zip(by_root.tolist(), parts.tolist()):
        g = out.setdefault((f[0], f[3]), [f[0], f[1], f[3], 0, p[4], p[5], p[6], p[7], 0, 0, 0, 0])
        g[3] += p[3]
        g[4], g[5], g[6], g[7] = min(g[4], p[4]), min(g[5], p[5]), max(g[6], p[6]), max(g[7], p[7])
        g[8] += p[8]; g[9] += p[9]; g[10] += p[10]
        g[11] = max(g[11], p[11])
    rec = np.array([out[k] for k in sorted(out)], np.int64).reshape(-1, 12)
    return rec, frag
