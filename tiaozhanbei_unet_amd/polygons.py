"""Predicted defects as Gear label polygons (no reference counterpart): the host side of ``evaluation.trace_class_regions``
(csrc/contours.hip).  numpy only; nothing here needs a GPU or the library.

``outlines`` groups the traced loops by region, ``simplify_closed`` thins an outline (Douglas-Peucker),
``gear_label_lines`` writes outlines in the format ``gear_dataset.parse_labelme_txt`` reads: one line per polygon,
``class_id x y x y ...`` with the coordinates divided by the frame's width and height.  A point is written at its pixel's
centre, ``(x + 0.5) / W``: the loader's ``int(v * W)`` then lands on ``x`` exactly at any width up to 16384 (six decimals
are off by at most 5e-7 * 16384 < 0.01 of a pixel), and the same line read at another image size lands on the pixel that
holds that centre.  Pillow's ``ImageDraw.polygon`` of an outer loop fills the region and its holes.

Two limits follow from the format, not from this code.  It has no holes: a hole is filled on the way back (the hole
loops are kept in ``predictions.json``).  And the loader resolves overlapping classes by priority (spalling > pitting >
scrape), not by nesting: a defect of a lower class inside the hole of a higher one is overwritten.
"""
from __future__ import annotations

import numpy as np


def outlines(loops, points, fragments=None):
    """{(image, root): (outer, holes)} of ``trace_class_regions``' (loops, points), in the loops' order: ``outer`` = the int32
    [K, 2] points (x, y) of the region's one loop with area2 > 0, ``holes`` = a list of those of its loops with area2 < 0,
    by leader.

    ``fragments``: the fragment table of ``describe_and_measure_class_regions(..., merge_gap=g)`` ([F, 5]: image, class,
    root, group, size) when the loops are those of the fragments of grouped defects.  The result is then keyed by
    (image, group root) and holds (outer, holes, fragment_outlines): ``outer`` = the outer loop of the group's largest
    fragment (ties: the smallest root), ``holes`` = the hole loops of all its fragments, ``fragment_outlines`` = every
    fragment's outer loop in root order."""
    loops = np.asarray(loops, np.int64).reshape(-1, 6)
    points = np.asarray(points, np.int32).reshape(-1, 2)
    out = {}
    for image, root, _leader, n, first, area2 in loops.tolist():
        pts = points[first:first + n]
        if len(pts) != n or n < 1 or area2 == 0:
            raise ValueError(f"outlines: loop of image {image}, root {root}: {n} points from {first}, area2 {area2}")
        outer, holes = out.setdefault((image, root), ([], []))
        (outer if area2 > 0 else holes).append(pts)
    for key, (outer, holes) in out.items():
        if len(outer) != 1:
            raise ValueError(f"outlines: region {key} has {len(outer)} outer loops")
        out[key] = (outer[0], holes)
    if fragments is None:
        return out
    frag = np.asarray(fragments, np.int64).reshape(-1, 5)
    frag = frag[np.lexsort((frag[:, 2], frag[:, 3], frag[:, 0]))]
    if sorted(out) != sorted((i, r) for i, r in frag[:, [0, 2]].tolist()):
        raise ValueError("outlines: the fragment table is not the one of these loops")
    grouped, largest = {}, {}
    for image, _cls, root, group, size in frag.tolist():
        outer, holes = out[(image, root)]
        lead, all_holes, pieces = grouped.get((image, group), (None, [], []))
        if size > largest.get((image, group), 0):                # in root order: a tie keeps the smaller root
            largest[(image, group)], lead = size, outer
        grouped[(image, group)] = (lead, all_holes + holes, pieces + [outer])
    return grouped


def _segment_distances(pts, a, b):
    """distances of the points [K, 2] (float64) from the segment a b"""
    ab = b - a
    t = np.clip(((pts - a) @ ab) / (ab @ ab), 0.0, 1.0) if (ab @ ab) > 0 else np.zeros(len(pts))
    return np.hypot(*(pts - (a + t[:, None] * ab)).T)


def _thin_chain(pts, lo, hi, tolerance, keep):
    """Douglas-Peucker on the open chain pts[lo .. hi]: marks the kept indices strictly between them"""
    stack = [(lo, hi)]
    while stack:
        i, j = stack.pop()
        if j - i < 2:
            continue
        d = _segment_distances(pts[i + 1:j], pts[i], pts[j])
        k = int(np.argmax(d))
        if d[k] > tolerance:
            keep[i + 1 + k] = True
            stack += [(i, i + 1 + k), (i + 1 + k, j)]


def simplify_closed(points, tolerance):
    """Douglas-Peucker on the closed polygon ``points`` [K, 2]: it is split at its first point (the leader's) and the
    point farthest from it, and each half is thinned as an open chain.  The result is a subsequence of the input that
    keeps those two points, and every dropped point lies within ``tolerance`` of it.  ``tolerance == 0`` (and fewer than
    4 points) returns the input."""
    pts = np.asarray(points)
    if tolerance < 0:
        raise ValueError(f"simplify_closed: tolerance {tolerance} is negative")
    if tolerance == 0 or len(pts) < 4:
        return pts
    f = pts.astype(np.float64)
    closed = np.concatenate([f, f[:1]])
    far = int(np.argmax(np.hypot(*(f - f[0]).T)))
    keep = np.zeros(len(closed), bool)
    keep[[0, far, len(f)]] = True
    _thin_chain(closed, 0, far, tolerance, keep)
    _thin_chain(closed, far, len(f), tolerance, keep)
    return pts[keep[:len(f)]]


def gear_label_lines(outer_loops, classes, frame_hw):
    """One Gear label line per outline: ``"{class - 1} x y x y ..."`` with ``(x + 0.5) / W`` and ``(y + 0.5) / H`` to six
    decimals.  ``outer_loops``: [K, 2] integer (x, y) arrays in a frame of ``frame_hw`` = (H, W); ``classes``: their final
    class ids (pitting 1, spalling 2, scrape 3: the file's ids are one less).  The loader drops polygons of fewer than 3
    points, so a shorter outline repeats points: A becomes A A A and A B becomes A B A."""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    lines = []
    for pts, cls in zip(outer_loops, classes):
        pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2).tolist()]
        if not pts or int(cls) < 1:
            raise ValueError(f"gear_label_lines: an outline of {len(pts)} points of class {cls}")
        if len(pts) < 3:
            pts = (pts + pts + pts)[:3]
        lines.append(f"{int(cls) - 1} " + " ".join(f"{(x + 0.5) / w:.6f} {(y + 0.5) / h:.6f}" for x, y in pts))
    return lines


def attach_outlines(entries, records, traced, frame_hw, original_hw_per_image, tolerance=0.0):
    """Adds to every defect of ``defects.defect_entries``' per-image ``entries`` (built from the same ``records``) its
    ``outline`` ([[x, y], ...] in frame pixels, thinned by ``simplify_closed`` with ``tolerance``), ``outline_original``
    (the pixel centres in the image's own pixels, as ``centroid_original``) and ``hole_outlines``.  ``traced``:
    ``outlines`` of the same maps with the records' ``min_pixels`` and image numbering.  Where that was made with a
    fragment table (grouped defects), ``outline`` is the largest fragment's and every defect gains ``fragment_outlines``,
    the outlines of all its fragments in root order, thinned alike."""
    rec = np.asarray(records, np.int64).reshape(-1, 12)
    rec = rec[np.lexsort((rec[:, 2], rec[:, 0]))]                # defect_entries' order
    h, w = int(frame_hw[0]), int(frame_hw[1])
    at = [0] * len(entries)
    for image, root in rec[:, [0, 2]].tolist():
        d = entries[image]["defects"][at[image]]
        at[image] += 1
        outer, holes, *pieces = traced[(image, root)]
        h0, w0 = (int(v) for v in original_hw_per_image[image])
        outer = simplify_closed(outer, tolerance)
        d["outline"] = outer.tolist()
        d["outline_original"] = [[(x + 0.5) * w0 / w - 0.5, (y + 0.5) * h0 / h - 0.5] for x, y in d["outline"]]
        d["hole_outlines"] = [simplify_closed(hole, tolerance).tolist() for hole in holes]
        if pieces:
            d["fragment_outlines"] = [simplify_closed(piece, tolerance).tolist() for piece in pieces[0]]
    return entries


def entry_label_lines(entry, frame_hw):
    """``gear_label_lines`` of an image entry's defects with ``"counted": true`` (after ``attach_outlines``); a grouped
    defect (one with ``fragment_outlines``) writes one line per fragment"""
    kept = [d for d in entry["defects"] if d["counted"]]
    loops = [(piece, d["class"]) for d in kept for piece in d.get("fragment_outlines", [d["outline"]])]
    return gear_label_lines([piece for piece, _ in loops], [cls for _, cls in loops], frame_hw)
