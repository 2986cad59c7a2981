"""Class-overlap analysis of a Gear label set (reference analyze_class_overlaps.py), from device histograms.

The reference draws, for every polygon of every file, a full-resolution Pillow image, ORs the images per raw class and
then forms ``mask_a & mask_b`` and ``np.sum`` over full frames for every pair of classes.  Here a file travels to the
GPU as its parsed polygons only; ``augment.polygon_class_histogram`` (csrc/polygon.hip) returns, per file, how many
pixels carry each of the eight possible sets of raw classes, and every figure of the report is a sum of those bins:

    pixels of class c            = sum of hist[b] over b with bit c
    overlap of classes a and b   = sum of hist[m] over m with bits a and b
    triple overlap               = hist[7]
    after the priority rule      = background hist[0]; spalling (raw 1) bins with bit 1; pitting (raw 0) bins 1 and 5;
                                   scrape (raw 2) bin 4

``overlap_stats`` is that arithmetic in plain Python over per-file records and needs no GPU; ``scan`` reads the tree
(image headers and label text only, no pixel is decoded) and ``histograms`` runs the kernel in batches.

Differences from the reference, on purpose:
  - files are listed in sorted order, as ``gear_dataset.py`` does (the reference uses ``os.listdir`` order, so the order
    of its lists and the order in which pair keys first appear depend on the file system);
  - raw class ids outside 0..2 are dropped with one printed warning per file (the reference counts their pixels and then
    raises ``KeyError`` at their first overlap); a file left without a polygon is not counted;
  - a polygon of more than ``augment.POLY_MAX_VERTICES`` vertices, or an image wider than ``augment.POLY_MAX_WIDTH``,
    stops the run with an error that names the file, before anything is launched;
  - coverage is the polygon kernel's rule: equal to Pillow's except for a few pixels on the row of a vertex that a
    polygon visits twice (csrc/polygon.hip, "Known divergence");
  - no PNG charts: the 3 x 3 ``overlap_matrix`` of the ``device_extras`` block stands in for ``overlap_matrix.png``,
    and the bar chart's numbers are ``overlap_percentages`` and ``files_with_overlaps`` themselves;
  - the ``device_extras`` block is an addition (the overlap matrix, the triple overlap, the pixels per class after
    priority resolution and the polygon census that the reference's analyze_classes.py prints); the reference's blocks
    keep its layout.
"""
from __future__ import annotations

import os

from .gear_dataset import IMAGE_EXTS, RAW_TO_FINAL, flatten_polygons, parse_labelme_txt

CLASS_NAMES = {0: "pitting", 1: "spalling", 2: "scrape"}     # reference analyze_class_overlaps.py:67


def class_pixels(hist, c):
    """Pixels covered by raw class ``c`` in one file's 8-bin histogram."""
    return sum(int(hist[b]) for b in range(8) if b >> c & 1)


def pair_pixels(hist, a, b):
    """Pixels covered by raw classes ``a`` and ``b`` both."""
    return sum(int(hist[m]) for m in range(8) if m >> a & 1 and m >> b & 1)


def first_appearance(polys):
    """Raw class ids of parsed polygons in the order of their first polygon of 3 or more points."""
    order = []
    for cls, pts in polys:
        if len(pts) >= 3 and cls not in order:
            order.append(cls)
    return order


def overlap_stats(records):
    """The reference's ``calculate_overlaps`` result from per-file records ``(split, file name, class ids in order of
    first appearance, hist[8])``, with an optional fifth entry ``{class id: polygon instances}`` for the census.  Records
    whose class list is empty are files without a polygon: the reference does not count them.  Pair keys follow the
    reference: for classes first appearing in the order [a, b, ...] the pair is ``name[a]_vs_name[b]`` for position(a) <
    position(b), so ``pitting_vs_spalling`` and ``spalling_vs_pitting`` are different keys and accumulate separately."""
    total, overlap, files, detailed = {}, {}, {}, []
    n_files = n_overlap = triple = 0
    matrix = [[0] * 3 for _ in range(3)]
    after = {"background": 0, "pitting": 0, "spalling": 0, "scrape": 0}
    instances = {name: 0 for name in CLASS_NAMES.values()}
    for rec in records:
        split, name, order, hist = rec[:4]
        order = [int(c) for c in order]
        if not order:
            continue
        hist = [int(v) for v in hist]
        n_files += 1
        for c in order:
            total[c] = total.get(c, 0) + class_pixels(hist, c)
        has_overlap = False
        for i, a in enumerate(order):
            for b in order[i + 1:]:
                ov = pair_pixels(hist, a, b)
                if ov <= 0:
                    continue
                has_overlap = True
                key = f"{CLASS_NAMES[a]}_vs_{CLASS_NAMES[b]}"
                overlap[key] = overlap.get(key, 0) + ov
                files.setdefault(key, []).append(f"{split}/{name}")
                ta, tb = class_pixels(hist, a), class_pixels(hist, b)
                detailed.append({"file": f"{split}/{name}", "class_a": CLASS_NAMES[a], "class_b": CLASS_NAMES[b],
                                 "overlap_pixels": ov, "class_a_total": ta, "class_b_total": tb,
                                 "overlap_ratio_a": ov / ta if ta > 0 else 0, "overlap_ratio_b": ov / tb if tb > 0 else 0})
                matrix[a][b] += ov
                matrix[b][a] += ov
        n_overlap += has_overlap
        triple += hist[7]
        after["background"] += hist[0]
        after["pitting"] += hist[1] + hist[5]
        after["spalling"] += hist[2] + hist[3] + hist[6] + hist[7]
        after["scrape"] += hist[4]
        if len(rec) > 4:
            for c, k in rec[4].items():
                instances[CLASS_NAMES[int(c)]] += int(k)
    ids = {v: k for k, v in CLASS_NAMES.items()}
    pct = {}
    for key, ov in overlap.items():
        a_name, b_name = key.split("_vs_")
        ta, tb = total.get(ids[a_name], 0), total.get(ids[b_name], 0)
        if ta > 0:
            pct[f"{key}_pct_of_{a_name}"] = (ov / ta) * 100
        if tb > 0:
            pct[f"{key}_pct_of_{b_name}"] = (ov / tb) * 100
    return {
        "total_pixels_per_class": total,
        "overlap_pixels": overlap,
        "overlap_percentages": pct,
        "files_with_overlaps": files,
        "detailed_stats": detailed,
        "summary": {"total_files_processed": n_files, "files_with_any_overlap": n_overlap,
                    "percentage_files_with_overlap": (n_overlap / n_files * 100) if n_files > 0 else 0,
                    "class_names": dict(CLASS_NAMES),
                    "total_pixels_per_class_name": {CLASS_NAMES[k]: v for k, v in total.items()}},
        "device_extras": {"overlap_matrix": matrix, "triple_overlap_pixels": triple,
                          "pixels_per_class_after_priority": after, "polygon_instances_per_class": instances},
    }


def to_jsonable(stats):
    """``stats`` with every dict key a string, as ``overlap_analysis_detailed.json`` holds it."""
    if isinstance(stats, dict):
        return {str(k): to_jsonable(v) for k, v in stats.items()}
    if isinstance(stats, (list, tuple)):
        return [to_jsonable(v) for v in stats]
    return stats


def scan(root_dir, splits=("train", "val", "test")):
    """Per-file entries ``(split, file name, (h, w), polygons)`` of the splits' labelled images, in sorted order: the
    image header gives the size, the label text the polygons (``keep_partial`` parsing, raw classes outside 0..2
    dropped with a warning).  Raises ValueError, naming the file, for a polygon or an image the kernel cannot take."""
    from PIL import Image

    from .augment import POLY_MAX_VERTICES, POLY_MAX_WIDTH
    entries = []
    for split in splits:
        images_dir, labels_dir = os.path.join(root_dir, "images", split), os.path.join(root_dir, "labels", split)
        if not os.path.exists(images_dir) or not os.path.exists(labels_dir):
            print(f"Skipping {split} split - directories not found")
            continue
        for name in sorted(os.listdir(images_dir)):
            if not name.lower().endswith(IMAGE_EXTS):
                continue
            label = os.path.join(labels_dir, os.path.splitext(name)[0] + ".txt")
            if not os.path.exists(label):
                continue
            with Image.open(os.path.join(images_dir, name)) as im:
                w, h = im.size
            polys = parse_labelme_txt(label, w, h, keep_partial=True)
            unknown = sorted({cls for cls, _ in polys if cls not in RAW_TO_FINAL})
            if unknown:
                print(f"Warning: {label}: raw class ids {unknown} are not Gear classes; their polygons are dropped")
                polys = [(cls, pts) for cls, pts in polys if cls in RAW_TO_FINAL]
            big = [len(pts) for _, pts in polys if len(pts) > POLY_MAX_VERTICES]
            if big:
                raise ValueError(f"{label}: polygon of {max(big)} vertices; the GPU polygon kernel takes at most "
                                 f"{POLY_MAX_VERTICES} vertices per polygon")
            if polys and w > POLY_MAX_WIDTH:
                raise ValueError(f"{os.path.join(images_dir, name)}: {w} pixels wide; the GPU polygon kernel takes at "
                                 f"most {POLY_MAX_WIDTH}")
            entries.append((split, name, (h, w), polys))
    return entries


def histograms(entries, batch_size=32, device="cuda"):
    """Records for ``overlap_stats`` from ``scan`` entries: one ``polygon_class_histogram`` launch per ``batch_size``
    files that have a polygon (the others are not counted and need no launch)."""
    from .augment import polygon_class_histogram
    drawn = [e for e in entries if e[3]]
    records = []
    for i in range(0, len(drawn), max(int(batch_size), 1)):
        chunk = drawn[i:i + max(int(batch_size), 1)]
        hist = polygon_class_histogram(flatten_polygons([e[3] for e in chunk]), [e[2] for e in chunk], device=device)
        for (split, name, _, polys), row in zip(chunk, hist.cpu().tolist()):
            census = {}
            for cls, _ in polys:
                census[cls] = census.get(cls, 0) + 1
            records.append((split, name, first_appearance(polys), row, census))
    return records
