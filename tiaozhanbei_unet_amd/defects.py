"""Host side of the ``predict`` CLI (no reference counterpart): which files to read, and what the per-defect records of
``evaluation.describe_class_regions`` say about every image.  numpy and the standard library only: importable and
testable without a GPU.

A record is one predicted class region of one image in the FRAME the model ran at (h x w); ``defect_entries`` restates
it per image, in the frame and in the image's own pixels (H0 x W0), and takes the accept / reject decision.  A frame
pixel x covers the image interval [x W0 / w, (x + 1) W0 / w): a box maps to the image pixels that its pixels touch
(integer arithmetic), a centroid by pixel centres, (c + 0.5) W0 / w - 0.5.

``shape_measures`` is the host geometry of ``evaluation.measure_class_regions``' integer shape records: area, equivalent
ellipse, Feret extents, perimeter and holes of a region, in the image's own pixels and, with a pixel size, in millimetres.
"""
from __future__ import annotations

import os

import numpy as np

IMAGE_EXTS = (".jpg", ".jpeg", ".png", ".bmp")
LABEL_SUFFIX = "_label.bmp"                              # KolektorSDD's ground truth beside its images: never an input
Q_ONE = 65536                                            # the fixed-point 1.0 of conf_sum_q / conf_max_q
FIELDS = ("image", "class", "root", "size", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "conf_sum_q", "conf_max_q")


def is_image(name):
    low = name.lower()
    return low.endswith(IMAGE_EXTS) and not low.endswith(LABEL_SUFFIX)


def list_images(path):
    """The image files of ``path``: the file itself, or every jpg / jpeg / png / bmp (any letter case) below the
    directory, walked recursively and sorted by path; names ending in ``_label.bmp`` are skipped."""
    if os.path.isfile(path):
        if not is_image(path):
            raise ValueError(f"{path} is not an image file ({', '.join(e[1:] for e in IMAGE_EXTS)})")
        return [path]
    if not os.path.isdir(path):
        raise ValueError(f"Input not found: {path}")
    found = []
    for folder, _dirs, names in os.walk(path):
        found.extend(os.path.join(folder, n) for n in names if is_image(n))
    return sorted(found)


def output_name(image_path, input_path):
    """The name of an image's output files: its path relative to a directory ``input_path`` without the extension, the
    separators replaced by ``__`` (two files of one stem in different folders stay apart); a single file's stem."""
    rel = os.path.relpath(image_path, input_path) if os.path.isdir(input_path) else os.path.basename(image_path)
    return os.path.splitext(rel)[0].replace(os.sep, "__")


def output_names(image_paths, input_path):
    """``output_name`` of every path, unique: ``a/b.png`` and ``a__b.png``, or ``x.png`` and ``x.jpg``, would collide, so
    a name that is taken gets its extension and then a counter appended."""
    names, taken = [], set()
    for p in image_paths:
        name = output_name(p, input_path)
        if name in taken:
            name += "_" + os.path.splitext(p)[1][1:].lower()
        stem, k = name, 1
        while name in taken:
            k += 1
            name = f"{stem}_{k}"
        taken.add(name)
        names.append(name)
    return names


def class_names_for(task_names, num_classes, given=None):
    """``num_classes`` names: the given ones or the task's, cut or extended with ``class_<i>``."""
    names = list(given if given else task_names)[:num_classes]
    return names + [f"class_{i}" for i in range(len(names), num_classes)]


def _scale_box(x0, y0, x1, y1, frame_hw, original_hw):
    (h, w), (h0, w0) = frame_hw, original_hw
    return [x0 * w0 // w, y0 * h0 // h, -(-(x1 + 1) * w0 // w) - 1, -(-(y1 + 1) * h0 // h) - 1]


SHAPE_HEAD = ("image", "root", "size", "sum_xx", "sum_yy", "sum_xy", "q1", "q2", "qd", "q3", "q4")
Q_DIRECTION = 1 << 14                                    # the fixed-point 1.0 of a direction vector


def direction_table(directions=32):
    """int32 [D, 2]: (c_k, s_k) = (rint(cos(pi k / D) 2^14), rint(sin(pi k / D) 2^14)), k = 0 .. D - 1: D directions over
    half a turn (an extent along u is the extent along -u).  The kernel and its reference project on these integers."""
    d = int(directions)
    if not 2 <= d <= 32 or d % 2:
        raise ValueError(f"direction_table: {directions} directions, an even number of 2..32 is supported")
    a = np.pi * np.arange(d, dtype=np.float64) / d
    return np.stack([np.rint(np.cos(a) * Q_DIRECTION), np.rint(np.sin(a) * Q_DIRECTION)], axis=1).astype(np.int32)


def shape_measures(shape_record, directions, frame_hw, original_hw, pixel_size=None, defect_record=None, components=1):
    """What a shape record of ``evaluation.measure_class_regions`` (SHAPE_HEAD, pmin_k, pmax_k) says about its region, as
    a dict.  ``directions``: D or the ``direction_table`` the record was made with; ``defect_record``: the aligned record
    of ``describe_class_regions`` (FIELDS; needed: the moments are central about its sum_x / size, sum_y / size);
    ``frame_hw`` (h, w): the frame the maps have; ``original_hw`` (H0, W0): the image's own size, so a frame pixel is
    sx = W0 / w by sy = H0 / h image pixels; ``pixel_size``: millimetres per image pixel, or None.

    ``area`` (frame pixels), ``area_original`` = size sx sy.
    ``major_axis``, ``minor_axis``, ``orientation_deg``, ``eccentricity``: the ellipse with the region's second central
        moments, in image pixels.  The moments are exact integers (size sum_xx - sum_x^2, ...) divided by size^2, plus
        1 / 12 per axis for the extent of a pixel, scaled by sx^2, sy^2, sx sy; axes = 4 sqrt(eigenvalue),
        orientation = atan2(2 mu_xy, mu_xx - mu_yy) / 2 with x to the right and y down.
    ``feret_length``, ``feret_width``, ``feret_angle_deg``: the largest and the smallest of the D extents
        (pmax_k - pmin_k + |c_k| + |s_k|) / hypot(c_k / sx, s_k / sy) in image pixels -- the extent of the union of the
        pixel squares, not of their centres; the denominator carries the anisotropic squeeze exactly, since the support
        function of a scaled set is the support function at the scaled direction -- and the angle atan2(s_k / sy,
        c_k / sx) of the largest.  With D directions the true maximum lies at most pi / 2D from a sampled one: the length
        is low by at most the factor cos(pi / 2D) (0.12 % at D = 32), the width high by up to length sin(pi / 2D) (4.9 %
        of the length at D = 32).  For thin defects ``minor_axis`` is therefore the robust width figure.
    ``perimeter_crack`` = q1 + q2 + q3 + 2 qd (member / non-member pixel edges), ``perimeter`` = q2 + (q1 + q3 + 2 qd) /
        sqrt 2 (Duda), both in frame pixels; ``perimeter_original`` = perimeter sx only where |sx / sy - 1| <= 1e-6, else
        None: these counts cannot be rescaled anisotropically.  ``circularity`` = 4 pi area / perimeter^2.
    ``euler_number`` = (q1 - q3 - 2 qd) / 4 (exact, 8-connectivity), ``holes`` = components - euler_number.
    ``components``: the 8-connected pieces the record was summed over: 1 for a region, the number of fragments for a group
        of ``evaluation.group_class_regions`` (a group's Euler number is its fragments minus its holes).  For such a
        group ``perimeter`` and ``perimeter_crack`` are the sums over the fragments, and ``circularity``, computed from
        that sum, is NOT a roundness: several round fragments score far below 1.  The moments and the Feret extents
        are those of the union of the fragments, which is what the length of a broken scratch is.
    With ``pixel_size``: ``feret_length_mm``, ``feret_width_mm``, ``major_axis_mm``, ``minor_axis_mm``,
        ``perimeter_original_mm`` (or None) and ``area_mm2``."""
    import math
    table = direction_table(directions) if np.ndim(directions) == 0 else np.asarray(directions, np.int64).reshape(-1, 2)
    d = len(table)
    components = int(components)
    if components < 1:
        raise ValueError(f"shape_measures: {components} components, at least 1")
    r = [int(v) for v in np.asarray(shape_record).reshape(-1)]
    if len(r) != len(SHAPE_HEAD) + 2 * d:
        raise ValueError(f"shape_measures: a record of {len(r)} fields, {len(SHAPE_HEAD) + 2 * d} go with {d} directions")
    if defect_record is None:
        raise ValueError("shape_measures: the aligned describe_class_regions record is needed for the centroid")
    dr = [int(v) for v in np.asarray(defect_record).reshape(-1)]
    image, root, size, sum_xx, sum_yy, sum_xy, q1, q2, qd, q3, q4 = r[:len(SHAPE_HEAD)]
    if len(dr) != len(FIELDS) or (dr[0], dr[2], dr[3]) != (image, root, size) or size < 1:
        raise ValueError("shape_measures: the two records are not of one region")
    sum_x, sum_y = dr[8], dr[9]
    (h, w), (h0, w0) = frame_hw, original_hw
    sx, sy = w0 / w, h0 / h
    n2 = size * size                                     # Python integers: nothing is cancelled in floating point
    mxx = ((size * sum_xx - sum_x * sum_x) / n2 + 1 / 12) * sx * sx
    myy = ((size * sum_yy - sum_y * sum_y) / n2 + 1 / 12) * sy * sy
    mxy = (size * sum_xy - sum_x * sum_y) / n2 * sx * sy
    mid, half = (mxx + myy) / 2, math.hypot((mxx - myy) / 2, mxy)
    big, small = mid + half, max(mid - half, 0.0)
    out = {"area": size, "area_original": size * sx * sy,
           "major_axis": 4 * math.sqrt(big), "minor_axis": 4 * math.sqrt(small),
           "orientation_deg": math.degrees(0.5 * math.atan2(2 * mxy, mxx - myy)),
           "eccentricity": math.sqrt(max(1 - small / big, 0.0))}
    pmin, pmax = r[len(SHAPE_HEAD):len(SHAPE_HEAD) + d], r[len(SHAPE_HEAD) + d:]
    extents = [(pmax[k] - pmin[k] + abs(int(c)) + abs(int(s))) / math.hypot(c / sx, s / sy)
               for k, (c, s) in enumerate(table.tolist())]
    longest = max(range(d), key=extents.__getitem__)
    out.update(feret_length=extents[longest], feret_width=min(extents),
               feret_angle_deg=math.degrees(math.atan2(table[longest][1] / sy, table[longest][0] / sx)))
    perimeter = q2 + (q1 + q3 + 2 * qd) / math.sqrt(2)
    euler, rest = divmod(q1 - q3 - 2 * qd, 4)
    if rest:
        raise ValueError("shape_measures: q1 - q3 - 2 qd is no multiple of 4: these are not the quads of a mask")
    out.update(perimeter_crack=q1 + q2 + q3 + 2 * qd, perimeter=perimeter,
               perimeter_original=perimeter * sx if abs(sx / sy - 1) <= 1e-6 else None,
               circularity=4 * math.pi * size / (perimeter * perimeter), euler_number=euler, holes=components - euler)
    if pixel_size is not None:
        mm = float(pixel_size)
        for key in ("feret_length", "feret_width", "major_axis", "minor_axis"):
            out[key + "_mm"] = out[key] * mm
        out["perimeter_original_mm"] = None if out["perimeter_original"] is None else out["perimeter_original"] * mm
        out["area_mm2"] = out["area_original"] * mm * mm
    return out


def size_rules(pixel_size=None, min_defect_length=0.0, min_defect_area=0.0):
    """The ``size_rules`` block of the predict tools: thresholds on ``feret_length`` and ``area_original``, in millimetres
    and mm^2 when ``pixel_size`` (mm per image pixel) is given and in image pixels otherwise."""
    mm = pixel_size is not None
    return {"units": {"length": "mm" if mm else "pixel", "area": "mm2" if mm else "pixel2"}, "pixel_size": pixel_size,
            "min_defect_length": float(min_defect_length), "min_defect_area": float(min_defect_area)}


def passes_size_rules(shape, rules):
    """whether a ``shape_measures`` dict is at least as long and as large as the ``size_rules`` ask"""
    mm = rules["pixel_size"] is not None
    return (shape["feret_length_mm" if mm else "feret_length"] >= rules["min_defect_length"]
            and shape["area_mm2" if mm else "area_original"] >= rules["min_defect_area"])


def defect_entries(records, class_names, frame_hw, original_hw_per_image, min_confidence=0.0, reject_classes=None,
                   shapes=None, rules=None, fragments=None):
    """Per-image dicts of the records [K, 12] (FIELDS; ``image`` indexes ``original_hw_per_image``, a list of (H0, W0)):
    ``{"defects": [...], "decision": "accept" | "reject"}``.  A defect holds ``class``, ``class_name``, ``pixels``, ``bbox``
    [x0, y0, x1, y1] in the frame (inclusive), ``bbox_original``, ``centroid`` [x, y], ``centroid_original``,
    ``mean_confidence`` = conf_sum_q / (65536 size), ``peak_confidence`` = conf_max_q / 65536 and ``counted`` =
    mean_confidence >= min_confidence.  The image is rejected iff it has a counted defect whose class name is in
    ``reject_classes`` (None: every class but class 0).

    ``shapes``: the aligned records of ``measure_class_regions`` (one per record, the same images and roots); every
    defect then holds ``shape`` = ``shape_measures`` of its record, and with ``rules`` (``size_rules``) ``counted``
    also requires ``passes_size_rules``.  Without ``shapes`` nothing is added.

    ``fragments``: the fragment table of ``describe_class_regions(..., merge_gap=g)`` ([F, 5]: image, class, root, group,
    size) when the records are groups.  Every defect then holds ``fragments``, a list of ``{"root": [x, y], "pixels": s}``
    in root order, and its ``shape`` is computed with that many components.  ``pixels``, ``bbox``, ``centroid`` and the
    confidences are those of the whole group; ``shape.perimeter`` is the sum over the fragments and
    ``shape.circularity`` of a defect of several fragments is not a roundness (``shape_measures``)."""
    rec = np.asarray(records, dtype=np.int64).reshape(-1, len(FIELDS))
    h, w = int(frame_hw[0]), int(frame_hw[1])
    reject = set(class_names[1:]) if reject_classes is None else set(reject_classes)
    out = [{"defects": [], "decision": "accept"} for _ in original_hw_per_image]
    rec = rec[np.lexsort((rec[:, 2], rec[:, 0]))]
    table = None
    if shapes is not None:
        shp = np.asarray(shapes, dtype=np.int64)
        if shp.ndim != 2 or len(shp) != len(rec):
            raise ValueError(f"defect_entries: {len(rec)} records and shape records of shape {shp.shape}")
        shp = shp[np.lexsort((shp[:, 1], shp[:, 0]))]
        table = direction_table((shp.shape[1] - len(SHAPE_HEAD)) // 2)
        pixel_size = None if rules is None else rules["pixel_size"]
    elif rules is not None:
        raise ValueError("defect_entries: size rules need the shape records")
    members = None
    if fragments is not None:
        members = {}
        frag = np.asarray(fragments, dtype=np.int64).reshape(-1, 5)
        for image, _cls, root, group, size in frag[np.lexsort((frag[:, 2], frag[:, 3], frag[:, 0]))].tolist():
            members.setdefault((image, group), []).append({"root": [root % w, root // w], "pixels": size})
        if sorted(members) != [(r[0], r[2]) for r in rec.tolist()]:
            raise ValueError("defect_entries: the fragment table is not the one of these records")
    for k, r in enumerate(rec.tolist()):
        image, cls, _root, size, x0, y0, x1, y1, sum_x, sum_y, conf_sum, conf_max = r
        if not 0 <= image < len(out):
            raise ValueError(f"defect_entries: a record of image {image}, {len(out)} images were given")
        h0, w0 = (int(v) for v in original_hw_per_image[image])
        name = class_names[cls] if 0 <= cls < len(class_names) else f"class_{cls}"
        cx, cy = sum_x / size, sum_y / size
        mean = conf_sum / (Q_ONE * size)
        counted = mean >= min_confidence
        extra = {}
        if members is not None:
            extra["fragments"] = members[(image, _root)]
        if table is not None:
            extra["shape"] = shape_measures(shp[k], table, (h, w), (h0, w0), pixel_size, defect_record=r,
                                            components=len(extra["fragments"]) if members is not None else 1)
            if rules is not None:
                counted = counted and passes_size_rules(extra["shape"], rules)
        out[image]["defects"].append({
            "class": cls, "class_name": name, "pixels": size, "bbox": [x0, y0, x1, y1],
            "bbox_original": _scale_box(x0, y0, x1, y1, (h, w), (h0, w0)), "centroid": [cx, cy],
            "centroid_original": [(cx + 0.5) * w0 / w - 0.5, (cy + 0.5) * h0 / h - 0.5],
            "mean_confidence": mean, "peak_confidence": conf_max / Q_ONE, "counted": bool(counted), **extra})
        if counted and name in reject:
            out[image]["decision"] = "reject"
    return out


def summarize(entries, class_names):
    """{"images", "rejected", "defects": {class name: count}} over the per-image entries (every listed defect)."""
    per_class = {name: 0 for name in class_names[1:]}
    for e in entries:
        for d in e["defects"]:
            per_class[d["class_name"]] = per_class.get(d["class_name"], 0) + 1
    return {"images": len(entries), "rejected": sum(e["decision"] == "reject" for e in entries), "defects": per_class}
