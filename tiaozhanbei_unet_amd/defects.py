"""Host side of the ``predict`` CLI (no reference counterpart): which files to read, and what the per-defect records of
``evaluation.describe_class_regions`` say about every image.  numpy and the standard library only: importable and
testable without a GPU.

A record is one predicted class region of one image in the FRAME the model ran at (h x w); ``defect_entries`` restates
it per image, in the frame and in the image's own pixels (H0 x W0), and takes the accept / reject decision.  A frame
pixel x covers the image interval [x W0 / w, (x + 1) W0 / w): a box maps to the image pixels that its pixels touch
(integer arithmetic), a centroid by pixel centres, (c + 0.5) W0 / w - 0.5.
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


def defect_entries(records, class_names, frame_hw, original_hw_per_image, min_confidence=0.0, reject_classes=None):
    """Per-image dicts of the records [K, 12] (FIELDS; ``image`` indexes ``original_hw_per_image``, a list of (H0, W0)):
    ``{"defects": [...], "decision": "accept" | "reject"}``.  A defect holds ``class``, ``class_name``, ``pixels``, ``bbox``
    [x0, y0, x1, y1] in the frame (inclusive), ``bbox_original``, ``centroid`` [x, y], ``centroid_original``,
    ``mean_confidence`` = conf_sum_q / (65536 size), ``peak_confidence`` = conf_max_q / 65536 and ``counted`` =
    mean_confidence >= min_confidence.  The image is rejected iff it has a counted defect whose class name is in
    ``reject_classes`` (None: every class but class 0)."""
    rec = np.asarray(records, dtype=np.int64).reshape(-1, len(FIELDS))
    h, w = int(frame_hw[0]), int(frame_hw[1])
    reject = set(class_names[1:]) if reject_classes is None else set(reject_classes)
    out = [{"defects": [], "decision": "accept"} for _ in original_hw_per_image]
    for r in rec[np.lexsort((rec[:, 2], rec[:, 0]))].tolist():
        image, cls, _root, size, x0, y0, x1, y1, sum_x, sum_y, conf_sum, conf_max = r
        if not 0 <= image < len(out):
            raise ValueError(f"defect_entries: a record of image {image}, {len(out)} images were given")
        h0, w0 = (int(v) for v in original_hw_per_image[image])
        name = class_names[cls] if 0 <= cls < len(class_names) else f"class_{cls}"
        cx, cy = sum_x / size, sum_y / size
        mean = conf_sum / (Q_ONE * size)
        counted = mean >= min_confidence
        out[image]["defects"].append({
            "class": cls, "class_name": name, "pixels": size, "bbox": [x0, y0, x1, y1],
            "bbox_original": _scale_box(x0, y0, x1, y1, (h, w), (h0, w0)), "centroid": [cx, cy],
            "centroid_original": [(cx + 0.5) * w0 / w - 0.5, (cy + 0.5) * h0 / h - 0.5],
            "mean_confidence": mean, "peak_confidence": conf_max / Q_ONE, "counted": bool(counted)})
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
