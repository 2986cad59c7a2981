"""Outline accuracy of a segmentation checkpoint from the (image, class) records and the pooled distance histogram of
``evaluation.BoundaryMatcher``.  Pure numpy on the host; every count is an integer, every ratio one float64 division,
and an empty denominator gives 0.0, never NaN.

A record is one row of ``evaluation.BOUNDARY_FIELDS``.  Figures are micro-averaged: the counts are summed over the
records (all classes, or one class) before anything is divided.

    boundary precision / recall / F1 at a tolerance tau: p_near / p_boundary, t_near / t_boundary and their harmonic
        mean.  Boundary pixels whose class has no boundary in the other map of their image stay in the denominators: they
        are unmatched at every tolerance.
    boundary_iou: sum band_inter / sum band_union.
    mean_dist_pred_to_truth / mean_dist_truth_to_pred, in pixels: sum of dist_sum_q8 / 256 / matched boundary pixels, where
        a record's boundary pixels are matched iff the other map of that record has a boundary too; assd is the same ratio
        over both directions together (the average symmetric surface distance).
    hausdorff_mean / hausdorff_max: sqrt(max(p_dist_max_sq, t_dist_max_sq)) per record where both maps have a boundary,
        its mean and maximum over those records (``hausdorff_pairs`` of them).
    dist_p50_* / dist_p95_*: percentiles of the pooled histogram per direction.  They are WHOLE pixels (a bin holds the
        distances d with floor(d) = bin, the value reported is the bin), and the LAST bin, 1024, is open: it holds every
        distance of 1024 pixels or more.  None where no boundary pixel was matched.
    unmatched: records with a boundary on one side only, and the boundary pixels in them.

Where these differ from the published definitions: Boundary IoU (Cheng et al., CVPR 2021) takes the band by iterated
3 x 3 erosion, here it is the pixels of the class within a Euclidean distance of the class's boundary pixels; and the
frame edge is no boundary here (a region cut off by the frame has no outline there), while mask erosion treats the
outside of the frame as background.  Distances run between boundary PIXELS of the two maps, so two identical maps are at
distance 0.
"""
from __future__ import annotations

import math

import numpy as np

FIELDS = (("image", "class", "t_pixels", "p_pixels", "t_boundary", "p_boundary")
          + tuple(f"p_near{k}" for k in range(4)) + tuple(f"t_near{k}" for k in range(4))
          + ("band_inter", "band_union", "p_dist_sum_q8", "t_dist_sum_q8", "p_dist_max_sq", "t_dist_max_sq"))
F = {name: i for i, name in enumerate(FIELDS)}
LAST_BIN = 1024
BAND_WIDTH_RULE = "--boundary_width pixels; 0: max(1, round(0.02 * sqrt(H^2 + W^2))) of each image"


def _records(a):
    return np.asarray(a, dtype=np.int64).reshape(-1, len(FIELDS))


def _ratio(num, den):
    return float(num) / float(den) if den else 0.0


def _col(r, name):
    return r[:, F[name]]


def tolerance_key(tau):
    return str(int(tau))


def percentile_bin(hist, q):
    """The smallest bin whose cumulative count reaches q of the total (0 < q <= 1); None for an empty histogram."""
    h = np.asarray(hist, dtype=np.int64).reshape(-1)
    total = int(h.sum())
    if total == 0:
        return None
    need = max(1, math.ceil(q * total))
    return int(np.searchsorted(np.cumsum(h), need))


def _figures(r, hist2, tolerances):
    """r: records; hist2: int64 [2, 1025] pooled over the same classes"""
    tb, pb = _col(r, "t_boundary"), _col(r, "p_boundary")
    both = (tb > 0) & (pb > 0)
    out = {"records": int(len(r)), "truth_pixels": int(_col(r, "t_pixels").sum()),
           "pred_pixels": int(_col(r, "p_pixels").sum()), "truth_boundary": int(tb.sum()), "pred_boundary": int(pb.sum()),
           "tolerances": {}}
    for k, tau in enumerate(tolerances):
        precision = _ratio(_col(r, f"p_near{k}").sum(), pb.sum())
        recall = _ratio(_col(r, f"t_near{k}").sum(), tb.sum())
        out["tolerances"][tolerance_key(tau)] = {
            "pred_near": int(_col(r, f"p_near{k}").sum()), "truth_near": int(_col(r, f"t_near{k}").sum()),
            "boundary_precision": precision, "boundary_recall": recall,
            "boundary_f1": _ratio(2.0 * precision * recall, precision + recall)}
    out["band_inter"], out["band_union"] = int(_col(r, "band_inter").sum()), int(_col(r, "band_union").sum())
    out["boundary_iou"] = _ratio(out["band_inter"], out["band_union"])
    mp, mt = int(pb[both].sum()), int(tb[both].sum())
    sp, st = int(_col(r, "p_dist_sum_q8").sum()), int(_col(r, "t_dist_sum_q8").sum())
    out["matched_pred_boundary"], out["matched_truth_boundary"] = mp, mt
    out["mean_dist_pred_to_truth"] = _ratio(sp / 256.0, mp)
    out["mean_dist_truth_to_pred"] = _ratio(st / 256.0, mt)
    out["assd"] = _ratio((sp + st) / 256.0, mp + mt)
    hd = np.sqrt(np.maximum(_col(r, "p_dist_max_sq"), _col(r, "t_dist_max_sq"))[both].astype(np.float64))
    out["hausdorff_pairs"] = int(both.sum())
    out["hausdorff_mean"] = float(hd.mean()) if len(hd) else 0.0
    out["hausdorff_max"] = float(hd.max()) if len(hd) else 0.0
    for name, direction in (("pred_to_truth", 0), ("truth_to_pred", 1)):
        out[f"dist_p50_{name}"] = percentile_bin(hist2[direction], 0.5)
        out[f"dist_p95_{name}"] = percentile_bin(hist2[direction], 0.95)
    return out


def _unmatched(r):
    tb, pb = _col(r, "t_boundary"), _col(r, "p_boundary")
    t_only, p_only = (tb > 0) & (pb == 0), (pb > 0) & (tb == 0)
    return {"truth_only": {"records": int(t_only.sum()), "boundary_pixels": int(tb[t_only].sum())},
            "pred_only": {"records": int(p_only.sum()), "boundary_pixels": int(pb[p_only].sum())}}


def boundary_results(records, hist, images, num_classes, tolerances, class_names=None):
    """What ``boundary_results.json`` holds besides the arguments and names: ``images``, ``tolerances``, ``overall`` and
    ``per_class`` {name: ...} (the figures of the module docstring), ``unmatched`` {"overall", "per_class"}.  Classes
    1 .. num_classes - 1; ``class_names[c]`` names class c (default ``class_c``)."""
    r = _records(records)
    hist = np.asarray(hist, dtype=np.int64).reshape(num_classes - 1, 2, LAST_BIN + 1)
    tolerances = [int(t) for t in tolerances]
    names = [class_names[c] if class_names is not None else f"class_{c}" for c in range(num_classes)]
    by_class = [(names[c], r[_col(r, "class") == c], hist[c - 1]) for c in range(1, num_classes)]
    return {"images": int(images), "tolerances": tolerances,
            "overall": _figures(r, hist.sum(axis=0), tolerances),
            "per_class": {name: _figures(rc, hc, tolerances) for name, rc, hc in by_class},
            "unmatched": {"overall": _unmatched(r), "per_class": {name: _unmatched(rc) for name, rc, _ in by_class}}}


def image_entries(records, paths, class_names, tolerances, band_widths):
    """The list of ``per_image_boundaries.json``: one entry per image with its path, band width and, per class that has a
    pixel in either map, the record's counts, its boundary F1 per tolerance, Boundary IoU, mean distances and Hausdorff
    distance (None where one side has no boundary)."""
    r = _records(records)
    empty = np.zeros((2, LAST_BIN + 1), np.int64)
    entries = []
    for i, path in enumerate(paths):
        classes = {}
        for row in r[_col(r, "image") == i]:
            if row[F["t_pixels"]] == 0 and row[F["p_pixels"]] == 0:
                continue
            f = _figures(row[None], empty, tolerances)
            for key in ("records", "hausdorff_pairs", "hausdorff_mean", "dist_p50_pred_to_truth", "dist_p95_pred_to_truth",
                        "dist_p50_truth_to_pred", "dist_p95_truth_to_pred"):
                del f[key]
            f["hausdorff"] = f.pop("hausdorff_max") if row[F["t_boundary"]] and row[F["p_boundary"]] else None
            classes[class_names[int(row[F["class"]])]] = f
        entries.append({"image_path": path, "band_width": int(band_widths[i]), "classes": classes})
    return entries


def format_table(results, class_names):
    """The short table the CLI prints."""
    un = results["unmatched"]["overall"]
    lines = [f"Images: {results['images']}   outlines on one side only: truth {un['truth_only']['records']} "
             f"({un['truth_only']['boundary_pixels']} px), prediction {un['pred_only']['records']} "
             f"({un['pred_only']['boundary_pixels']} px)",
             f"{'class':<16} {'b-IoU':>7} {'ASSD':>8} {'p->t':>8} {'t->p':>8} {'HD mean':>8} {'HD max':>8} {'p95 p->t':>8} "
             f"{'p95 t->p':>8} " + " ".join(f"{'P@' + tolerance_key(t):>7} {'R@' + tolerance_key(t):>7} "
                                             f"{'F1@' + tolerance_key(t):>7}" for t in results["tolerances"])]

    def cell(v):
        return f"{'-':>8}" if v is None else f"{v:>8}"

    for name, f in [("all", results["overall"])] + [(n, results["per_class"][n]) for n in class_names[1:]]:
        at = " ".join(f"{a['boundary_precision']:>7.4f} {a['boundary_recall']:>7.4f} {a['boundary_f1']:>7.4f}"
                      for a in f["tolerances"].values())
        lines.append(f"{name:<16} {f['boundary_iou']:>7.4f} {f['assd']:>8.3f} {f['mean_dist_pred_to_truth']:>8.3f} "
                     f"{f['mean_dist_truth_to_pred']:>8.3f} {f['hausdorff_mean']:>8.3f} {f['hausdorff_max']:>8.3f} "
                     f"{cell(f['dist_p95_pred_to_truth'])} {cell(f['dist_p95_truth_to_pred'])} {at}")
    return "\n".join(lines)
