"""Defect-level figures of a segmentation checkpoint from the region records of ``evaluation.ClassRegionMatcher``: how many
defects were found, how many false alarms were raised per image, which parts would have been rejected.  Pure numpy on
the host; every count is an integer and every ratio one float64 division.

A record is (image, class, root index y * W + x, size, hit).  ``truth`` holds one record per ground-truth region,
``pred`` one per *kept* predicted region (the matcher drops predicted regions below ``min_pixels`` before it counts
anything).  At a coverage threshold ``t`` a region counts -- a truth region is *detected*, a predicted region is
*matched* -- iff ``hit >= 1 and hit >= t * size`` in float64: ``t = 0`` asks for one common pixel, not for none.
An empty denominator gives 0.0, never NaN.
"""
from __future__ import annotations

import numpy as np

IMAGE, CLASS, ROOT, SIZE, HIT = range(5)
DEFAULT_THRESHOLDS = (0.0, 0.25, 0.5)


def _records(a):
    a = np.asarray(a, dtype=np.int64)
    return a.reshape(-1, 5)


def _ratio(num, den):
    return float(num) / float(den) if den else 0.0


def covered(records, t):
    """bool per record: hit >= 1 and hit >= t * size (float64)"""
    r = _records(records)
    return (r[:, HIT] >= 1) & (r[:, HIT].astype(np.float64) >= np.float64(t) * r[:, SIZE].astype(np.float64))


def threshold_key(t):
    return repr(float(t))


def _figures(truth, pred, t, images):
    det, mat = int(covered(truth, t).sum()), int(covered(pred, t).sum())
    recall, precision = _ratio(det, len(truth)), _ratio(mat, len(pred))
    return {"truth_regions": int(len(truth)), "detected": det, "region_recall": recall,
            "pred_regions": int(len(pred)), "matched": mat, "region_precision": precision,
            "region_f1": _ratio(2.0 * precision * recall, precision + recall),
            "false_alarms_per_image": _ratio(len(pred) - mat, images)}


def _mean_coverage(truth):
    if not len(truth):
        return 0.0
    return float(np.mean(truth[:, HIT].astype(np.float64) / truth[:, SIZE].astype(np.float64)))


def region_metrics(truth, pred, images, num_classes, thresholds=DEFAULT_THRESHOLDS, class_names=None):
    """What ``region_results.json`` holds besides the arguments and names: ``image_level`` {tp, fp, fn, tn, precision,
    recall, accuracy} (an image is truly defective iff it has a truth region, predicted defective iff it has a kept
    predicted region), ``thresholds`` {repr(t): {"overall", "per_class": {name: ...}}} with truth_regions, detected,
    region_recall, pred_regions, matched, region_precision, region_f1 and false_alarms_per_image (unmatched kept
    predicted regions / images), ``mean_coverage`` {"overall", "per_class"}: the mean of hit / size over the truth
    regions, and ``images``.  Classes 1 .. num_classes - 1; ``class_names[c]`` names class c (default ``class_c``)."""
    truth, pred, images = _records(truth), _records(pred), int(images)
    names = [class_names[c] if class_names is not None else f"class_{c}" for c in range(num_classes)]
    by_class = [(names[c], truth[truth[:, CLASS] == c], pred[pred[:, CLASS] == c]) for c in range(1, num_classes)]
    t_img, p_img = np.zeros(images, bool), np.zeros(images, bool)
    t_img[truth[:, IMAGE]] = True
    p_img[pred[:, IMAGE]] = True
    tp, fp = int((t_img & p_img).sum()), int((~t_img & p_img).sum())
    fn, tn = int((t_img & ~p_img).sum()), int((~t_img & ~p_img).sum())
    return {
        "images": images,
        "image_level": {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "precision": _ratio(tp, tp + fp),
                        "recall": _ratio(tp, tp + fn), "accuracy": _ratio(tp + tn, images)},
        "thresholds": {threshold_key(t): {"overall": _figures(truth, pred, t, images),
                                          "per_class": {name: _figures(tr, pr, t, images) for name, tr, pr in by_class}}
                       for t in thresholds},
        "mean_coverage": {"overall": _mean_coverage(truth),
                          "per_class": {name: _mean_coverage(tr) for name, tr, _ in by_class}},
    }


def region_entries(truth, pred, image_paths, class_names, width, threshold):
    """The list of ``per_region_results.json``: one entry per truth region, then one per kept predicted region that is
    not matched at ``threshold`` (a false alarm), each with image path, class name, root y / x, size, hit, coverage."""
    truth, pred = _records(truth), _records(pred)

    def entry(kind, r):
        return {"kind": kind, "image_path": image_paths[int(r[IMAGE])], "class": class_names[int(r[CLASS])],
                "y": int(r[ROOT]) // int(width), "x": int(r[ROOT]) % int(width), "size": int(r[SIZE]),
                "hit": int(r[HIT]), "coverage": _ratio(int(r[HIT]), int(r[SIZE]))}

    return [entry("truth", r) for r in truth] + [entry("false_alarm", r) for r in pred[~covered(pred, threshold)]]


def format_table(results, class_names):
    """The short table the CLI prints."""
    il = results["image_level"]
    lines = [f"Images: {results['images']}   defective {il['tp'] + il['fn']}, rejected {il['tp'] + il['fp']} "
             f"(tp {il['tp']} fp {il['fp']} fn {il['fn']} tn {il['tn']})   precision {il['precision']:.4f} "
             f"recall {il['recall']:.4f} accuracy {il['accuracy']:.4f}",
             f"Mean coverage of the truth regions: {results['mean_coverage']['overall']:.4f}",
             f"{'coverage':>8} {'class':<16} {'defects':>8} {'found':>8} {'recall':>8} {'alarms':>8} {'matched':>8} "
             f"{'precision':>9} {'f1':>8} {'false/img':>9}"]
    for key, at in results["thresholds"].items():
        for name, f in [("all", at["overall"])] + [(n, at["per_class"][n]) for n in class_names[1:]]:
            lines.append(f"{key:>8} {name:<16} {f['truth_regions']:>8} {f['detected']:>8} {f['region_recall']:>8.4f} "
                         f"{f['pred_regions']:>8} {f['matched']:>8} {f['region_precision']:>9.4f} {f['region_f1']:>8.4f} "
                         f"{f['false_alarms_per_image']:>9.3f}")
    return "\n".join(lines)
