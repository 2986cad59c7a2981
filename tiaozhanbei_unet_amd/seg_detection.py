"""Defect detection as a function of confidence, from the region records of ``evaluation.DetectionMatcher``: which
``--min_confidence`` to give ``predict``, which defects are found with the wrong class, IoU-matched panoptic quality.
Pure numpy on the host, importable without a GPU or the library; every count is an integer, every ratio one float64
division, and an empty denominator gives 0.0, never NaN.

``truth`` / ``pred`` are records of ``evaluation.DEFECT_FIELDS`` (image, class, root, size, box, coordinate sums,
conf_sum_q, conf_max_q), one per truth region and one per *kept* predicted region; ``pairs`` are records of
``evaluation.PAIR_FIELDS`` (image, truth_root, pred_root, overlap), one per truth region and kept predicted region of one
image that share a pixel, whatever their classes.  A region is named by (image, root).

The score of a predicted region is ``conf_sum_q / (65536 size)``: the ``mean_confidence`` of ``defects.defect_entries``,
the very number ``predict --min_confidence`` compares, so a threshold read off the curve means the same there.  At a
minimum confidence tau the predicted regions with score >= tau are kept.  A region counts at a coverage ``t`` by
``seg_regions.covered``'s rule, ``hit >= 1 and hit >= t * size`` in float64, where ``hit`` sums the overlaps with its
partners of its own class: a truth region over the kept predicted regions, a predicted region over ALL truth regions
(whether a predicted region is a false alarm does not depend on tau).
"""
from __future__ import annotations

import numpy as np

from .seg_regions import _ratio, threshold_key

IMAGE, CLASS, ROOT, SIZE = 0, 1, 2, 3
CONF_SUM = 10
Q_ONE = 65536                                            # the fixed-point 1.0 of conf_sum_q
P_IMAGE, P_TRUTH, P_PRED, P_OVERLAP = range(4)
FIGURE_KEYS = ("truth_regions", "detected", "region_recall", "pred_regions", "matched", "region_precision", "region_f1",
               "false_alarms_per_image")


def _defects(a):
    return np.asarray(a, dtype=np.int64).reshape(-1, 12)


def _pairs(a):
    return np.asarray(a, dtype=np.int64).reshape(-1, 4)


def region_scores(pred):
    """float64 per predicted region: conf_sum_q / (65536 size), the expression of ``defects.defect_entries``"""
    return np.array([int(r[CONF_SUM]) / (Q_ONE * int(r[SIZE])) for r in _defects(pred)], dtype=np.float64)


def _counts(hit, size, t):
    """seg_regions.covered's rule on integer arrays"""
    return (hit >= 1) & (hit.astype(np.float64) >= np.float64(t) * size.astype(np.float64))


def _join(truth, pred, pairs):
    """(row of the truth region, row of the predicted region) of every pair"""
    t_row = {(int(r[IMAGE]), int(r[ROOT])): i for i, r in enumerate(truth)}
    p_row = {(int(r[IMAGE]), int(r[ROOT])): i for i, r in enumerate(pred)}
    try:
        ti = np.array([t_row[(int(q[P_IMAGE]), int(q[P_TRUTH]))] for q in pairs], dtype=np.int64)
        pi = np.array([p_row[(int(q[P_IMAGE]), int(q[P_PRED]))] for q in pairs], dtype=np.int64)
    except KeyError as e:
        raise ValueError(f"a pair names the region (image, root) = {e.args[0]}, which has no record") from None
    return ti, pi


def detection_scores(truth, pred, pairs, t):
    """{"scores": float64 [Kp], "matched": bool [Kp], "d": [Kt] of float or None} at the coverage ``t``.  ``matched``:
    the predicted region's overlap summed over the truth regions of its class counts.  ``d``, the detection score of a
    truth region: the largest tau at which the overlap summed over the predicted regions of its class with score >= tau
    still counts -- its partners sorted by score, descending, equal scores entering together, the score at which the
    cumulative overlap first reaches the need; None if all of them together do not reach it.  The region is detected at
    tau iff d is not None and d >= tau."""
    truth, pred, pairs = _defects(truth), _defects(pred), _pairs(pairs)
    scores = region_scores(pred)
    ti, pi = _join(truth, pred, pairs)
    same = truth[ti, CLASS] == pred[pi, CLASS]
    ti, pi, overlap = ti[same], pi[same], pairs[same, P_OVERLAP]
    p_hit = np.zeros(len(pred), np.int64)
    np.add.at(p_hit, pi, overlap)
    matched = _counts(p_hit, pred[:, SIZE], t)
    d = [None] * len(truth)
    order = np.lexsort((-scores[pi], ti))                # by truth region, then by score descending
    ti, sc, overlap = ti[order], scores[pi][order], overlap[order]
    starts = np.flatnonzero(np.r_[True, ti[1:] != ti[:-1]]) if len(ti) else np.zeros(0, np.int64)
    for a, b in zip(starts, np.r_[starts[1:], len(ti)]):
        region = int(ti[a])
        size = truth[region:region + 1, SIZE]
        cum = np.cumsum(overlap[a:b])
        last = np.r_[sc[a + 1:b] != sc[a:b - 1], True]   # the last partner of every score: ties enter together
        ok = last & _counts(cum, np.broadcast_to(size, cum.shape), t)
        if ok.any():
            d[region] = float(sc[a:b][int(np.argmax(ok))])
    return {"scores": scores, "matched": matched, "d": d}


def _point(tau, d, scores, matched, t_images, p_images, images):
    """one operating point: seg_regions._figures' keys and arithmetic, min_confidence, image-level tp / fp / fn / tn"""
    kept = scores >= tau
    det, mat, n_pred = int((d >= tau).sum()), int((kept & matched).sum()), int(kept.sum())
    recall, precision = _ratio(det, len(d)), _ratio(mat, n_pred)
    t_img, p_img = np.zeros(images, bool), np.zeros(images, bool)
    t_img[t_images] = True
    p_img[p_images[kept]] = True
    return {"min_confidence": float(tau), "truth_regions": int(len(d)), "detected": det, "region_recall": recall,
            "pred_regions": n_pred, "matched": mat, "region_precision": precision,
            "region_f1": _ratio(2.0 * precision * recall, precision + recall),
            "false_alarms_per_image": _ratio(n_pred - mat, images),
            "tp": int((t_img & p_img).sum()), "fp": int((~t_img & p_img).sum()),
            "fn": int((t_img & ~p_img).sum()), "tn": int((~t_img & ~p_img).sum())}


def average_precision(points):
    """sum of (R_k - R_{k-1}) P_k over the points in descending min_confidence, R before the first = 0; no interpolation"""
    ap, before = 0.0, 0.0
    for p in sorted(points, key=lambda p: -p["min_confidence"]):
        ap += (p["region_recall"] - before) * p["region_precision"]
        before = p["region_recall"]
    return float(ap)


def detection_curve(truth, pred, pairs, images, num_classes, t, class_names=None):
    """The operating points at the coverage ``t``, one per tau in {0} and the distinct scores, ascending: {"overall":
    [point], "per_class": {name: [point]}, "average_precision": {"overall", "per_class": {name}}}.  A point holds
    ``min_confidence``, the keys of ``seg_regions``' figures (truth_regions, detected, region_recall, pred_regions,
    matched, region_precision, region_f1, false_alarms_per_image) over the predicted regions with score >= tau, and the
    image-level tp / fp / fn / tn: an image is predicted defective iff it has a predicted region with score >= tau,
    truly defective iff it has a truth region (per class: of that class).  Every list has the same taus."""
    truth, pred, images = _defects(truth), _defects(pred), int(images)
    got = detection_scores(truth, pred, pairs, t)
    scores, matched = got["scores"], got["matched"]
    d = np.array([-1.0 if v is None else v for v in got["d"]], dtype=np.float64)      # scores and taus are >= 0
    taus = sorted({0.0} | set(scores.tolist()))
    names = [class_names[c] if class_names is not None else f"class_{c}" for c in range(num_classes)]

    def curve(tm, pm):
        return [_point(tau, d[tm], scores[pm], matched[pm], truth[tm, IMAGE], pred[pm, IMAGE], images) for tau in taus]

    overall = curve(np.ones(len(truth), bool), np.ones(len(pred), bool))
    per_class = {names[c]: curve(truth[:, CLASS] == c, pred[:, CLASS] == c) for c in range(1, num_classes)}
    return {"overall": overall, "per_class": per_class,
            "average_precision": {"overall": average_precision(overall),
                                  "per_class": {n: average_precision(p) for n, p in per_class.items()}}}


def recommend(curve, max_false_alarms):
    """{"best_f1": the point of the largest region_f1 (ties: the smallest min_confidence), "within_false_alarm_budget":
    the point of the smallest min_confidence whose false_alarms_per_image <= max_false_alarms -- false alarms do not
    increase with tau, so that is the point of the highest recall within the budget -- or None}.  ``curve``: a list of
    points or ``detection_curve``'s result (its overall points)."""
    points = curve["overall"] if isinstance(curve, dict) else list(curve)
    points = sorted(points, key=lambda p: p["min_confidence"])
    best = None
    for p in points:
        if best is None or p["region_f1"] > best["region_f1"]:
            best = p
    within = next((p for p in points if p["false_alarms_per_image"] <= max_false_alarms), None)
    return {"best_f1": best, "within_false_alarm_budget": within}


def _iou(overlap, t_size, p_size):
    return overlap.astype(np.float64) / (t_size + p_size - overlap).astype(np.float64)


def best_partners(truth, pred, pairs):
    """Per truth region, over its partners of ANY class: (class of the predicted region with the largest overlap, ties
    to the smaller class and then the smaller root; 0 without a partner), (the largest IoU; 0.0 without a partner)."""
    truth, pred, pairs = _defects(truth), _defects(pred), _pairs(pairs)
    ti, pi = _join(truth, pred, pairs)
    best_class, best_iou = np.zeros(len(truth), np.int64), np.zeros(len(truth), np.float64)
    iou = _iou(pairs[:, P_OVERLAP], truth[ti, SIZE], pred[pi, SIZE])
    np.maximum.at(best_iou, ti, iou)
    order = np.lexsort((pred[pi, ROOT], pred[pi, CLASS], -pairs[:, P_OVERLAP], ti))
    ti, pi = ti[order], pi[order]
    first = np.r_[True, ti[1:] != ti[:-1]] if len(ti) else np.zeros(0, bool)
    best_class[ti[first]] = pred[pi[first], CLASS]
    return best_class, best_iou


def region_confusion(truth, pred, pairs, num_classes):
    """int64 [num_classes - 1, num_classes]: row c - 1 holds the truth regions of class c, column 0 those that no kept
    predicted region touches (``missed``), column k those whose largest-overlap partner has class k (``best_partners``).
    "Found with the wrong class" (off the diagonal) is apart from "not found" (column 0)."""
    truth = _defects(truth)
    best_class, _ = best_partners(truth, pred, pairs)
    m = np.zeros((num_classes - 1, num_classes), np.int64)
    ok = (truth[:, CLASS] >= 1) & (truth[:, CLASS] < num_classes) & (best_class < num_classes)
    np.add.at(m, (truth[ok, CLASS] - 1, best_class[ok]), 1)
    return m


def panoptic_quality(truth, pred, pairs, num_classes, class_names=None):
    """{"overall", "per_class": {name}} of {tp, fp, fn, sq, rq, pq}.  A pair is a true positive iff both regions have
    the same class and IoU = o / (|T| + |P| - o) > 0.5 (decided on integers: 3 o > |T| + |P|), which matches every region
    at most once; fp / fn: the kept predicted / the truth regions that are in no true positive.  sq = sum of the true
    positives' IoU / tp, rq = tp / (tp + fp / 2 + fn / 2), pq = sum IoU / (tp + fp / 2 + fn / 2) = sq rq.  ``overall``
    pools the counts and the IoU sums of the classes."""
    truth, pred, pairs = _defects(truth), _defects(pred), _pairs(pairs)
    ti, pi = _join(truth, pred, pairs)
    o, ts, ps = pairs[:, P_OVERLAP], truth[ti, SIZE], pred[pi, SIZE]
    tp_pair = (truth[ti, CLASS] == pred[pi, CLASS]) & (3 * o > ts + ps)
    iou = _iou(o, ts, ps)
    names = [class_names[c] if class_names is not None else f"class_{c}" for c in range(num_classes)]

    def figures(tp, n_truth, n_pred, iou_sum):
        fp, fn = n_pred - tp, n_truth - tp
        den = tp + 0.5 * fp + 0.5 * fn
        return {"tp": int(tp), "fp": int(fp), "fn": int(fn), "sq": _ratio(iou_sum, tp), "rq": _ratio(tp, den),
                "pq": _ratio(iou_sum, den)}

    per_class, total = {}, [0, 0, 0, 0.0]
    for c in range(1, num_classes):
        sel = tp_pair & (truth[ti, CLASS] == c)
        part = [int(sel.sum()), int((truth[:, CLASS] == c).sum()), int((pred[:, CLASS] == c).sum()), float(iou[sel].sum())]
        per_class[names[c]] = figures(*part)
        total = [a + b for a, b in zip(total, part)]
    return {"overall": figures(*total), "per_class": per_class}


def region_entries(truth, pred, pairs, image_paths, class_names, image_sizes, t):
    """The list of ``detection_regions.json``: every truth region (kind "truth": image path, class, root y / x in its own
    image's width, bbox, size, detection_score at the coverage ``t`` or null, best_overlap_class or null, best_iou), then
    every kept predicted region (kind "pred": image path, class, y / x, bbox, size, score, matched)."""
    truth, pred = _defects(truth), _defects(pred)
    got = detection_scores(truth, pred, pairs, t)
    best_class, best_iou = best_partners(truth, pred, pairs)

    def common(kind, r):
        width = int(image_sizes[int(r[IMAGE])][1])
        return {"kind": kind, "image_path": image_paths[int(r[IMAGE])], "class": class_names[int(r[CLASS])],
                "y": int(r[ROOT]) // width, "x": int(r[ROOT]) % width, "bbox": [int(v) for v in r[4:8]],
                "size": int(r[SIZE])}

    out = []
    for i, r in enumerate(truth):
        out.append({**common("truth", r), "detection_score": got["d"][i],
                    "best_overlap_class": class_names[int(best_class[i])] if best_class[i] else None,
                    "best_iou": float(best_iou[i])})
    for i, r in enumerate(pred):
        out.append({**common("pred", r), "score": float(got["scores"][i]), "matched": bool(got["matched"][i])})
    return out


def detection_results(truth, pred, pairs, images, num_classes, thresholds, class_names, max_false_alarms):
    """What ``detection_results.json`` holds besides the arguments, names and mode: per ``seg_regions.threshold_key(t)``
    the curve (``overall``, ``per_class``), ``average_precision`` and ``recommended``; ``region_confusion`` {"rows",
    "columns", "matrix"}; ``panoptic``; ``images``."""
    res = {"images": int(images), "thresholds": {}}
    for t in thresholds:
        curve = detection_curve(truth, pred, pairs, images, num_classes, t, class_names)
        res["thresholds"][threshold_key(t)] = {**curve, "recommended": recommend(curve, max_false_alarms)}
    res["region_confusion"] = {"rows": list(class_names[1:num_classes]),
                               "columns": ["missed"] + list(class_names[1:num_classes]),
                               "matrix": region_confusion(truth, pred, pairs, num_classes).tolist()}
    res["panoptic"] = panoptic_quality(truth, pred, pairs, num_classes, class_names)
    return res


def _spread(points, most):
    """at most ``most`` points of a curve, evenly spread, both ends among them"""
    if len(points) <= most:
        return list(points)
    idx = sorted({round(k * (len(points) - 1) / (most - 1)) for k in range(most)})
    return [points[i] for i in idx]


def format_table(results, class_names, max_rows=12):
    """The short table the CLI prints: per coverage threshold up to ``max_rows`` points of the overall curve, the
    average precision and the recommended points; then the region confusion and the panoptic quality."""
    head = (f"{'coverage':>8} {'min_conf':>9} {'defects':>8} {'found':>8} {'recall':>8} {'alarms':>8} {'matched':>8} "
            f"{'precision':>9} {'f1':>8} {'false/img':>9} {'img tp/fp/fn/tn':>16}")
    lines = [f"Images: {results['images']}", head]

    def row(key, p):
        return (f"{key:>8} {p['min_confidence']:>9.4f} {p['truth_regions']:>8} {p['detected']:>8} {p['region_recall']:>8.4f} "
                f"{p['pred_regions']:>8} {p['matched']:>8} {p['region_precision']:>9.4f} {p['region_f1']:>8.4f} "
                f"{p['false_alarms_per_image']:>9.3f} {p['tp']:>4}/{p['fp']}/{p['fn']}/{p['tn']}")

    for key, at in results["thresholds"].items():
        lines += [row(key, p) for p in _spread(at["overall"], max_rows)]
        lines.append(f"{key:>8} average precision {at['average_precision']['overall']:.4f}")
        for rule, p in at["recommended"].items():
            lines.append(f"{key:>8} {rule}: " + ("none" if p is None else
                         f"--min_confidence {p['min_confidence']:.6f} (recall {p['region_recall']:.4f}, precision "
                         f"{p['region_precision']:.4f}, {p['false_alarms_per_image']:.3f} false alarms per image)"))
    conf = results["region_confusion"]
    lines.append("Truth regions by the class of their largest-overlap predicted region:")
    lines.append(f"{'':<16} " + " ".join(f"{c:>12}" for c in conf["columns"]))
    for name, r in zip(conf["rows"], conf["matrix"]):
        lines.append(f"{name:<16} " + " ".join(f"{v:>12}" for v in r))
    lines.append(f"{'panoptic':<16} {'tp':>6} {'fp':>6} {'fn':>6} {'sq':>8} {'rq':>8} {'pq':>8}")
    pan = results["panoptic"]
    for name, f in [("all", pan["overall"])] + list(pan["per_class"].items()):
        lines.append(f"{name:<16} {f['tp']:>6} {f['fp']:>6} {f['fn']:>6} {f['sq']:>8.4f} {f['rq']:>8.4f} {f['pq']:>8.4f}")
    return "\n".join(lines)
