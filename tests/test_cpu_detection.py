"""CPU checks of the region-pair records and the detection curves: the numpy restatement of the pair kernel on
hand-drawn maps, the exports and host-side refusals of the new entry points, seg_detection.py on hand-built records and
against a brute-force recount through seg_regions._figures, and the eval_detection CLI's flags."""
import ctypes
import os
import re

import numpy as np
import pytest

import _region_pairs_ref as P
from tiaozhanbei_unet_amd import _lib, defects, eval_detection, eval_regions, evaluation, ops, seg_detection, seg_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unet_region_pair_bound", "unet_region_pairs_workspace", "unet_region_pairs")


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_hand_drawn_maps():
    truth = np.array([[[1, 1, 0, 0, 0],
                       [1, 1, 0, 2, 2],
                       [0, 0, 0, 2, 2]]], np.uint8)
    pred = np.array([[[1, 1, 1, 0, 0],
                      [0, 2, 0, 2, 1],
                      [0, 0, 0, 2, 1]]], np.uint8)
    # truth regions: root 0 (class 1), root 8 (class 2); predicted: root 0 (class 1), 6 (class 2), 8 (class 2), 9 (class 1)
    assert P.pairs_of_labels(truth, pred, 3).tolist() == [[0, 0, 0, 2], [0, 0, 6, 1], [0, 8, 8, 2], [0, 8, 9, 2]]
    assert P.pairs_of_labels(truth, pred, 3, image_base=7)[:, 0].tolist() == [7] * 4
    treg = np.array([[[1, 1, 0], [1, 0, 6]], [[1, 1, 0], [1, 0, 6]]])
    preg = np.array([[[0, 2, 2], [2, 2, 2]], [[1, 1, 1], [1, 1, 1]]])
    assert P.pairs(treg, preg).tolist() == [[0, 0, 1, 2], [0, 5, 1, 1], [1, 0, 0, 3], [1, 5, 0, 1]]
    assert P.pair_starts(treg, preg).tolist() == [3, 3]       # a pair starts again at x = 0 and after a pixel without one
    assert P.pairs(np.ones((1, 2, 2), int), np.zeros((1, 2, 2), int)).shape == (0, 4)
    for t, p in ((treg, preg), (preg, treg)):                 # the starts bound the distinct pairs of every image
        got = P.pairs(t, p)
        assert all(P.pair_starts(t, p)[i] >= (got[:, 0] == i).sum() for i in range(2))


# ------------------------------------------------------------------------------------------------ exports
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert handle.unet_abi_version() == 1
    makefile = open(os.path.join(ROOT, "tiaozhanbei_unet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bregionpairs\.hip\b", makefile, re.M)
    assert ops.pair_class_regions is evaluation.pair_class_regions
    assert ops.DetectionMatcher is evaluation.DetectionMatcher
    assert ops.PAIR_FIELDS is evaluation.PAIR_FIELDS == ("image", "truth_root", "pred_root", "overlap")


def test_workspace_query_and_refusals_on_the_host():
    """decided before anything reaches the device"""
    lib = _lib.lib()
    assert lib.unet_region_pairs_workspace(3, 1024) == 3 * 1024 * 12
    assert lib.unet_region_pairs_workspace(1, 1) == 16
    for n, cap in ((1, 0), (1, 3), (1, 1000), (1, -4), (65536, 16), (0, 16), (1, 1 << 31)):
        assert lib.unet_region_pairs_workspace(n, cap) == 0, (n, cap)
    dummy = ctypes.c_void_p(16)                        # only checked for NULL and alignment: refused before any use
    call = lambda n, h, w, cap, base=0, rcap=16, ws=1 << 40: lib.unet_region_pairs(          # noqa: E731
        dummy, dummy, n, h, w, cap, base, dummy, rcap, dummy, dummy, dummy, ws, None)
    for cap in (0, 3, 1000, -4):
        assert call(2, 8, 8, cap) == -1
        assert b"unet_region_pairs" in lib.unet_last_error() and b"power of two" in lib.unet_last_error()
    for n, h, w in ((65536, 1, 1), (2, 32768, 32768), (1, 1 << 16, 1 << 15)):
        assert call(n, h, w, 16) == -2, (n, h, w)
        assert b"unet_region_pairs:" in lib.unet_last_error()
        assert lib.unet_region_pair_bound(dummy, dummy, n, h, w, dummy, None) == -2
        assert b"unet_region_pair_bound:" in lib.unet_last_error()
    assert call(2, 8, 8, 1 << 31) == -2 and call(2, 8, 8, 16, base=(1 << 31) - 2) == -2
    assert call(2, 8, 8, 16, rcap=1 << 31) == -2
    assert call(0, 8, 8, 16) == -1 and call(2, 8, 8, 16, base=-1) == -1 and call(2, 8, 8, 16, rcap=-1) == -1
    assert call(2, 8, 8, 16, ws=2 * 16 * 12 - 1) == -3
    assert lib.unet_region_pairs(None, dummy, 2, 8, 8, 16, 0, dummy, 16, dummy, dummy, dummy, 1 << 40, None) == -1
    assert lib.unet_region_pair_bound(dummy, dummy, 2, 0, 8, dummy, None) == -1
    assert lib.unet_region_pair_bound(dummy, None, 2, 8, 8, dummy, None) == -1


# ------------------------------------------------------------------------------------------------ seg_detection
def _region(image, cls, root, size, score=0.0):
    """a DEFECT_FIELDS record; score * 65536 * size must be an integer"""
    q = score * 65536 * size
    assert q == int(q)
    return [image, cls, root, size, 0, 0, 0, 0, 0, 0, int(q), 0]


def _arr(rows, width):
    return np.array(rows, np.int64).reshape(-1, width)


def test_detection_score_of_a_region_under_two_predictions():
    truth = _arr([_region(0, 1, 5, 10)], 12)
    pred = _arr([_region(0, 1, 3, 6, 0.75), _region(0, 1, 40, 8, 0.5)], 12)
    pairs = _arr([[0, 5, 3, 4], [0, 5, 40, 3]], 4)
    want = {0.0: 0.75, 0.25: 0.75, 0.4: 0.75, 0.5: 0.5, 0.7: 0.5, 0.8: None, 1.0: None}      # needs 1, 2.5, 4, 5, 7, 8, 10
    for t, d in want.items():
        got = seg_detection.detection_scores(truth, pred, pairs, t)
        assert got["d"] == [d], t
        assert got["scores"].tolist() == [0.75, 0.5]
    got = seg_detection.detection_scores(truth, pred, pairs, 0.5)
    assert got["matched"].tolist() == [True, False]            # 4 of 6 pixels, 3 of 8
    # the order of the records and of the pairs does not matter
    again = seg_detection.detection_scores(truth, pred[::-1], pairs[::-1], 0.5)
    assert again["d"] == [0.5] and again["matched"].tolist() == [False, True]


def test_tied_scores_enter_together():
    truth = _arr([_region(0, 1, 5, 10), _region(1, 1, 0, 4)], 12)
    pred = _arr([_region(0, 1, 3, 6, 0.5), _region(0, 1, 40, 8, 0.5), _region(0, 1, 90, 8, 0.25),
                 _region(1, 1, 0, 4, 0.5)], 12)
    pairs = _arr([[0, 5, 3, 3], [0, 5, 40, 2], [0, 5, 90, 5], [1, 0, 0, 4]], 4)
    assert seg_detection.detection_scores(truth, pred, pairs, 0.5)["d"] == [0.5, 0.5]      # 3 + 2 reach 5 at 0.5
    assert seg_detection.detection_scores(truth, pred, pairs, 0.6)["d"] == [0.25, 0.5]
    curve = seg_detection.detection_curve(truth, pred, pairs, 2, 2, 0.5)["overall"]
    assert [p["min_confidence"] for p in curve] == [0.0, 0.25, 0.5]
    assert [p["detected"] for p in curve] == [2, 2, 2] and [p["pred_regions"] for p in curve] == [4, 4, 3]


def test_a_region_under_another_class_is_missed_but_has_a_class():
    truth = _arr([_region(0, 2, 5, 10), _region(0, 1, 50, 10), _region(0, 3, 70, 2)], 12)
    pred = _arr([_region(0, 1, 3, 12, 0.5), _region(0, 2, 48, 4, 0.5), _region(0, 1, 60, 4, 0.75)], 12)
    pairs = _arr([[0, 5, 3, 9], [0, 50, 48, 4], [0, 50, 60, 4]], 4)
    got = seg_detection.detection_scores(truth, pred, pairs, 0.0)
    assert got["d"] == [None, 0.75, None] and got["matched"].tolist() == [False, False, True]
    conf = seg_detection.region_confusion(truth, pred, pairs, 4)
    #                       missed 1  2  3
    assert conf.tolist() == [[0, 1, 0, 0],             # class 1: overlaps 4 and 4 tie, the smaller class wins
                             [0, 1, 0, 0],             # class 2: found, as class 1
                             [1, 0, 0, 0]]             # class 3: nothing touches it
    best_class, best_iou = seg_detection.best_partners(truth, pred, pairs)
    assert best_class.tolist() == [1, 1, 0] and best_iou.tolist() == [9 / 13, 4 / 10, 0.0]
    pred2 = _arr([_region(0, 2, 48, 4, 0.5), _region(0, 2, 60, 4, 0.75)], 12)       # a tie within a class: the smaller root
    entries = seg_detection.region_entries(truth[1:2], pred2, pairs[1:], ["a.png"], ["bg", "x", "y", "z"], [(10, 10)], 0.0)
    assert entries[0] == {"kind": "truth", "image_path": "a.png", "class": "x", "y": 5, "x": 0, "bbox": [0, 0, 0, 0],
                          "size": 10, "detection_score": None, "best_overlap_class": "y", "best_iou": 0.4}
    assert [e["kind"] for e in entries] == ["truth", "pred", "pred"] and entries[2]["score"] == 0.75
    with pytest.raises(ValueError, match="no record"):
        seg_detection.detection_scores(truth, pred[:1], pairs, 0.0)


def test_the_empty_cases():
    none12, none4 = np.zeros((0, 12), np.int64), np.zeros((0, 4), np.int64)
    zero = {"min_confidence": 0.0, "truth_regions": 0, "detected": 0, "region_recall": 0.0, "pred_regions": 0,
            "matched": 0, "region_precision": 0.0, "region_f1": 0.0, "false_alarms_per_image": 0.0,
            "tp": 0, "fp": 0, "fn": 0, "tn": 3}
    curve = seg_detection.detection_curve(none12, none12, none4, 3, 3, 0.5, ["bg", "a", "b"])
    assert curve["overall"] == [zero] and curve["per_class"] == {"a": [zero], "b": [zero]}
    assert curve["average_precision"] == {"overall": 0.0, "per_class": {"a": 0.0, "b": 0.0}}
    assert seg_detection.recommend(curve, 0.0) == {"best_f1": zero, "within_false_alarm_budget": zero}
    assert seg_detection.region_confusion(none12, none12, none4, 3).tolist() == [[0, 0, 0], [0, 0, 0]]
    pq = seg_detection.panoptic_quality(none12, none12, none4, 3)
    assert pq["overall"] == {"tp": 0, "fp": 0, "fn": 0, "sq": 0.0, "rq": 0.0, "pq": 0.0}
    truth = _arr([_region(1, 1, 0, 4)], 12)            # defects and no prediction; no images at all
    curve = seg_detection.detection_curve(truth, none12, none4, 3, 2, 0.0)
    assert curve["overall"] == [{**zero, "truth_regions": 1, "fn": 1, "tn": 2}]
    assert seg_detection.detection_scores(truth, none12, none4, 0.0)["d"] == [None]
    pred = _arr([_region(2, 1, 0, 4, 0.5)], 12)        # a prediction and no defect
    points = seg_detection.detection_curve(none12, pred, none4, 3, 2, 0.0)["overall"]
    assert [(p["min_confidence"], p["pred_regions"], p["false_alarms_per_image"], p["fp"]) for p in points] == \
        [(0.0, 1, 1 / 3, 1), (0.5, 1, 1 / 3, 1)]
    assert seg_detection.detection_curve(none12, none12, none4, 0, 2, 0.0)["overall"][0]["tn"] == 0
    assert "Images: 3" in seg_detection.format_table(
        seg_detection.detection_results(none12, none12, none4, 3, 3, [0.0, 0.5], ["bg", "a", "b"], 0.1), ["bg", "a", "b"])


def _random_records(seed, images=5, classes=4):
    """record sets as a matcher could give them: regions with distinct roots per image, kept predicted regions with
    scores k / 8 (many ties), pairs between regions of one image with overlaps that fit both regions"""
    rng = np.random.default_rng(seed)
    truth, pred, pairs = [], [], []
    for i in range(images):
        nt, npred = (int(v) for v in rng.integers(0, 6, 2))
        troots, proots = rng.choice(1000, nt, replace=False), rng.choice(1000, npred, replace=False)
        ts, ps = rng.integers(1, 40, nt), rng.integers(1, 40, npred)
        truth += [_region(i, int(rng.integers(1, classes)), int(r), int(s)) for r, s in zip(troots, ts)]
        pred += [_region(i, int(rng.integers(1, classes)), int(r), int(s), int(rng.integers(0, 9)) / 8)
                 for r, s in zip(proots, ps)]
        for a in range(nt):
            for b in range(npred):
                if rng.random() < 0.5:
                    pairs.append([i, int(troots[a]), int(proots[b]), int(rng.integers(1, min(ts[a], ps[b]) + 1))])
    truth, pred = _arr(truth, 12), _arr(pred, 12)
    order = lambda r: r[np.lexsort((r[:, 2], r[:, 0]))]      # noqa: E731
    return order(truth), order(pred), _arr(pairs, 4), images, classes


def _recount(truth, pred, pairs, tau, t, images, cls=None):
    """seg_regions._figures of the records a ClassRegionMatcher would give with the predicted regions below tau dropped"""
    scores = np.array([r[10] / (65536 * r[3]) for r in pred.tolist()])
    kept = {(r[0], r[2]) for r, s in zip(pred.tolist(), scores) if s >= tau}
    tcls = {(r[0], r[2]): r[1] for r in truth.tolist()}
    pcls = {(r[0], r[2]): r[1] for r in pred.tolist()}
    thit, phit = {k: 0 for k in tcls}, {k: 0 for k in kept}
    for image, tr, pr, o in pairs.tolist():
        if (image, pr) in kept and tcls[(image, tr)] == pcls[(image, pr)]:
            thit[(image, tr)] += o
            phit[(image, pr)] += o
    trec = [[r[0], r[1], r[2], r[3], thit[(r[0], r[2])]] for r in truth.tolist() if cls in (None, r[1])]
    prec = [[r[0], r[1], r[2], r[3], phit[(r[0], r[2])]] for r in pred.tolist()
            if (r[0], r[2]) in kept and cls in (None, r[1])]
    figures = seg_regions._figures(_arr(trec, 5), _arr(prec, 5), t, images)
    t_img = {r[0] for r in trec}
    p_img = {r[0] for r in prec}
    figures.update(tp=len(t_img & p_img), fp=len(p_img - t_img), fn=len(t_img - p_img),
                   tn=images - len(t_img | p_img), min_confidence=float(tau))
    return figures


@pytest.mark.parametrize("seed", range(6))
def test_curve_equals_a_brute_force_recount(seed):
    truth, pred, pairs, images, classes = _random_records(seed)
    names = ["bg", "a", "b", "c"]
    for t in (0.0, 0.25, 0.5, 1.0):
        curve = seg_detection.detection_curve(truth, pred, pairs, images, classes, t, names)
        scores = seg_detection.region_scores(pred)
        assert [p["min_confidence"] for p in curve["overall"]] == sorted({0.0} | set(scores.tolist()))
        for k, point in enumerate(curve["overall"]):
            tau = point["min_confidence"]
            assert point == _recount(truth, pred, pairs, tau, t, images), (t, tau)
            for c in range(1, classes):
                assert curve["per_class"][names[c]][k] == _recount(truth, pred, pairs, tau, t, images, c), (t, tau, c)
        # tau = 0 keeps everything: eval_regions' own arithmetic on the matcher's records
        whole = seg_regions.region_metrics(*_matcher_records(truth, pred, pairs), images, classes, [t], names)
        at = whole["thresholds"][seg_regions.threshold_key(t)]
        first = curve["overall"][0]
        assert {k: first[k] for k in seg_detection.FIGURE_KEYS} == at["overall"]
        assert {k: first[k] for k in ("tp", "fp", "fn", "tn")} == {k: whole["image_level"][k] for k in ("tp", "fp", "fn", "tn")}
        for series in [curve["overall"]] + list(curve["per_class"].values()):
            for a, b in zip(series, series[1:]):       # a higher threshold finds no more and raises no more alarms
                assert b["region_recall"] <= a["region_recall"] and b["detected"] <= a["detected"]
                assert b["false_alarms_per_image"] <= a["false_alarms_per_image"]
        ap, before = 0.0, 0.0
        for p in curve["overall"][::-1]:
            ap += (p["region_recall"] - before) * p["region_precision"]
            before = p["region_recall"]
        assert curve["average_precision"]["overall"] == ap


def _matcher_records(truth, pred, pairs):
    """the (image, class, root, size, hit) records of ClassRegionMatcher from the three record sets"""
    tcls = {(r[0], r[2]): r[1] for r in truth.tolist()}
    pcls = {(r[0], r[2]): r[1] for r in pred.tolist()}
    thit, phit = {k: 0 for k in tcls}, {k: 0 for k in pcls}
    for image, tr, pr, o in pairs.tolist():
        if tcls[(image, tr)] == pcls[(image, pr)]:
            thit[(image, tr)] += o
            phit[(image, pr)] += o
    return (_arr([[r[0], r[1], r[2], r[3], thit[(r[0], r[2])]] for r in truth.tolist()], 5),
            _arr([[r[0], r[1], r[2], r[3], phit[(r[0], r[2])]] for r in pred.tolist()], 5))


@pytest.mark.parametrize("seed", range(3))
def test_kept_set_is_what_predict_counts(seed):
    """defects.defect_entries(min_confidence = tau) counts the very regions the curve keeps at tau"""
    truth, pred, pairs, images, classes = _random_records(10 + seed)
    names = ["bg", "a", "b", "c"]
    scores = seg_detection.region_scores(pred)
    curve = seg_detection.detection_curve(truth, pred, pairs, images, classes, 0.0, names)["overall"]
    for point in curve:
        tau = point["min_confidence"]
        entries = defects.defect_entries(pred, names, (100, 10), [(100, 10)] * images, min_confidence=tau)
        counted = [d["counted"] for e in entries for d in e["defects"]]           # by (image, root), as pred is
        assert counted == (scores >= tau).tolist()
        assert [d["mean_confidence"] for e in entries for d in e["defects"]] == scores.tolist()
        assert sum(counted) == point["pred_regions"]
        rejected = sum(e["decision"] == "reject" for e in entries)
        assert rejected == point["tp"] + point["fp"]   # predict's accept / reject decision is the image-level count


def test_recommend_rules():
    def point(tau, f1, alarms):
        return {"min_confidence": tau, "region_f1": f1, "false_alarms_per_image": alarms}
    curve = [point(0.0, 0.2, 3.0), point(0.3, 0.6, 1.0), point(0.5, 0.6, 0.1), point(0.7, 0.4, 0.1), point(0.9, 0.1, 0.0)]
    got = seg_detection.recommend(curve[::-1], 0.1)
    assert got["best_f1"] is curve[1]                  # the tie goes to the smaller threshold
    assert got["within_false_alarm_budget"] is curve[2]       # the smallest threshold within the budget
    assert seg_detection.recommend(curve, 0.0)["within_false_alarm_budget"] is curve[4]
    assert seg_detection.recommend(curve[:2], 0.5)["within_false_alarm_budget"] is None
    assert seg_detection.recommend({"overall": curve}, 5.0)["within_false_alarm_budget"] is curve[0]


def test_panoptic_quality_by_hand():
    truth = _arr([_region(0, 1, 0, 10), _region(0, 1, 50, 6), _region(1, 2, 7, 4)], 12)
    pred = _arr([_region(0, 1, 1, 10, 0.5), _region(0, 1, 52, 6, 0.5), _region(1, 1, 7, 4, 0.5)], 12)
    pairs = _arr([[0, 0, 1, 8],                        # IoU 8 / 12: a true positive
                  [0, 50, 52, 3],                      # IoU 3 / 9: none
                  [1, 7, 7, 4]], 4)                    # IoU 1 and another class: none
    got = seg_detection.panoptic_quality(truth, pred, pairs, 3, ["bg", "a", "b"])
    assert got["per_class"]["a"] == {"tp": 1, "fp": 2, "fn": 1, "sq": 8 / 12, "rq": 1 / 2.5, "pq": (8 / 12) / 2.5}
    assert got["per_class"]["b"] == {"tp": 0, "fp": 0, "fn": 1, "sq": 0.0, "rq": 0.0, "pq": 0.0}
    assert got["overall"] == {"tp": 1, "fp": 2, "fn": 2, "sq": 8 / 12, "rq": 1 / 3.0, "pq": (8 / 12) / 3.0}
    half = seg_detection.panoptic_quality(_arr([_region(0, 1, 0, 4)], 12), _arr([_region(0, 1, 0, 4, 0.5)], 12),
                                          _arr([[0, 0, 0, 2]], 4), 2)           # IoU 2 / 6; 4 of 8 would be 1 / 2 exactly
    assert half["overall"]["tp"] == 0
    exact = seg_detection.panoptic_quality(_arr([_region(0, 1, 0, 3)], 12), _arr([_region(0, 1, 0, 3, 0.5)], 12),
                                           _arr([[0, 0, 0, 2]], 4), 2)          # IoU 2 / 4: not above one half
    assert exact["overall"] == {"tp": 0, "fp": 1, "fn": 1, "sq": 0.0, "rq": 0.0, "pq": 0.0}


# ------------------------------------------------------------------------------------------------ CLI
def test_parse_args_defaults_and_refusals(capsys):
    args = eval_detection.parse_args(["--dataset", "gear", "--checkpoint", "m.pth"])
    assert (args.max_false_alarms, args.tiled, args.tile, args.min_overlap) == (0.1, False, [512, 512], 64)
    assert args.min_region_pixels == 1 and args.coverage_thresholds == list(seg_regions.DEFAULT_THRESHOLDS)
    args = eval_detection.parse_args(["--dataset", "kolektorsdd", "--checkpoint", "m.pth"])
    assert args.tile == [1024, 512] and not args.tiled
    args = eval_detection.parse_args(["--dataset", "gear", "--checkpoint", "m.pth", "--tiled", "--tile", "64", "96",
                                      "--min_overlap", "8", "--max_false_alarms", "0"])
    assert (args.tiled, args.tile, args.min_overlap, args.max_false_alarms) == (True, [64, 96], 8, 0.0)
    args = eval_detection.parse_args(["--dataset", "gear", "--checkpoint", "m.pth", "--image_size", "32"])
    assert args.tile == [32, 32] and args.min_overlap == 64        # the overlap only binds with --tiled
    for dataset in eval_regions.DATASETS:
        names = [n for n, _ in eval_detection.flags_of(dataset)]
        assert names == [n for n, _ in eval_regions.flags_of(dataset)] + ["--max_false_alarms", "--tiled", "--tile",
                                                                            "--min_overlap"]
    for bad in (["--dataset", "kolektorsdd", "--checkpoint", "m.pth", "--tiled"],
                ["--dataset", "gear", "--checkpoint", "m.pth", "--max_false_alarms", "-0.5"],
                ["--dataset", "gear", "--checkpoint", "m.pth", "--tiled", "--tile", "64", "64", "--min_overlap", "64"],
                ["--dataset", "gear", "--checkpoint", "m.pth", "--min_overlap", "-1"],
                ["--dataset", "gear", "--checkpoint", "m.pth", "--min_region_pixels", "0"]):
        with pytest.raises(SystemExit):
            eval_detection.parse_args(bad)
    assert "full-resolution" in capsys.readouterr().err


def test_eval_detection_refuses_cpu():
    with pytest.raises(SystemExit) as e:
        eval_detection.main(["--dataset", "gear", "--checkpoint", "m.pth", "--device", "cpu"])
    assert "no CPU path" in str(e.value)
