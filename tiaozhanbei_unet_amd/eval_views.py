#!/usr/bin/env python3
"""Does a view ensemble earn its cost?  ``eval_detection --tiled`` of a Gear checkpoint twice in one pass over the split
(no reference counterpart): once from the plain view alone, once from the views of ``--view_scales`` x ``--view_flips``
merged on the GPU (``views.ViewEnsemble``, csrc/views.hip), and the two sets of detection figures side by side.

    python -m tiaozhanbei_unet_amd.eval_views --dataset gear --checkpoint best_model.pth --data_root datasets/Gear \
        --tile 512 512 --view_scales 0.75 1 1.5 --view_flips h

Takes ``eval_detection``'s flags plus ``--view_scales`` and ``--view_flips`` (``predict_views``).  Tiled mode is implied,
so it is Gear only (KolektorSDD's masks are bitmaps, there is no full-resolution loader).  The plain view at scale 1 must
be among the views; it is moved to the front, and its logits, which the ensemble needs anyway, also give the single
prediction: exactly ``eval_detection --tiled``'s.  Both predictions feed an ``evaluation.DetectionMatcher`` each, and
``seg_detection.detection_results`` runs on each.

Writes ``{save_dir}/views_results.json``: evaluation_args, class_names, views, ``single`` and ``ensemble`` (each what
``detection_results.json`` holds: images, thresholds, region_confusion, panoptic), ``comparison`` {t: {single, ensemble}}
of average_precision, recall_within_false_alarm_budget, recall_at_best_f1, the two recommended min_confidence values and
panoptic_quality, and ``view_agreement``: at the first coverage threshold the mean over the ensemble's matched predicted
regions of their mean view agreement (the share of the views whose own label is the merged one) beside that of its false
alarms.  Prints the comparison as a two-column table.  The numbers describe the checkpoint given, on the split given.
"""
from __future__ import annotations

import json
import os

from . import eval_detection, seg_cli, seg_detection
from . import views as V
from .predict_views import VIEW_FLAGS, check_views

DATASETS = seg_cli.DATASETS


def flags_of(dataset):
    return eval_detection.flags_of(dataset) + VIEW_FLAGS


def _gear_flags(dataset):
    if dataset != "gear":
        raise ValueError("eval_views needs --dataset gear: KolektorSDD's masks are bitmaps, there is no full-resolution "
                         "loader")
    return flags_of(dataset)


def parse_args(argv=None):
    ap, args = seg_cli.parse_dataset_args(argv, "A view ensemble against the single view: detection figures of both "
                                                "(MI355X HIP path)", _gear_flags)
    args.tiled = True
    eval_detection.check_flags(ap, args)
    check_views(ap, args)
    plain = (1.0, 0, 0)
    if plain not in args.views:
        ap.error("--view_scales must hold 1: the plain view is the single prediction the ensemble is compared with")
    args.views = [plain] + [v for v in args.views if v != plain]
    return args


def match_views(ensemble, loader, num_classes, min_pixels, device):
    """One pass over a raw Gear loader, every image at its own size: (the matcher's result from the first view alone,
    the matcher's result from the ensemble, per predicted region of the latter its mean view agreement, the paths)."""
    import numpy as np
    import torch
    from .evaluation import DetectionMatcher, describe_class_regions
    from .sheets import seg_confidence
    single, merged = DetectionMatcher(num_classes, min_pixels), DetectionMatcher(num_classes, min_pixels)
    agree, all_paths, n_views = [], [], len(ensemble.views)
    flips = [(fx, fy) for _s, fx, fy in ensemble.views]
    with torch.no_grad():
        for image, mask, path in seg_cli.full_resolution_images(loader, device):
            frame_hw = (int(image.shape[0]), int(image.shape[1]))
            logits, _plan = ensemble.view_logits(image, frame_hw)
            labels, conf = seg_confidence(logits[0][None])
            single.update(labels, conf, mask[None])
            labels, conf, agreement = V.merge_views(logits, flips, frame_hw)
            base = merged.images
            merged.update(labels[None], conf[None], mask[None])
            agree.append(describe_class_regions(labels[None], num_classes, agreement[None].float() / float(n_views),
                                                min_pixels, image_base=base))
            all_paths.append(path)
    got = merged.compute()
    rec = np.concatenate(agree) if agree else np.zeros((0, 12), np.int64)
    if rec.shape != got["pred"].shape or (rec[:, :4] != got["pred"][:, :4]).any():
        raise RuntimeError("match_views: the agreement records are not those of the matcher's predicted regions")
    return single.compute(), got, seg_detection.region_scores(rec), all_paths


def compare(single, ensemble):
    """{threshold key: {"single": figures, "ensemble": figures}} of two ``seg_detection.detection_results``"""

    def figures(res, key):
        at = res["thresholds"][key]
        within, best = at["recommended"]["within_false_alarm_budget"], at["recommended"]["best_f1"]
        return {"average_precision": at["average_precision"]["overall"],
                "recall_within_false_alarm_budget": None if within is None else within["region_recall"],
                "recall_at_best_f1": None if best is None else best["region_recall"],
                "min_confidence_within_false_alarm_budget": None if within is None else within["min_confidence"],
                "min_confidence_at_best_f1": None if best is None else best["min_confidence"],
                "panoptic_quality": res["panoptic"]["overall"]["pq"]}

    return {key: {"single": figures(single, key), "ensemble": figures(ensemble, key)} for key in single["thresholds"]}


def agreement_summary(got, agreement, t):
    """the mean view agreement of the matched predicted regions and of the false alarms at the coverage ``t``"""
    matched = seg_detection.detection_scores(got["truth"], got["pred"], got["pairs"], t)["matched"]

    def mean(sel):
        return float(agreement[sel].mean()) if sel.any() else None

    return {"coverage_threshold": float(t), "matched_regions": int(matched.sum()), "matched_mean": mean(matched),
            "false_alarms": int((~matched).sum()), "false_alarm_mean": mean(~matched)}


def format_comparison(comparison, agreement, n_views):
    def cell(v):
        return f"{'none':>12}" if v is None else f"{v:>12.4f}"

    lines = [f"{'coverage':>8} {'figure':<42} {'single':>12} {f'{n_views} views':>12}"]
    for key, sides in comparison.items():
        for name in sides["single"]:
            lines.append(f"{key:>8} {name:<42} {cell(sides['single'][name])} {cell(sides['ensemble'][name])}")
    lines.append(f"Mean view agreement at coverage {agreement['coverage_threshold']}: matched regions "
                 f"({agreement['matched_regions']}) {cell(agreement['matched_mean']).strip()}, false alarms "
                 f"({agreement['false_alarms']}) {cell(agreement['false_alarm_mean']).strip()}")
    return "\n".join(lines)


def main(argv=None):
    args = parse_args(argv)

    device, _cli, loader, num_classes, class_names, model = seg_cli.open_checkpoint_session(args, "VIEW-ENSEMBLE EVALUATION")
    if not 2 <= num_classes <= 8:
        raise SystemExit(f"{num_classes} classes: the merge kernel takes 2 to 8")
    predictor = seg_cli.tiled_predictor(args, loader, model)
    print(f"Views: {len(args.views)} (scales {args.view_scales}, flips {args.view_flips})")
    ensemble = V.ViewEnsemble(predictor, args.views)
    got_single, got_merged, agreement, _paths = match_views(ensemble, loader, num_classes, args.min_region_pixels, device)

    sides = {}
    for name, got in (("single", got_single), ("ensemble", got_merged)):
        sides[name] = seg_detection.detection_results(got["truth"], got["pred"], got["pairs"], got["images"], num_classes,
                                                      args.coverage_thresholds, class_names, args.max_false_alarms)
    comparison = compare(sides["single"], sides["ensemble"])
    summary = agreement_summary(got_merged, agreement, args.coverage_thresholds[0])
    print(format_comparison(comparison, summary, len(args.views)))
    out_path = os.path.join(args.save_dir, "views_results.json")
    with open(out_path, "w") as f:
        json.dump({"evaluation_args": vars(args), "class_names": list(class_names), "min_region_pixels": args.min_region_pixels,
                   "views": [{"scale": s, "flip_x": bool(fx), "flip_y": bool(fy)} for s, fx, fy in args.views],
                   "single": sides["single"], "ensemble": sides["ensemble"], "comparison": comparison,
                   "view_agreement": summary}, f, indent=2)
    print(f"View-ensemble results saved to: {out_path}")
    return out_path


if __name__ == "__main__":
    main()
