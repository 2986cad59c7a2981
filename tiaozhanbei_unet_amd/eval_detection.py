#!/usr/bin/env python3
"""Defect detection of a Gear or KolektorSDD segmentation checkpoint as a function of confidence (no reference
counterpart): recall, precision and false alarms per image for every ``--min_confidence`` that ``predict`` could be given,
the value to give it, defects found with the wrong class, and IoU-matched panoptic quality.

    python -m tiaozhanbei_unet_amd.eval_detection --dataset gear --checkpoint best_model.pth --data_root datasets/Gear
    python -m tiaozhanbei_unet_amd.eval_detection --dataset gear --checkpoint best_model.pth --tiled --tile 512 512
    python -m tiaozhanbei_unet_amd.eval_detection --dataset kolektorsdd --checkpoint best_model.pth

Takes ``eval_regions``' flags (``--min_region_pixels`` and ``--coverage_thresholds`` among them) plus
``--max_false_alarms``, ``--tiled``, ``--tile H W`` and ``--min_overlap``, and ``--merge_gap PX`` (2..32 frame pixels;
absent: off), with which the predicted regions of one class that come within PX pixels of each other are matched as
one defect (``evaluation.group_class_regions``; the truth regions stay as labelled).  Running the tool with and without
it is how to measure whether grouping changes the detection figures on a data set.

Frame mode (the default): ``eval_regions``' loaders, device preprocessing and model construction; per batch the model,
``sheets.seg_confidence`` for the argmax map and its confidence, ``evaluation.DetectionMatcher.update``.
Tiled mode (``--tiled``, Gear only: KolektorSDD's masks are bitmaps and have no full-resolution loader): every image of the
split is only normalised, at its own size, and run through ``tiling.TiledPredictor`` with tiles of ``--tile`` (default: the
frame flags) overlapping by ``--min_overlap``; the truth is ``crops.full_resolution_masks``; one update per image.

``DetectionMatcher`` (csrc/segregions.hip, defects.hip, regionpairs.hip) yields every truth region, every predicted
region of at least ``--min_region_pixels`` pixels with its mean confidence, and the overlap of every pair of them;
``seg_detection`` does the rest on the host.  Writes ``{save_dir}/detection_results.json`` (evaluation_args, class_names,
images, mode, min_region_pixels, thresholds {t: {overall, per_class, average_precision, recommended}},
region_confusion, panoptic) and ``{save_dir}/detection_regions.json`` (every truth region, then every kept predicted
region).  The numbers describe the checkpoint given, on the split given.
"""
from __future__ import annotations

import json
import os

from . import eval_regions, seg_cli, seg_detection

DATASETS = seg_cli.DATASETS
EXTRA_FLAGS = [("--max_false_alarms", dict(type=float, default=0.1,
                                           help="false alarms per image the recommended --min_confidence may cost")),
               *seg_cli.TILING_FLAGS]


def flags_of(dataset):
    return eval_regions.flags_of(dataset) + EXTRA_FLAGS


def check_flags(ap, args):
    """the refusals of this tool's own flags (``eval_views`` takes them too)"""
    seg_cli.check_region_flags(ap, args)
    if not args.max_false_alarms >= 0.0:
        ap.error("--max_false_alarms must be at least 0")
    seg_cli.check_tiling(ap, args)


def parse_args(argv=None):
    ap, args = seg_cli.parse_dataset_args(argv, "Defect detection curves over confidence of a segmentation checkpoint "
                                                "(MI355X HIP path)", lambda dataset: flags_of(dataset) + seg_cli.GROUP_FLAGS)
    check_flags(ap, args)
    seg_cli.check_group_flags(ap, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    from .evaluation import DetectionMatcher

    mode = seg_cli.mode_of(args)
    device, cli, loader, num_classes, class_names, model = seg_cli.open_checkpoint_session(args, "DETECTION EVALUATION",
                                                                                           mode)
    matcher, paths = DetectionMatcher(num_classes, args.min_region_pixels, getattr(args, "merge_gap", 0)), []
    for labels, conf, masks, batch_paths in seg_cli.labelled_predictions(args, cli, loader, model, device):
        matcher.update(labels, conf, masks)
        paths.extend(batch_paths)
    got = matcher.compute()

    results = seg_detection.detection_results(got["truth"], got["pred"], got["pairs"], got["images"], num_classes,
                                              args.coverage_thresholds, class_names, args.max_false_alarms)
    print(seg_detection.format_table(results, class_names))
    first = results["thresholds"][seg_detection.threshold_key(args.coverage_thresholds[0])]["recommended"]
    said = {k: ("none" if p is None else repr(p["min_confidence"])) for k, p in first.items()}
    print(f"Recommended --min_confidence at coverage {args.coverage_thresholds[0]}: best F1 {said['best_f1']}; within "
          f"{args.max_false_alarms} false alarms per image {said['within_false_alarm_budget']}")
    summary_path = os.path.join(args.save_dir, "detection_results.json")
    images = results.pop("images")
    with open(summary_path, "w") as f:
        json.dump({"evaluation_args": vars(args), "class_names": list(class_names), "images": images, "mode": mode,
                   "min_region_pixels": args.min_region_pixels,
                   **({"merge_gap": args.merge_gap} if hasattr(args, "merge_gap") else {}), **results}, f, indent=2)
    with open(os.path.join(args.save_dir, "detection_regions.json"), "w") as f:
        json.dump(seg_detection.region_entries(got["truth"], got["pred"], got["pairs"], paths, class_names,
                                               got["image_sizes"], args.coverage_thresholds[0]), f, indent=2)
    print(f"Detection results saved to: {summary_path}")
    return summary_path


if __name__ == "__main__":
    main()
