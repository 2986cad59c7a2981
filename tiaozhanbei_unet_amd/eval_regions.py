#!/usr/bin/env python3
"""Defect-level evaluation of a Gear or KolektorSDD segmentation checkpoint (no reference counterpart): how many
defects the model found, how many false alarms per image it raised, which parts it would have rejected.

    python -m tiaozhanbei_unet_amd.eval_regions --dataset gear --checkpoint best_model.pth --data_root datasets/Gear
    python -m tiaozhanbei_unet_amd.eval_regions --dataset kolektorsdd --checkpoint best_model.pth

Takes the flags of ``eval_gear`` / ``eval_kolektorsdd`` for data, model, split, batch, workers, device, precision and
save_dir, and uses their loaders, device preprocessing, class names and model construction.  Per batch: model forward,
``metrics.per_image_stats(labels=True)`` for the argmax map, ``evaluation.ClassRegionMatcher.update`` (csrc/segregions.hip:
8-connected regions per class of truth and prediction, and how many pixels of each the other map covers); everything
is read back once, after the last batch.  ``--min_region_pixels`` drops smaller predicted regions before anything is
counted; a region counts at a coverage threshold t iff it has a common pixel and ``hit >= t * size``
(seg_regions.py).  Writes ``{save_dir}/region_results.json`` (evaluation_args, class_names, images,
min_region_pixels, image_level, thresholds {t: {overall, per_class}}, mean_coverage) and
``{save_dir}/per_region_results.json`` (every truth region, then the false alarms at the first threshold).
"""
from __future__ import annotations

import json
import os

from . import seg_cli, seg_regions

DATASETS = seg_cli.DATASETS
EXTRA_FLAGS = [("--min_region_pixels", dict(type=int, default=1)),
               ("--coverage_thresholds", dict(type=float, nargs="+", default=list(seg_regions.DEFAULT_THRESHOLDS)))]


def flags_of(dataset):
    return seg_cli.base_flags(dataset) + EXTRA_FLAGS


def parse_args(argv=None):
    ap, args = seg_cli.parse_dataset_args(argv, "Defect-level region metrics of a segmentation checkpoint (MI355X HIP path)",
                                          flags_of)
    seg_cli.check_region_flags(ap, args)
    return args


def match(model, batches, num_classes, min_pixels):
    """Eval-mode pass over (images, masks, paths) device batches: the matcher's result, the paths, the frame width."""
    import torch
    from .metrics import per_image_stats
    from .evaluation import ClassRegionMatcher
    model.eval()
    matcher, paths, width = ClassRegionMatcher(num_classes, min_pixels), [], 1
    with torch.no_grad():
        for images, masks, batch_paths in batches:
            labels = per_image_stats(model(images), labels=True)["labels"]
            matcher.update(labels, masks)
            paths.extend(batch_paths)
            width = int(labels.shape[-1])
    return matcher.compute(), paths, width                      # the one read-back of the pass


def main(argv=None):
    args = parse_args(argv)
    device, cli, loader, num_classes, class_names, model = seg_cli.open_checkpoint_session(args, "REGION EVALUATION")

    got, paths, width = match(model, cli._batches(args, loader, device), num_classes, args.min_region_pixels)
    results = seg_regions.region_metrics(got["truth"], got["pred"], got["images"], num_classes,
                                         args.coverage_thresholds, class_names)
    print(seg_regions.format_table(results, class_names))
    summary_path = os.path.join(args.save_dir, "region_results.json")
    with open(summary_path, "w") as f:
        json.dump({"evaluation_args": vars(args), "class_names": list(class_names),
                   "min_region_pixels": args.min_region_pixels, **results}, f, indent=2)
    with open(os.path.join(args.save_dir, "per_region_results.json"), "w") as f:
        json.dump(seg_regions.region_entries(got["truth"], got["pred"], paths, class_names, width,
                                             args.coverage_thresholds[0]), f, indent=2)
    print(f"Region results saved to: {summary_path}")
    return summary_path


if __name__ == "__main__":
    main()
