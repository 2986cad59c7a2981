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

import argparse
import json
import os
import sys

from . import seg_eval, seg_regions

DATASETS = ("gear", "kolektorsdd")
_NOT_HERE = ("--save_predictions", "--save_confusion_matrix", "--debug", "--debug_samples")
EXTRA_FLAGS = [("--min_region_pixels", dict(type=int, default=1)),
               ("--coverage_thresholds", dict(type=float, nargs="+", default=list(seg_regions.DEFAULT_THRESHOLDS)))]


def _cli(dataset):
    from . import eval_gear, eval_kolektorsdd
    return {"gear": eval_gear, "kolektorsdd": eval_kolektorsdd}[dataset]


def flags_of(dataset):
    return [(n, kw) for n, kw in _cli(dataset).FLAGS if n not in _NOT_HERE] + EXTRA_FLAGS


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    first = argparse.ArgumentParser(add_help=False)
    first.add_argument("--dataset", required=True, choices=DATASETS)
    dataset = first.parse_known_args(argv)[0].dataset          # its flags depend on the data set
    ap = argparse.ArgumentParser(description="Defect-level region metrics of a segmentation checkpoint (MI355X HIP path)")
    ap.add_argument("--dataset", required=True, choices=DATASETS)
    for name, kw in flags_of(dataset):
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    if args.min_region_pixels < 1:
        ap.error("--min_region_pixels must be at least 1")
    if any(not 0.0 <= t <= 1.0 for t in args.coverage_thresholds):
        ap.error("--coverage_thresholds must lie in 0..1")
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
    from .train_gear import build_seg_model, require_gpu
    from .utils import load_checkpoint

    device = require_gpu(args)
    cli = _cli(args.dataset)
    print("=" * 60 + f"\n{args.dataset.upper()} DATASET REGION EVALUATION\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nDataset: {args.split} split")
    os.makedirs(args.save_dir, exist_ok=True)
    loader, num_classes = cli._split_loader(args)
    class_names = cli._class_names(loader.dataset, num_classes)
    print(f"Number of classes: {num_classes}\nClass names: {class_names}\nSamples: {len(loader.dataset)}")
    model = build_seg_model(args, num_classes, device)
    epoch, loss = load_checkpoint(model, None, args.checkpoint, device)
    print(f"Loaded checkpoint from epoch {epoch} with loss {loss:.4f}")

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
