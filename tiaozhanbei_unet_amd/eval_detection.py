#!/usr/bin/env python3
"""Defect detection of a Gear or KolektorSDD segmentation checkpoint as a function of confidence (no reference
counterpart): recall, precision and false alarms per image for every ``--min_confidence`` that ``predict`` could be given,
the value to give it, defects found with the wrong class, and IoU-matched panoptic quality.

    python -m tiaozhanbei_unet_amd.eval_detection --dataset gear --checkpoint best_model.pth --data_root datasets/Gear
    python -m tiaozhanbei_unet_amd.eval_detection --dataset gear --checkpoint best_model.pth --tiled --tile 512 512
    python -m tiaozhanbei_unet_amd.eval_detection --dataset kolektorsdd --checkpoint best_model.pth

Takes ``eval_regions``' flags (``--min_region_pixels`` and ``--coverage_thresholds`` among them) plus
``--max_false_alarms``, ``--tiled``, ``--tile H W`` and ``--min_overlap``.

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

import argparse
import json
import os
import sys

from . import eval_regions, seg_detection

DATASETS = eval_regions.DATASETS
EXTRA_FLAGS = [("--max_false_alarms", dict(type=float, default=0.1,
                                           help="false alarms per image the recommended --min_confidence may cost")),
               ("--tiled", dict(action="store_true", help="Gear: predict every image at its own size, in tiles")),
               ("--tile", dict(type=int, nargs=2, default=None, metavar=("H", "W"), help="default: the frame flags")),
               ("--min_overlap", dict(type=int, default=64, help="pixels neighbouring tiles share at least"))]


def flags_of(dataset):
    return eval_regions.flags_of(dataset) + EXTRA_FLAGS


def frame_of(args):
    if args.dataset == "gear":
        return [args.image_size, args.image_size]
    return [args.image_height, args.image_width]


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    first = argparse.ArgumentParser(add_help=False)
    first.add_argument("--dataset", required=True, choices=DATASETS)
    dataset = first.parse_known_args(argv)[0].dataset          # its flags depend on the data set
    ap = argparse.ArgumentParser(description="Defect detection curves over confidence of a segmentation checkpoint "
                                             "(MI355X HIP path)")
    ap.add_argument("--dataset", required=True, choices=DATASETS)
    for name, kw in flags_of(dataset):
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    if args.min_region_pixels < 1:
        ap.error("--min_region_pixels must be at least 1")
    if any(not 0.0 <= t <= 1.0 for t in args.coverage_thresholds):
        ap.error("--coverage_thresholds must lie in 0..1")
    if not args.max_false_alarms >= 0.0:
        ap.error("--max_false_alarms must be at least 0")
    if args.tiled and dataset != "gear":
        ap.error("--tiled needs --dataset gear: KolektorSDD's masks are bitmaps, there is no full-resolution loader")
    if args.tile is None:
        args.tile = frame_of(args)
    if min(args.tile) < 1:
        ap.error("--tile sides must be positive")
    if args.min_overlap < 0 or (args.tiled and args.min_overlap >= min(args.tile)):
        ap.error("--min_overlap must be at least 0 and, with --tiled, smaller than both tile sides")
    return args


def match_frames(model, batches, num_classes, min_pixels):
    """Eval-mode pass over (images, masks, paths) device batches: the matcher's result and the paths."""
    import torch
    from .evaluation import DetectionMatcher
    from .sheets import seg_confidence
    model.eval()
    matcher, paths = DetectionMatcher(num_classes, min_pixels), []
    with torch.no_grad():
        for images, masks, batch_paths in batches:
            labels, conf = seg_confidence(model(images))
            matcher.update(labels, conf, masks)
            paths.extend(batch_paths)
    return matcher.compute(), paths


def match_tiled(predictor, loader, num_classes, min_pixels, device):
    """Every image of a raw Gear loader at its own size, the way ``predict_tiled`` predicts and
    ``train_gear_crops.validate_tiled`` validates: the matcher's result and the paths."""
    import torch
    from .augment import color_jitter_normalize_u8
    from .crops import full_resolution_masks
    from .evaluation import DetectionMatcher
    matcher, all_paths = DetectionMatcher(num_classes, min_pixels), []
    with torch.no_grad():
        for images, polys, sizes, paths in loader:
            masks = full_resolution_masks(polys, sizes, device=device)
            for i in range(len(sizes)):
                frame = color_jitter_normalize_u8(images[i].to(device, non_blocking=True).unsqueeze(0))[0]
                labels, conf, _plan = predictor(frame)
                matcher.update(labels.unsqueeze(0), conf.unsqueeze(0), masks[i].unsqueeze(0))
            all_paths.extend(paths)
    return matcher.compute(), all_paths


def main(argv=None):
    args = parse_args(argv)
    from .train_gear import build_seg_model, require_gpu
    from .utils import load_checkpoint

    device = require_gpu(args)
    cli = eval_regions._cli(args.dataset)
    mode = "tiled" if args.tiled else "frame"
    print("=" * 60 + f"\n{args.dataset.upper()} DATASET DETECTION EVALUATION ({mode})\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nDataset: {args.split} split")
    os.makedirs(args.save_dir, exist_ok=True)
    loader, num_classes = cli._split_loader(args)
    class_names = cli._class_names(loader.dataset, num_classes)
    print(f"Number of classes: {num_classes}\nClass names: {class_names}\nSamples: {len(loader.dataset)}")
    model = build_seg_model(args, num_classes, device)
    epoch, loss = load_checkpoint(model, None, args.checkpoint, device)
    print(f"Loaded checkpoint from epoch {epoch} with loss {loss:.4f}")

    if args.tiled:
        from .tiling import TiledPredictor
        from .train_gear_crops import check_image_sizes
        check_image_sizes([loader.dataset])
        print(f"Tile: {args.tile}  min overlap: {args.min_overlap}")
        predictor = TiledPredictor(model, args.tile, args.min_overlap, args.batch_size)
        got, paths = match_tiled(predictor, loader, num_classes, args.min_region_pixels, device)
    else:
        got, paths = match_frames(model, cli._batches(args, loader, device), num_classes, args.min_region_pixels)

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
                   "min_region_pixels": args.min_region_pixels, **results}, f, indent=2)
    with open(os.path.join(args.save_dir, "detection_regions.json"), "w") as f:
        json.dump(seg_detection.region_entries(got["truth"], got["pred"], got["pairs"], paths, class_names,
                                               got["image_sizes"], args.coverage_thresholds[0]), f, indent=2)
    print(f"Detection results saved to: {summary_path}")
    return summary_path


if __name__ == "__main__":
    main()
