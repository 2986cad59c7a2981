#!/usr/bin/env python3
"""Outline accuracy of a Gear or KolektorSDD segmentation checkpoint (no reference counterpart): how well the predicted
defect outlines are PLACED, which pixel IoU (large regions swamp their borders) and a coverage threshold (0.5 is 0.5
whether the outline is 1 or 20 pixels off) do not say.

    python -m tiaozhanbei_unet_amd.eval_boundaries --dataset gear --checkpoint best_model.pth --data_root datasets/Gear
    python -m tiaozhanbei_unet_amd.eval_boundaries --dataset gear --checkpoint best_model.pth --tiled --tile 512 512
    python -m tiaozhanbei_unet_amd.eval_boundaries --dataset kolektorsdd --checkpoint best_model.pth

Takes the flags of ``eval_gear`` / ``eval_kolektorsdd`` that ``eval_regions`` takes, ``eval_detection``'s ``--tiled``,
``--tile H W`` and ``--min_overlap`` with the same rules, ``--boundary_tolerances`` (pixels, at most 4, default 1 2 4) and
``--boundary_width`` (the band of Boundary IoU in pixels; 0, the default: 2 % of each image's diagonal).

Frame mode (the default): ``eval_regions``' loaders, device preprocessing and model construction; per batch the model,
``sheets.seg_confidence`` for the argmax map, ``evaluation.BoundaryMatcher.update``.  Tiled mode (``--tiled``, Gear only):
every image at its own size through ``tiling.TiledPredictor``, the truth from ``crops.full_resolution_masks``, one update
per image, as ``eval_detection`` does it.  ``BoundaryMatcher`` (csrc/distance.hip) computes an exact squared Euclidean
distance transform of every class's boundary in truth and prediction and reduces the two to one record per (image,
class) and a pooled distance histogram; everything is read back once, after the last batch, and ``seg_boundaries`` does
the rest on the host (its docstring defines every figure and says where they differ from the published ones).

Writes ``{save_dir}/boundary_results.json`` (evaluation_args, class_names, images, mode, tolerances, band_width, overall,
per_class, unmatched) and ``{save_dir}/per_image_boundaries.json`` (one entry per image).  The dist_p50_* / dist_p95_*
keys are percentiles of the pooled histogram in WHOLE pixels (floor of the distance), and its last bin, 1024, is open: it
stands for every distance of 1024 pixels or more.  The numbers describe the checkpoint given, on the split given.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

from . import eval_detection, eval_regions, seg_boundaries

DATASETS = eval_regions.DATASETS
_TILE_FLAGS = ("--tiled", "--tile", "--min_overlap")
EXTRA_FLAGS = [(n, kw) for n, kw in eval_detection.EXTRA_FLAGS if n in _TILE_FLAGS] + [
    ("--boundary_tolerances", dict(type=int, nargs="+", default=[1, 2, 4], help="pixels; at most 4 values")),
    ("--boundary_width", dict(type=int, default=0, help="Boundary IoU's band in pixels; 0: 2 %% of the diagonal"))]


def flags_of(dataset):
    return [(n, kw) for n, kw in eval_regions._cli(dataset).FLAGS if n not in eval_regions._NOT_HERE] + EXTRA_FLAGS


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    first = argparse.ArgumentParser(add_help=False)
    first.add_argument("--dataset", required=True, choices=DATASETS)
    dataset = first.parse_known_args(argv)[0].dataset          # its flags depend on the data set
    ap = argparse.ArgumentParser(description="Outline accuracy of a segmentation checkpoint (MI355X HIP path)")
    ap.add_argument("--dataset", required=True, choices=DATASETS)
    for name, kw in flags_of(dataset):
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    if not 1 <= len(args.boundary_tolerances) <= 4 or any(not 0 <= t <= 4096 for t in args.boundary_tolerances):
        ap.error("--boundary_tolerances takes 1 to 4 values in 0..4096")
    if not 0 <= args.boundary_width <= 4096:
        ap.error("--boundary_width must lie in 0..4096")
    if args.tiled and dataset != "gear":
        ap.error("--tiled needs --dataset gear: KolektorSDD's masks are bitmaps, there is no full-resolution loader")
    if args.tile is None:
        args.tile = eval_detection.frame_of(args)
    if min(args.tile) < 1:
        ap.error("--tile sides must be positive")
    if args.min_overlap < 0 or (args.tiled and args.min_overlap >= min(args.tile)):
        ap.error("--min_overlap must be at least 0 and, with --tiled, smaller than both tile sides")
    return args


def match_frames(model, batches, num_classes, tolerances, band_width):
    """Eval-mode pass over (images, masks, paths) device batches: the matcher's result and the paths."""
    import torch
    from .evaluation import BoundaryMatcher
    from .sheets import seg_confidence
    model.eval()
    matcher, paths = BoundaryMatcher(num_classes, tolerances, band_width), []
    with torch.no_grad():
        for images, masks, batch_paths in batches:
            labels, _conf = seg_confidence(model(images))
            matcher.update(labels, masks)
            paths.extend(batch_paths)
    return matcher.compute(), paths                            # the one read-back of the pass


def match_tiled(predictor, loader, num_classes, tolerances, band_width, device):
    """Every image of a raw Gear loader at its own size, as ``eval_detection.match_tiled`` walks them."""
    import torch
    from .augment import color_jitter_normalize_u8
    from .crops import full_resolution_masks
    from .evaluation import BoundaryMatcher
    matcher, all_paths = BoundaryMatcher(num_classes, tolerances, band_width), []
    with torch.no_grad():
        for images, polys, sizes, paths in loader:
            masks = full_resolution_masks(polys, sizes, device=device)
            for i in range(len(sizes)):
                frame = color_jitter_normalize_u8(images[i].to(device, non_blocking=True).unsqueeze(0))[0]
                labels, _conf, _plan = predictor(frame)
                matcher.update(labels.unsqueeze(0), masks[i].unsqueeze(0))
            all_paths.extend(paths)
    return matcher.compute(), all_paths


def main(argv=None):
    args = parse_args(argv)
    from .train_gear import build_seg_model, require_gpu
    from .utils import load_checkpoint

    device = require_gpu(args)
    cli = eval_regions._cli(args.dataset)
    mode = "tiled" if args.tiled else "frame"
    print("=" * 60 + f"\n{args.dataset.upper()} DATASET BOUNDARY EVALUATION ({mode})\n" + "=" * 60)
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
        got, paths = match_tiled(predictor, loader, num_classes, args.boundary_tolerances, args.boundary_width, device)
    else:
        got, paths = match_frames(model, cli._batches(args, loader, device), num_classes, args.boundary_tolerances,
                                  args.boundary_width)

    results = seg_boundaries.boundary_results(got["records"], got["hist"], got["images"], num_classes,
                                              args.boundary_tolerances, class_names)
    print(seg_boundaries.format_table(results, class_names))
    summary_path = os.path.join(args.save_dir, "boundary_results.json")
    with open(summary_path, "w") as f:
        json.dump({"evaluation_args": vars(args), "class_names": list(class_names), "images": results["images"],
                   "mode": mode, "tolerances": results["tolerances"], "band_width": seg_boundaries.BAND_WIDTH_RULE,
                   "overall": results["overall"], "per_class": results["per_class"], "unmatched": results["unmatched"]},
                  f, indent=2)
    with open(os.path.join(args.save_dir, "per_image_boundaries.json"), "w") as f:
        json.dump(seg_boundaries.image_entries(got["records"], paths, class_names, args.boundary_tolerances,
                                               got["band_widths"]), f, indent=2)
    print(f"Boundary results saved to: {summary_path}")
    return summary_path


if __name__ == "__main__":
    main()
