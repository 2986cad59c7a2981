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

import json
import os

from . import seg_boundaries, seg_cli

DATASETS = seg_cli.DATASETS
EXTRA_FLAGS = seg_cli.TILING_FLAGS + [
    ("--boundary_tolerances", dict(type=int, nargs="+", default=[1, 2, 4], help="pixels; at most 4 values")),
    ("--boundary_width", dict(type=int, default=0, help="Boundary IoU's band in pixels; 0: 2 %% of the diagonal"))]


def flags_of(dataset):
    return seg_cli.base_flags(dataset) + EXTRA_FLAGS


def parse_args(argv=None):
    ap, args = seg_cli.parse_dataset_args(argv, "Outline accuracy of a segmentation checkpoint (MI355X HIP path)", flags_of)
    if not 1 <= len(args.boundary_tolerances) <= 4 or any(not 0 <= t <= 4096 for t in args.boundary_tolerances):
        ap.error("--boundary_tolerances takes 1 to 4 values in 0..4096")
    if not 0 <= args.boundary_width <= 4096:
        ap.error("--boundary_width must lie in 0..4096")
    seg_cli.check_tiling(ap, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    from .evaluation import BoundaryMatcher

    mode = seg_cli.mode_of(args)
    device, cli, loader, num_classes, class_names, model = seg_cli.open_checkpoint_session(args, "BOUNDARY EVALUATION",
                                                                                           mode)
    matcher, paths = BoundaryMatcher(num_classes, args.boundary_tolerances, args.boundary_width), []
    for labels, _conf, masks, batch_paths in seg_cli.labelled_predictions(args, cli, loader, model, device):
        matcher.update(labels, masks)
        paths.extend(batch_paths)
    got = matcher.compute()                                    # the one read-back of the pass

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
