#!/usr/bin/env python3
"""Calibration of the per-pixel confidence of a Gear or KolektorSDD segmentation checkpoint (no reference counterpart):
reliability diagram, ECE, MCE and NLL of the softmax maximum that ``predict --min_confidence`` thresholds, and the one
temperature T that minimises the NLL of softmax(logits / T).

    python -m tiaozhanbei_unet_amd.eval_calibration --dataset gear --checkpoint best_model.pth --split val \\
        --save_calibrated best_model_calibrated.pth
    python -m tiaozhanbei_unet_amd.eval_calibration --dataset gear --checkpoint best_model.pth --tiled --tile 512 512
    python -m tiaozhanbei_unet_amd.eval_calibration --dataset kolektorsdd --checkpoint best_model.pth

Takes ``eval_regions``' flags for data, model, split, batch, workers, device, precision and save_dir, ``eval_detection``'s
``--tiled``, ``--tile H W`` and ``--min_overlap`` (same refusals), plus ``--bins``, ``--temperature_range LO HI``,
``--temperature_steps``, ``--fit_on {all,defects}`` and ``--save_calibrated OUT.pth``.

Two passes over the split with ``evaluation.CalibrationMeter`` (csrc/calibration.hip), each read back once.  Pass 1: the
histogram at T = 1 and the NLL at every temperature of the grid; ``seg_calibration.fit_temperature`` then picks T on the
host.  Pass 2: the histogram at T and the NLL at T itself.  Tiled mode (Gear only) takes the blended logits of
``tiling.TiledPredictor.blended_logits`` at every image's own size.  Writes ``{save_dir}/calibration_results.json``
(evaluation_args, class_names, mode, pixels, skipped, nonfinite, temperature {value, at_edge, resolution, grid,
nll_per_pixel, nll_at_value}, before / after {overall, defects, per_class, each with its bins}).

``--save_calibrated`` writes a copy of the checkpoint whose 1x1 head is divided by T (keys ``temperature`` and
``calibration`` added): every CLI of this package loads it as it is and then sees calibrated confidences.

Three cautions.  Fit on ``--split val``, never on the split you report figures for.  The fold into the head is exact only
up to the head's rounding: the scaled weights are rounded to fp32 once, and a bf16 model quantises them anew.  Whether
calibration improves the accept / reject decisions on real Gear data has not been measured.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

from . import eval_detection, eval_regions, seg_calibration

DATASETS = eval_regions.DATASETS
_TILE_FLAGS = ("--tiled", "--tile", "--min_overlap")
EXTRA_FLAGS = [(n, kw) for n, kw in eval_detection.EXTRA_FLAGS if n in _TILE_FLAGS] + [
    ("--bins", dict(type=int, default=15, help="confidence bins of the reliability diagram, 1..64")),
    ("--temperature_range", dict(type=float, nargs=2, default=[0.25, 4.0], metavar=("LO", "HI"),
                                 help="the temperatures searched, 0 < LO < HI")),
    ("--temperature_steps", dict(type=int, default=32, help="grid points, evenly spaced in log T, 3..32")),
    ("--fit_on", dict(type=str, default="all", choices=["all", "defects"],
                      help="defects: leave out the pixels whose truth and prediction are both background")),
    ("--save_calibrated", dict(type=str, default=None, metavar="OUT.pth",
                               help="write a copy of the checkpoint with 1 / T folded into its 1x1 head (exact up to the "
                                    "head's rounding; a bf16 model quantises the scaled weights anew)"))]
EPILOG = ("Fit on --split val, never on the split you report.  The fold of --save_calibrated is exact only up to the "
          "head's rounding.  Whether calibration improves decisions on real Gear data has not been measured.")


def flags_of(dataset):
    cli = eval_regions._cli(dataset)
    return [(n, kw) for n, kw in cli.FLAGS if n not in eval_regions._NOT_HERE] + EXTRA_FLAGS


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    first = argparse.ArgumentParser(add_help=False)
    first.add_argument("--dataset", required=True, choices=DATASETS)
    dataset = first.parse_known_args(argv)[0].dataset          # its flags depend on the data set
    ap = argparse.ArgumentParser(description="Confidence calibration of a segmentation checkpoint: reliability, ECE, a "
                                             "fitted temperature (MI355X HIP path)", epilog=EPILOG)
    ap.add_argument("--dataset", required=True, choices=DATASETS)
    for name, kw in flags_of(dataset):
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    if args.tiled and dataset != "gear":
        ap.error("--tiled needs --dataset gear: KolektorSDD's masks are bitmaps, there is no full-resolution loader")
    if args.tile is None:
        args.tile = eval_detection.frame_of(args)
    if min(args.tile) < 1:
        ap.error("--tile sides must be positive")
    if args.min_overlap < 0 or (args.tiled and args.min_overlap >= min(args.tile)):
        ap.error("--min_overlap must be at least 0 and, with --tiled, smaller than both tile sides")
    if not 1 <= args.bins <= 64:
        ap.error("--bins must lie in 1..64")
    lo, hi = args.temperature_range
    if not 0.0 < lo < hi < float("inf"):
        ap.error("--temperature_range needs 0 < LO < HI")
    if not 3 <= args.temperature_steps <= 32:
        ap.error("--temperature_steps must lie in 3..32")
    return args


def frame_logits(model, batches):
    """(logits, masks) of (images, masks, paths) device batches, the model in eval mode"""
    import torch
    model.eval()
    with torch.no_grad():
        for images, masks, _paths in batches:
            yield model(images), masks


def tiled_logits(predictor, loader, device):
    """(logits (1, C, H, W), mask (1, H, W)) of every image of a raw Gear loader at its own size, the way
    ``eval_detection.match_tiled`` walks it"""
    import torch
    from .augment import color_jitter_normalize_u8
    from .crops import full_resolution_masks
    with torch.no_grad():
        for images, polys, sizes, _paths in loader:
            masks = full_resolution_masks(polys, sizes, device=device)
            for i in range(len(sizes)):
                frame = color_jitter_normalize_u8(images[i].to(device, non_blocking=True).unsqueeze(0))[0]
                logits, _plan = predictor.blended_logits(frame)
                yield logits.unsqueeze(0), masks[i].unsqueeze(0)


def measure(pairs, num_classes, bins, temperatures, temperature, select):
    """One pass: ``CalibrationMeter`` over (logits, masks) pairs, read back once."""
    from .evaluation import CalibrationMeter
    meter = CalibrationMeter(num_classes, bins=bins, temperatures=temperatures, temperature=temperature, select=select)
    for logits, masks in pairs:
        meter.update(logits, masks)
    return meter.compute()


def main(argv=None):
    args = parse_args(argv)
    import torch
    from .train_gear import build_seg_model, require_gpu
    from .utils import load_checkpoint

    device = require_gpu(args)
    cli = eval_regions._cli(args.dataset)
    mode = "tiled" if args.tiled else "frame"
    print("=" * 60 + f"\n{args.dataset.upper()} DATASET CALIBRATION ({mode})\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nDataset: {args.split} split")
    os.makedirs(args.save_dir, exist_ok=True)
    loader, num_classes = cli._split_loader(args)
    class_names = list(cli._class_names(loader.dataset, num_classes))
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

        def pairs():
            return tiled_logits(predictor, loader, device)
    else:
        def pairs():
            return frame_logits(model, cli._batches(args, loader, device))

    grid = seg_calibration.temperature_grid(args.temperature_range[0], args.temperature_range[1], args.temperature_steps)
    first = measure(pairs(), num_classes, args.bins, grid, 1.0, args.fit_on)
    counted = first["counted"]
    fit = seg_calibration.fit_temperature(grid, first["nll"])
    second = measure(pairs(), num_classes, args.bins, [fit["value"]], fit["value"], args.fit_on)
    before = seg_calibration.calibration_summary(first["hist"], class_names)
    after = seg_calibration.calibration_summary(second["hist"], class_names)
    temperature = {"value": fit["value"], "at_edge": fit["at_edge"], "resolution": fit["resolution"], "grid": grid,
                   "nll_per_pixel": [float(v) / counted if counted else 0.0 for v in first["nll"]],
                   "nll_at_value": float(second["nll"][0]) / second["counted"] if second["counted"] else 0.0}

    print(seg_calibration.format_table(before, after, fit["value"], class_names))
    edge = "  (at an end of --temperature_range: the minimum may lie outside it)" if fit["at_edge"] else ""
    print(f"Fitted temperature: {fit['value']:.4f}{edge}  NLL per pixel {temperature['nll_at_value']:.6f}  "
          f"(grid ratio {fit['resolution']:.4f})")
    summary_path = os.path.join(args.save_dir, "calibration_results.json")
    with open(summary_path, "w") as f:
        json.dump({"evaluation_args": vars(args), "class_names": class_names, "mode": mode,
                   "pixels": before["overall"]["pixels"], "skipped": first["skipped"], "nonfinite": first["nonfinite"],
                   "temperature": temperature, "before": before, "after": after}, f, indent=2)
    print(f"Calibration results saved to: {summary_path}")
    if args.save_calibrated:
        ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        def no_bins(r):
            return {f: v for f, v in r.items() if f != "bins"}
        brief = {"overall": no_bins(after["overall"]), "defects": no_bins(after["defects"]),
                 "per_class": {k: no_bins(v) for k, v in after["per_class"].items()}}
        torch.save(seg_calibration.calibrated_checkpoint(ckpt, fit["value"], brief), args.save_calibrated)
        print(f"Calibrated checkpoint saved to: {args.save_calibrated}")
    return summary_path


if __name__ == "__main__":
    main()
