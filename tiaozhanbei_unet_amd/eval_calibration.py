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

import json
import os

from . import seg_calibration, seg_cli

DATASETS = seg_cli.DATASETS
EXTRA_FLAGS = seg_cli.TILING_FLAGS + [
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
    return seg_cli.base_flags(dataset) + EXTRA_FLAGS


def parse_args(argv=None):
    ap, args = seg_cli.parse_dataset_args(argv, "Confidence calibration of a segmentation checkpoint: reliability, ECE, a "
                                                "fitted temperature (MI355X HIP path)", flags_of, epilog=EPILOG)
    seg_cli.check_tiling(ap, args)
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
    ``seg_cli.tiled_predictions`` walks it"""
    import torch
    with torch.no_grad():
        for image, mask, _path in seg_cli.full_resolution_images(loader, device):
            logits, _plan = predictor.blended_logits(seg_cli.normalized_frame(image))
            yield logits[None], mask[None]


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

    mode = seg_cli.mode_of(args)
    device, cli, loader, num_classes, class_names, model = seg_cli.open_checkpoint_session(args, "CALIBRATION", mode)
    class_names = list(class_names)
    if args.tiled:
        predictor = seg_cli.tiled_predictor(args, loader, model)

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
