#!/usr/bin/env python3
"""Gear trainer for the resolution ``predict_tiled`` works at (no reference counterpart): ``train_gear`` squeezes every
image into one frame (1920 x 1080 -> 512 x 512), this one trains on crops cut from the images at their own resolution.

    python -m tiaozhanbei_unet_amd.train_gear_crops --data_root datasets/Gear --epochs 50 [--precision bf16] [--synthetic]

Training: the loader hands over ``--batch_size // --crops_per_image`` decoded images per step; ``crops.GearCropPreprocess``
draws ``--crops_per_image`` crops of ``--crop_size`` from each (scale log-uniform in ``--scale_range``, rotation within
+-``--degrees``, flip; with probability ``--defect_fraction`` centred inside a labelled defect's box) and cuts images
(bilinear) and full-resolution class masks (nearest) on the GPU in one launch each (csrc/crops.hip).  Where a crop leaves
its image the mask carries 255, which the loss and the training metrics ignore.

Validation: every validation image is only normalised, at its own size, and run through ``tiling.TiledPredictor`` with
tiles of ``--crop_size`` overlapping by ``--min_overlap`` -- the way ``predict_tiled`` will use the checkpoint; mIoU is
counted on the blended label map against the full-resolution polygon mask, the loss on the blended logits, and the best
model is chosen by that mIoU.

The output tree, ``args.json``, ``training_results.json`` and the checkpoints are ``train_gear``'s, under
``{save_dir}/gear_crops_{model}_{ts}``: ``predict``, ``predict_tiled``, ``eval_gear`` and ``eval_regions`` load them.
"""
import argparse
import json
import os
import random
import tempfile
from datetime import datetime

from .train_gear import FLAGS as TRAIN_GEAR_FLAGS

FLAGS = [(name, kw) for name, kw in TRAIN_GEAR_FLAGS if name not in ("--image_size", "--sync_mask")] + [
    ("--crop_size", dict(type=int, nargs=2, default=[512, 512], metavar=("H", "W"), help="the crop the model trains on")),
    ("--crops_per_image", dict(type=int, default=4, help="crops drawn from every loaded image")),
    ("--defect_fraction", dict(type=float, default=0.5, help="share of crops centred inside a labelled defect's box")),
    ("--scale_range", dict(type=float, nargs=2, default=[0.75, 1.5], metavar=("LO", "HI"),
                           help="source pixels per crop pixel, log-uniform (0 < LO <= HI <= 4)")),
    ("--degrees", dict(type=float, default=10.0, help="rotation within +-degrees")),
    ("--min_overlap", dict(type=int, default=64, help="validation: pixels neighbouring tiles share at least")),
]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Train UNet for Gear segmentation on native-resolution crops (MI355X HIP path)")
    for name, kw in FLAGS:
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    check_args(ap, args)
    return args


def check_args(ap, args):
    """the refusals of this trainer's own flags (``train_gear_paste`` shares them)"""
    if not all(1 <= v <= 4096 for v in args.crop_size):
        ap.error("--crop_size sides must lie in 1..4096")
    if args.crops_per_image < 1:
        ap.error("--crops_per_image must be at least 1")
    if args.batch_size < 1 or args.batch_size % args.crops_per_image:
        ap.error("--batch_size counts crops: it must be a positive multiple of --crops_per_image")
    if not 0.0 <= args.defect_fraction <= 1.0:
        ap.error("--defect_fraction must lie in 0..1")
    if not 0.0 < args.scale_range[0] <= args.scale_range[1] <= 4.0:
        ap.error("--scale_range needs 0 < LO <= HI <= 4")
    if not 0.0 <= args.degrees <= 180.0:
        ap.error("--degrees must lie in 0..180")
    if not 0 <= args.min_overlap < min(args.crop_size):
        ap.error("--min_overlap must be at least 0 and smaller than both crop sides")


def check_image_sizes(datasets):
    """Refuse, before the first epoch, an image the full-resolution mask or crop kernels cannot take: the header of
    every image file is read (no decode)."""
    from PIL import Image
    from .augment import POLY_MAX_WIDTH
    from .crops import MAX_IMAGE_SIDE
    for ds in datasets:
        for path in ds.image_paths:
            with Image.open(path) as im:
                w, h = im.size
            if w > POLY_MAX_WIDTH or h > MAX_IMAGE_SIDE:
                raise SystemExit(f"{path} is {w} x {h} pixels: crop training takes images at most {POLY_MAX_WIDTH} wide "
                                 f"and {MAX_IMAGE_SIDE} high (the full-resolution mask kernel's limits)")


def validate_tiled(model, criterion, loader, predictor, num_classes, device):
    """Validation the way ``predict_tiled`` predicts: image by image at its own size.  The loss is the unweighted mean of
    the per-image losses on the blended logits, the metrics those of the blended label maps."""
    import torch
    from .metrics import SegmentationMetrics
    from .seg_cli import full_resolution_images, normalized_frame
    metrics = SegmentationMetrics(num_classes)
    total = torch.zeros((), dtype=torch.float64, device=device)
    count = 0
    with torch.no_grad():
        for image, mask, _path in full_resolution_images(loader, device):
            labels, _conf, mixed, _plan = predictor.blended(normalized_frame(image))
            target = mask[None].long()
            total += criterion(mixed[None], target).detach().double()
            metrics.update(labels[None], target)
            count += 1
    return {"loss": float(total) / max(count, 1), "metrics": metrics.compute_all_metrics()}


def crop_preprocess(args, crop):
    """the training batches' ``GearCropPreprocess`` of this trainer's flags"""
    from .crops import GearCropPreprocess
    return GearCropPreprocess(crop, train=True, crops_per_image=args.crops_per_image, scale_range=tuple(args.scale_range),
                              degrees=args.degrees, defect_fraction=args.defect_fraction, seed=args.seed)


def run(args, prefix, make_preprocess):
    """The trainer behind ``train_gear_crops`` and ``train_gear_paste``: the experiment lies under
    ``{save_dir}/{prefix}_{model}_{ts}``, ``make_preprocess(args, crop)`` makes the training batches'
    ``GearCropPreprocess``.  Returns the experiment directory."""
    from .train_gear import build_seg_model, fit_segmentation, require_gpu
    device = require_gpu(args)
    import numpy as np
    import torch
    from .crops import IGNORE_INDEX
    from .gear_dataset import collate_raw, get_gear_dataloaders, write_synthetic_gear
    from .tiling import TiledPredictor
    from .utils import create_output_dirs

    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if args.synthetic:
        args.data_root = write_synthetic_gear(tempfile.mkdtemp(prefix="gear_syn_"), seed=args.seed)
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    exp_dir = os.path.join(args.save_dir, f"{prefix}_{args.model}_{stamp}")
    dirs = create_output_dirs(exp_dir)
    print(f"Using device: {device}\nExperiment directory: {exp_dir}")
    with open(os.path.join(exp_dir, "args.json"), "w") as f:
        json.dump(vars(args), f, indent=2)

    crop = tuple(args.crop_size)
    images_per_batch = args.batch_size // args.crops_per_image
    train_loader, val_loader, _test_loader, num_classes = get_gear_dataloaders(
        args.data_root, images_per_batch, crop, args.num_workers, seed=args.seed)
    if args.debug:
        from torch.utils.data import DataLoader, Subset

        def limit(loader, shuffle):
            idx = random.sample(range(len(loader.dataset)), min(args.debug_samples, len(loader.dataset)))
            sub = Subset(loader.dataset, idx)
            sub.image_paths = [loader.dataset.image_paths[i] for i in idx]
            return DataLoader(sub, batch_size=images_per_batch, shuffle=shuffle, num_workers=args.num_workers,
                              pin_memory=True, collate_fn=collate_raw)
        train_loader, val_loader = limit(train_loader, True), limit(val_loader, False)
    check_image_sizes([train_loader.dataset, val_loader.dataset])
    print(f"Number of classes: {num_classes}\nTrain samples: {len(train_loader.dataset)}\n"
          f"Val samples: {len(val_loader.dataset)}")
    print(f"Crops: {crop[0]} x {crop[1]}, {args.crops_per_image} per image, scale {args.scale_range}, "
          f"+-{args.degrees} degrees, {args.defect_fraction:.2f} on defects")

    model = build_seg_model(args, num_classes, device)
    train_pre = make_preprocess(args, crop)
    predictor = TiledPredictor(model, crop, args.min_overlap, args.batch_size)

    def train_batches(loader):
        for images, polys, sizes, _paths in loader:
            yield train_pre(images, polys, sizes, device=device)
        if train_pre.paste is not None:
            print(train_pre.paste.report())

    return fit_segmentation(args, exp_dir, dirs, model, train_loader, val_loader, num_classes, device, train_batches, None,
                            ignore_index=IGNORE_INDEX,
                            validate=lambda m, criterion: validate_tiled(m, criterion, val_loader, predictor, num_classes,
                                                                         device))


def main(argv=None):
    return run(parse_args(argv), "gear_crops", crop_preprocess)


if __name__ == "__main__":
    main()
