#!/usr/bin/env python3
"""KolektorSDD defect segmentation trainer with the reference's contract (reference train_kolektorsdd.py): same
flag names and defaults (:26-101), output tree ``{save_dir}/kolektorsdd_{model}_{ts}/{checkpoints,results,
visualizations,logs}``, ``args.json``, ``best_model.pth`` by validation mIoU, ``checkpoint_epoch_{e}.pth`` and
``training_results.json`` keys -- running on the HIP path: workers only decode, ``kolektorsdd_dataset.GpuPreprocess``
makes images and masks on the GPU, and the epoch loop is ``train_gear``'s.

    python -m tiaozhanbei_unet_amd.train_kolektorsdd --data_root datasets/KolektorSDD --epochs 50 [--precision bf16]

Build-only additions: --precision {fp32,bf16}, --synthetic (generate a small KolektorSDD-layout dataset), --sync_mask
(apply the image's random flip / rotation to the mask too).  Without --sync_mask the mask is neither flipped nor
rotated, as in the reference (its target transform has no augmentation).
"""
import argparse
import json
import os
import random
import tempfile
from datetime import datetime

import numpy as np
import torch

FLAGS = [  # name, kwargs  -- reference train_kolektorsdd.py:26-101
    ("--data_root", dict(type=str, default="datasets/KolektorSDD")),
    ("--image_height", dict(type=int, default=1024)),
    ("--image_width", dict(type=int, default=512)),
    ("--model", dict(type=str, default="seg_unet", choices=["unet", "seg_unet"])),
    ("--bilinear", dict(action="store_true")),
    ("--dropout", dict(type=float, default=0.1)),
    ("--train_split", dict(type=float, default=0.7)),
    ("--val_split", dict(type=float, default=0.15)),
    ("--epochs", dict(type=int, default=50)),
    ("--batch_size", dict(type=int, default=8)),
    ("--learning_rate", dict(type=float, default=1e-3)),
    ("--weight_decay", dict(type=float, default=1e-4)),
    ("--optimizer", dict(type=str, default="adam", choices=["adam", "adamw", "sgd"])),
    ("--ce_weight", dict(type=float, default=1.0)),
    ("--dice_weight", dict(type=float, default=1.0)),
    ("--focal_weight", dict(type=float, default=0.0)),
    ("--class_weights", dict(type=str, default="1.0,50.0,50.0")),
    ("--num_workers", dict(type=int, default=4)),
    ("--device", dict(type=str, default="auto")),
    ("--seed", dict(type=int, default=42)),
    ("--save_dir", dict(type=str, default="outputs")),
    ("--save_freq", dict(type=int, default=10)),
    ("--resume", dict(type=str, default=None)),
    ("--val_freq", dict(type=int, default=5)),
    ("--debug", dict(action="store_true")),
    ("--debug_samples", dict(type=int, default=20)),
    # build-only
    ("--precision", dict(type=str, default="fp32", choices=["fp32", "bf16"])),
    ("--synthetic", dict(action="store_true")),
    ("--sync_mask", dict(action="store_true")),
]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Train UNet for KolektorSDD defect detection (MI355X HIP path)")
    for name, kw in FLAGS:
        ap.add_argument(name, **kw)
    return ap.parse_args(argv)


def kolektor_batches(loader, preprocess, device):
    """(images fp32 NCHW, masks long NHW) on the device from ``kolektorsdd_dataset.collate_raw`` batches."""
    for images, masks, _paths in loader:
        yield preprocess(images, masks, device=device)


def main(argv=None):
    from .kolektorsdd_dataset import GpuPreprocess, collate_raw, get_kolektorsdd_dataloaders, write_synthetic_kolektorsdd
    from .train_gear import build_seg_model, fit_segmentation, require_gpu
    from .utils import create_output_dirs

    args = parse_args(argv)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    device = require_gpu(args)

    if args.synthetic:
        args.data_root = write_synthetic_kolektorsdd(tempfile.mkdtemp(prefix="kolektorsdd_syn_"), seed=args.seed)
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    exp_dir = os.path.join(args.save_dir, f"kolektorsdd_{args.model}_{stamp}")
    dirs = create_output_dirs(exp_dir)
    print(f"Using device: {device}\nExperiment directory: {exp_dir}")
    with open(os.path.join(exp_dir, "args.json"), "w") as f:
        json.dump(vars(args), f, indent=2)

    size = (args.image_height, args.image_width)
    train_loader, val_loader, _test_loader, num_classes = get_kolektorsdd_dataloaders(
        args.data_root, args.batch_size, size, args.num_workers, args.train_split, args.val_split, seed=args.seed,
        raw=True)
    if args.debug:
        from torch.utils.data import DataLoader, Subset

        def limit(loader, shuffle):
            idx = random.sample(range(len(loader.dataset)), min(args.debug_samples, len(loader.dataset)))
            return DataLoader(Subset(loader.dataset, idx), batch_size=args.batch_size, shuffle=shuffle,
                              num_workers=args.num_workers, pin_memory=True, collate_fn=collate_raw)
        train_loader, val_loader = limit(train_loader, True), limit(val_loader, False)
    print(f"Number of classes: {num_classes}\nTrain samples: {len(train_loader.dataset)}\n"
          f"Val samples: {len(val_loader.dataset)}")

    model = build_seg_model(args, num_classes, device)
    # the mask default is the reference's (no flip / rotation): pass it explicitly, GpuPreprocess defaults to True
    train_pre = GpuPreprocess(size, train=True, seed=args.seed, sync_mask=args.sync_mask)
    eval_pre = GpuPreprocess(size, train=False)
    return fit_segmentation(args, exp_dir, dirs, model, train_loader, val_loader, num_classes, device,
                            lambda loader: kolektor_batches(loader, train_pre, device),
                            lambda loader: kolektor_batches(loader, eval_pre, device))


if __name__ == "__main__":
    main()
