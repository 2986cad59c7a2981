#!/usr/bin/env python3
"""Gear multi-class segmentation trainer with the reference's contract (/root/reference/train.py): same flag names and
defaults (:26-97), output tree ``{save_dir}/gear_seg_{model}_{ts}/{checkpoints,results,visualizations,logs}`` (:237-240),
``args.json``, ``best_model.pth`` by validation mIoU, ``checkpoint_epoch_{e}.pth`` and ``training_results.json`` keys
(:389-400) -- running on the HIP path: workers decode and parse, ``gear_dataset.GearPreprocess`` makes images and masks
on the GPU, ``SegmentationUNet`` / ``UNet``, ``CombinedSegmentationLoss`` and ``SegmentationMetrics`` run in
libunet_hip.so.

    python -m tiaozhanbei_unet_amd.train_gear --data_root datasets/Gear --epochs 50 [--precision bf16] [--synthetic]

Build-only additions: --precision {fp32,bf16}, --synthetic (generate a small Gear-layout dataset), --sync_mask (apply
the image's random flip / rotation to the mask too; the reference leaves the mask unrotated).
"""
import argparse
import json
import os
import random
import tempfile
import time
from datetime import datetime

import numpy as np
import torch

FLAGS = [  # name, kwargs  -- reference train.py:26-97
    ("--data_root", dict(type=str, default="datasets/Gear")),
    ("--image_size", dict(type=int, default=512)),
    ("--model", dict(type=str, default="seg_unet", choices=["unet", "seg_unet"])),
    ("--bilinear", dict(action="store_true")),
    ("--dropout", dict(type=float, default=0.1)),
    ("--epochs", dict(type=int, default=50)),
    ("--batch_size", dict(type=int, default=8)),
    ("--learning_rate", dict(type=float, default=1e-3)),
    ("--weight_decay", dict(type=float, default=1e-4)),
    ("--optimizer", dict(type=str, default="adam", choices=["adam", "adamw", "sgd"])),
    ("--ce_weight", dict(type=float, default=1.0)),
    ("--dice_weight", dict(type=float, default=1.0)),
    ("--focal_weight", dict(type=float, default=0.0)),
    ("--class_weights", dict(type=str, default=None)),
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
    ap = argparse.ArgumentParser(description="Train UNet for Gear multi-class segmentation (MI355X HIP path)")
    for name, kw in FLAGS:
        ap.add_argument(name, **kw)
    return ap.parse_args(argv)


def _seg_batches(loader, preprocess, device):
    """(images fp32 NCHW, masks long NHW) on the device from ``gear_dataset.collate_raw`` batches."""
    for images, polys, sizes, _paths in loader:
        yield preprocess(images, polys, sizes, device=device)


def train_seg_epoch(model, dataloader, criterion, optimizer, device, epoch, num_classes, preprocess, *, batches=None,
                    ignore_index=None):
    """One training epoch (reference train.py:118-160): the loss is the UNWEIGHTED mean of the per-batch losses, the
    metrics those of a ``SegmentationMetrics`` updated with every batch.  Losses are summed on the device and read once.
    ``batches``: an iterable of (images, masks) device batches to use instead of ``dataloader`` + ``preprocess``.
    ``ignore_index``: a mask value the metrics leave out (None: none, as the reference)."""
    from .metrics import SegmentationMetrics
    model.train()
    metrics = SegmentationMetrics(num_classes, ignore_index=ignore_index)
    total = torch.zeros((), dtype=torch.float64, device=device)
    n_batches = 0
    for images, masks in _seg_batches(dataloader, preprocess, device) if batches is None else batches:
        optimizer.zero_grad(set_to_none=True)
        outputs = model(images)
        loss = criterion(outputs, masks)
        loss.backward()
        optimizer.step()
        total += loss.detach().double()
        metrics.update(outputs, masks)
        n_batches += 1
    return {"loss": float(total) / max(n_batches, 1), "metrics": metrics.compute_all_metrics()}


def validate_seg_epoch(model, dataloader, criterion, device, num_classes, preprocess, *, batches=None):
    """Eval-mode pass (reference train.py:163-202): unweighted mean of the per-batch losses + device metrics.
    ``batches``: as in ``train_seg_epoch``."""
    from .metrics import SegmentationMetrics
    model.eval()
    metrics = SegmentationMetrics(num_classes)
    total = torch.zeros((), dtype=torch.float64, device=device)
    n_batches = 0
    with torch.no_grad():
        for images, masks in _seg_batches(dataloader, preprocess, device) if batches is None else batches:
            outputs = model(images)
            total += criterion(outputs, masks).detach().double()
            metrics.update(outputs, masks)
            n_batches += 1
    return {"loss": float(total) / max(n_batches, 1), "metrics": metrics.compute_all_metrics()}


def _print_epoch(epoch, tr, vr, seconds):
    print("=" * 60)
    print(f"EPOCH {epoch:3d} RESULTS")
    for name, r in (("TRAINING", tr), ("VALIDATION", vr)):
        if r is None:
            continue
        m = r["metrics"]
        print(f"{name}: loss {r['loss']:.4f}  mIoU {m['mean_iou']:.4f}  mDice {m['mean_dice']:.4f}  "
              f"accuracy {m['pixel_accuracy']:.4f}")
    print(f"Epoch time: {seconds:.2f}s")


def require_gpu(args):
    """The device of a seg CLI (train or eval); exits with the package's one-line message for a CPU device."""
    if args.device == "cpu" or not torch.cuda.is_available():
        raise SystemExit("this build computes only on an AMD GPU (libunet_hip.so); there is no CPU path")
    device = torch.device(args.device if args.device not in ("auto", "cuda") else "cuda")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.set_device(device)
    return device


def build_seg_model(args, num_classes, device):
    """SegmentationUNet / UNet of the seg CLIs' --model, --bilinear, --dropout and --precision."""
    from . import SegmentationUNet, UNet
    if args.model == "seg_unet":
        model = SegmentationUNet(n_channels=3, n_classes=num_classes, bilinear=args.bilinear, dropout=args.dropout,
                                 precision=args.precision)
    else:
        model = UNet(n_channels=3, n_classes=num_classes, bilinear=args.bilinear, precision=args.precision)
    return model.to(device)


def fit_segmentation(args, exp_dir, dirs, model, train_loader, val_loader, num_classes, device, train_batches,
                     val_batches, *, ignore_index=None, validate=None):
    """The epoch loop, checkpoints and ``training_results.json`` shared by the Gear and KolektorSDD trainers (reference
    train.py:333-400, train_kolektorsdd.py:370-452).  ``train_batches`` / ``val_batches``: loader -> iterable of
    (images, masks) device batches.  ``ignore_index``: a mask value the loss and the training metrics leave out (None:
    none).  ``validate``: ``(model, criterion) -> {"loss", "metrics"}`` to use instead of ``validate_seg_epoch`` over
    ``val_batches`` (which may then be None)."""
    from .metrics import CombinedSegmentationLoss
    from .train_utils import get_optimizer
    from .utils import load_checkpoint, save_checkpoint

    total_params = sum(p.numel() for p in model.parameters())
    print(f"Total parameters: {total_params:,}")
    class_weights = [float(w) for w in args.class_weights.split(",")] if args.class_weights else None
    criterion = CombinedSegmentationLoss(ce_weight=args.ce_weight, dice_weight=args.dice_weight,
                                         focal_weight=args.focal_weight, ignore_index=ignore_index,
                                         class_weights=class_weights)
    optimizer = get_optimizer(model, args.optimizer, args.learning_rate, args.weight_decay)
    start_epoch = 0
    if args.resume:
        start_epoch = load_checkpoint(model, optimizer, args.resume, device)[0] + 1
        print(f"Resumed from epoch {start_epoch}")

    train_losses, val_losses, best_val_miou = [], [], 0.0
    for epoch in range(start_epoch, args.epochs):
        t0 = time.time()
        tr = train_seg_epoch(model, train_loader, criterion, optimizer, device, epoch, num_classes, None,
                             batches=train_batches(train_loader), ignore_index=ignore_index)
        train_seconds = time.time() - t0
        train_losses.append(tr["loss"])
        vr = None
        if epoch % args.val_freq == 0 or epoch == args.epochs - 1:
            if validate is not None:
                vr = validate(model, criterion)
            else:
                vr = validate_seg_epoch(model, val_loader, criterion, device, num_classes, None,
                                        batches=val_batches(val_loader))
            val_losses.append(vr["loss"])
            if vr["metrics"]["mean_iou"] > best_val_miou:
                best_val_miou = float(vr["metrics"]["mean_iou"])
                save_checkpoint(model, optimizer, epoch, vr["loss"], os.path.join(dirs["checkpoints"], "best_model.pth"))
                print(f"New best model saved with mIoU: {best_val_miou:.4f}")
            _print_epoch(epoch, tr, vr, time.time() - t0)
        print(f"Epoch {epoch}: train {len(train_loader.dataset) / max(train_seconds, 1e-9):.1f} img/s")
        if epoch % args.save_freq == 0 or epoch == args.epochs - 1:
            save_checkpoint(model, optimizer, epoch, tr["loss"],
                            os.path.join(dirs["checkpoints"], f"checkpoint_epoch_{epoch}.pth"))

    results = {"train_losses": train_losses, "val_losses": val_losses, "best_val_miou": best_val_miou,
               "total_epochs": args.epochs, "total_params": total_params, "num_classes": num_classes, "args": vars(args)}
    with open(os.path.join(dirs["results"], "training_results.json"), "w") as f:
        json.dump(results, f, indent=2)
    print(f"Training completed!\nBest validation mIoU: {best_val_miou:.4f}\nResults saved to: {exp_dir}")
    return exp_dir


def main(argv=None):
    from .gear_dataset import GearPreprocess, collate_raw, get_gear_dataloaders, write_synthetic_gear
    from .utils import create_output_dirs

    args = parse_args(argv)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    device = require_gpu(args)

    if args.synthetic:
        args.data_root = write_synthetic_gear(tempfile.mkdtemp(prefix="gear_syn_"), seed=args.seed)
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    exp_dir = os.path.join(args.save_dir, f"gear_seg_{args.model}_{stamp}")
    dirs = create_output_dirs(exp_dir)
    print(f"Using device: {device}\nExperiment directory: {exp_dir}")
    with open(os.path.join(exp_dir, "args.json"), "w") as f:
        json.dump(vars(args), f, indent=2)

    size = (args.image_size, args.image_size)
    train_loader, val_loader, _test_loader, num_classes = get_gear_dataloaders(
        args.data_root, args.batch_size, size, args.num_workers, seed=args.seed)
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
    train_pre = GearPreprocess(size, train=True, sync_mask=args.sync_mask, seed=args.seed)
    eval_pre = GearPreprocess(size, train=False)
    return fit_segmentation(args, exp_dir, dirs, model, train_loader, val_loader, num_classes, device,
                            lambda loader: _seg_batches(loader, train_pre, device),
                            lambda loader: _seg_batches(loader, eval_pre, device))


if __name__ == "__main__":
    main()
