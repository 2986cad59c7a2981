"""Shared implementation of the segmentation evaluation CLIs ``eval_gear`` and ``eval_kolektorsdd`` (reference test.py
and test_kolektorsdd.py): load a checkpoint, run the model over the val or test split in eval mode, and write
``{save_dir}/evaluation_results.json`` with the reference's schema (test.py:192-223: ``evaluation_args``,
``overall_metrics``, ``per_class_metrics``, ``confusion_matrix``).

Per batch one ``metrics.per_image_stats`` launch (csrc/segeval.hip) yields every image's confusion counts and
max-probability statistics on the device; the reference copies every prediction to the host instead.  The
confusions are summed on the device, and everything is read back once, after the last batch.  The total goes to a
``SegmentationMetrics`` through its ``confusion_matrix`` setter, so the overall and per-class numbers are that
class's.  Build-only output: ``per_image_results.json``, one entry per image with its path and the reference's
``compute_prediction_stats`` dict (visualize.py:239-257).  ``--save_predictions`` writes the reference's three-panel
PNGs for the first 5 batches (up to 4 images each) and ``confusion_matrix.png``, drawn from the kernel's uint8 label
maps; they are skipped silently when matplotlib is missing.
"""
from __future__ import annotations

import argparse
import json
import os
import random

import numpy as np
import torch

from .dataset import MEAN, STD

VIS_BATCHES, VIS_IMAGES = 5, 4          # reference test.py:113 (batch_idx < 5), :153 (up to 4 images per batch)


def eval_flags(size_flags, data_root, extra=()):
    """The reference's evaluation flags (test.py:20-64 / test_kolektorsdd.py:20-72) plus --precision."""
    return [("--data_root", dict(type=str, default=data_root)), *size_flags,
            ("--split", dict(type=str, default="test", choices=["test", "val"])),
            ("--model", dict(type=str, default="seg_unet", choices=["unet", "seg_unet"])),
            ("--checkpoint", dict(type=str, required=True)),
            ("--bilinear", dict(action="store_true")),
            ("--dropout", dict(type=float, default=0.1)),
            *extra,
            ("--batch_size", dict(type=int, default=8)),
            ("--num_workers", dict(type=int, default=4)),
            ("--device", dict(type=str, default="auto")),
            ("--save_dir", dict(type=str, default="test_results")),
            ("--save_predictions", dict(action="store_true")),
            ("--save_confusion_matrix", dict(action="store_true")),
            ("--debug", dict(action="store_true")),
            ("--debug_samples", dict(type=int, default=50)),
            # build-only
            ("--precision", dict(type=str, default="fp32", choices=["fp32", "bf16"]))]


def parse_args(flags, description, argv=None):
    ap = argparse.ArgumentParser(description=description)
    for name, kw in flags:
        ap.add_argument(name, **kw)
    return ap.parse_args(argv)


def evaluate(model, batches, num_classes, class_names, vis_dir=None):
    """Eval-mode pass over ``batches`` of (images, masks, paths) on the device.  Returns the ``SegmentationMetrics``
    of the whole split and the per-image entries; draws the prediction PNGs into ``vis_dir`` when it is given."""
    from .metrics import SegmentationMetrics, image_prediction_stats, per_image_stats
    model.eval()
    total, cms, means, stds, paths, vis = None, [], [], [], [], []
    with torch.no_grad():
        for b, (images, masks, batch_paths) in enumerate(batches):
            outputs = model(images)
            draw = vis_dir is not None and b < VIS_BATCHES
            st = per_image_stats(outputs, masks, labels=draw)
            batch_cm = st["confusion"].sum(0)
            total = batch_cm if total is None else total + batch_cm
            cms.append(st["confusion"]); means.append(st["conf_mean"]); stds.append(st["conf_std"])
            paths.extend(batch_paths)
            if draw:
                k = min(len(batch_paths), VIS_IMAGES)
                vis.append((images[:k].clone(), masks[:k].clone(), st["labels"][:k], list(batch_paths[:k])))
    metrics = SegmentationMetrics(num_classes)
    if total is not None:                              # the one read-back of the pass
        metrics.confusion_matrix = total.cpu().numpy()
        cms, means, stds = torch.cat(cms).cpu().numpy(), torch.cat(means).tolist(), torch.cat(stds).tolist()
    per_image = [{"image_path": p, **image_prediction_stats(cm, mu, sd, class_names)}
                 for p, cm, mu, sd in zip(paths, cms, means, stds)]
    if vis_dir is not None:
        plt = _pyplot()
        if plt is not None:
            for b, (images, masks, labels, batch_paths) in enumerate(vis):
                _save_batch_predictions(plt, images.float().cpu(), masks.cpu(), labels.cpu(), batch_paths, vis_dir, b,
                                        class_names)
            _plot_confusion_matrix(plt, metrics.confusion_matrix, class_names, os.path.join(vis_dir, "confusion_matrix.png"))
    return metrics, per_image


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:                                          # plotting is optional (utils.plot_training_curves)
        return None
    return plt


def _save_batch_predictions(plt, images, masks, labels, paths, save_dir, batch_idx, class_names):
    """reference test.py:145-191: image | ground truth | prediction, tab10 over the class range, 150 dpi"""
    mean, std = torch.tensor(MEAN).reshape(3, 1, 1), torch.tensor(STD).reshape(3, 1, 1)
    for i in range(len(paths)):
        fig, axes = plt.subplots(1, 3, figsize=(15, 5))
        img = torch.clamp(images[i] * std + mean, 0, 1).permute(1, 2, 0).numpy()
        panels = (("Original Image", img, {}),
                  ("Ground Truth", masks[i].numpy(), dict(cmap="tab10", vmin=0, vmax=len(class_names) - 1)),
                  ("Prediction", labels[i].numpy(), dict(cmap="tab10", vmin=0, vmax=len(class_names) - 1)))
        for ax, (title, data, kw) in zip(axes, panels):
            ax.imshow(data, **kw)
            ax.set_title(title)
            ax.axis("off")
        plt.tight_layout()
        name = os.path.basename(paths[i]).split(".")[0]
        plt.savefig(os.path.join(save_dir, f"prediction_batch{batch_idx}_img{i}_{name}.png"), dpi=150, bbox_inches="tight")
        plt.close(fig)


def _plot_confusion_matrix(plt, cm, class_names, save_path):
    """reference metrics.py:178-204 (row-normalised, annotated, 'Blues'), drawn with matplotlib alone"""
    norm = cm.astype(np.float64) / (cm.sum(axis=1)[:, None] + 1e-8)
    fig, ax = plt.subplots(figsize=(10, 8))
    im = ax.imshow(norm, cmap="Blues")
    fig.colorbar(im, ax=ax)
    ax.set_xticks(range(len(class_names)), class_names)
    ax.set_yticks(range(len(class_names)), class_names)
    for r in range(norm.shape[0]):
        for c in range(norm.shape[1]):
            ax.text(c, r, f"{norm[r, c]:.3f}", ha="center", va="center",
                    color="white" if norm[r, c] > 0.5 * max(norm.max(), 1e-8) else "black")
    ax.set_title("Normalized Confusion Matrix")
    ax.set_xlabel("Predicted Label")
    ax.set_ylabel("True Label")
    plt.tight_layout()
    fig.savefig(save_path, dpi=300, bbox_inches="tight")
    plt.close(fig)


def results_summary(metrics, args):
    """reference test.py:192-223 save_results_summary, key for key"""
    m = metrics.compute_all_metrics()
    return {"evaluation_args": vars(args),
            "overall_metrics": {k: float(m[k]) for k in ("pixel_accuracy", "mean_accuracy", "mean_iou", "mean_dice",
                                                         "mean_precision", "mean_recall", "mean_f1")},
            "per_class_metrics": {k: m[f"{k}_per_class"].tolist() for k in ("iou", "dice", "precision", "recall", "f1")},
            "confusion_matrix": m["confusion_matrix"].tolist()}


def run(args, title, split_loader, batches, class_names_of):
    """The evaluation CLI body.  split_loader(args) -> (loader of the --split, num_classes); batches(loader, device)
    -> iterable of (images, masks, paths) device batches; class_names_of(dataset, num_classes) -> names."""
    from .train_gear import build_seg_model, require_gpu
    from .utils import load_checkpoint

    device = require_gpu(args)
    print("=" * 60 + f"\n{title} DATASET EVALUATION\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nDataset: {args.split} split")
    os.makedirs(args.save_dir, exist_ok=True)
    loader, num_classes = split_loader(args)
    if args.debug:
        from torch.utils.data import DataLoader, Subset
        print(f"DEBUG MODE: Limiting evaluation to {args.debug_samples} samples")
        idx = random.sample(range(len(loader.dataset)), min(args.debug_samples, len(loader.dataset)))
        loader = DataLoader(Subset(loader.dataset, idx), batch_size=args.batch_size, shuffle=False,
                            num_workers=args.num_workers, pin_memory=True, collate_fn=loader.collate_fn)
    class_names = class_names_of(loader.dataset, num_classes)
    print(f"Number of classes: {num_classes}\nClass names: {class_names}\nSamples: {len(loader.dataset)}")

    model = build_seg_model(args, num_classes, device)
    epoch, loss = load_checkpoint(model, None, args.checkpoint, device)
    print(f"Loaded checkpoint from epoch {epoch} with loss {loss:.4f}")
    print(f"Model parameters: {sum(p.numel() for p in model.parameters()):,}")

    metrics, per_image = evaluate(model, batches(loader, device), num_classes, class_names,
                                  args.save_dir if args.save_predictions else None)
    metrics.print_metrics(class_names)
    summary_path = os.path.join(args.save_dir, "evaluation_results.json")
    with open(summary_path, "w") as f:
        json.dump(results_summary(metrics, args), f, indent=2)
    with open(os.path.join(args.save_dir, "per_image_results.json"), "w") as f:
        json.dump(per_image, f, indent=2)
    m = metrics.compute_all_metrics()
    print(f"Results summary saved to: {summary_path}")
    print(f"Samples evaluated: {len(per_image):,}\nPixel Accuracy: {m['pixel_accuracy']:.4f}\n"
          f"Mean IoU: {m['mean_iou']:.4f}\nMean Dice: {m['mean_dice']:.4f}\nMean F1: {m['mean_f1']:.4f}")
    return summary_path
