"""Shared implementation of the prediction visualisers ``visualize_gear`` and ``visualize_kolektorsdd`` (reference
visualize.py and visualize_kolektorsdd.py): load a checkpoint, run the model in eval mode over the first
``--num_samples`` samples of the split in loader order, and write the pictures into ``--save_dir``.

Per batch one forward, one ``sheets.seg_confidence`` launch (label map and per-pixel confidence, csrc/segvis.hip) and one
``metrics.per_image_stats`` launch (csrc/segeval.hip); the collected tensors stay on the device, and every picture is
one ``sheets.render_seg_sheet`` launch whose uint8 sheet is read back and encoded once by Pillow.  matplotlib is not
used: a sheet is at the native resolution of the tensors, its bytes are a function of the inputs alone, and it
carries no titles, legend or colour bar -- the text is in the JSON files beside it:

``prediction_{i:03d}_{name}.png``  one per sample (the reference's name)
``predictions_grid.png``           the first rows x cols samples of ``--grid_size``, ``cols`` samples per sheet row
``visualizations.json``            (build-only) class names with their palette colours -- the legend --, the panel order
                                   of both kinds of picture, and per sample its path, file and the reference's
                                   ``compute_prediction_stats`` dict (``metrics.image_prediction_stats``)
``class_distribution.json``        (build-only, in place of the reference's bar chart ``class_distribution.png``) per
                                   class the truth and prediction pixel counts over the collected samples: the row and
                                   column sums of the summed confusion matrices.  Pixels whose truth lies outside
                                   0..C-1 are left out of both, as ``image_prediction_stats`` documents
"""
from __future__ import annotations

import json
import os
import random
import tempfile

import torch

GUTTER = 4                  # pixels of white between panels
OVERLAY_ALPHA = 0.4         # reference visualize.py:138-139

# the panels of a picture by name -> the sheets.render_seg_sheet column
_COLUMNS = {"image": lambda s, a: ("image",),
            "truth": lambda s, a: ("classes", s["masks"]),
            "prediction": lambda s, a: ("classes", s["labels"]),
            "confidence": lambda s, a: ("lut", s["conf"]),
            "overlay_truth": lambda s, a: ("overlay", s["masks"], a),
            "overlay_prediction": lambda s, a: ("overlay", s["labels"], a)}


def vis_flags(size_flags, data_root, save_dir, extra=()):
    """The reference's visualiser flags (visualize.py:20-72 / visualize_kolektorsdd.py:21-73) plus --precision and
    --synthetic."""
    return [("--data_root", dict(type=str, default=data_root)), *size_flags,
            ("--split", dict(type=str, default="test", choices=["test", "val", "train"])),
            ("--model", dict(type=str, default="seg_unet", choices=["unet", "seg_unet"])),
            ("--checkpoint", dict(type=str, required=True)),
            ("--bilinear", dict(action="store_true")),
            ("--dropout", dict(type=float, default=0.1)),
            ("--num_samples", dict(type=int, default=10)),
            ("--batch_size", dict(type=int, default=4)),
            ("--num_workers", dict(type=int, default=4)),
            ("--device", dict(type=str, default="auto")),
            ("--seed", dict(type=int, default=42)),
            ("--save_dir", dict(type=str, default=save_dir)),
            ("--save_individual", dict(action="store_true")),
            ("--save_grid", dict(action="store_true")),
            ("--show_confidence", dict(action="store_true")),
            ("--figsize", dict(type=int, nargs=2, default=[15, 5],
                               help="accepted for the reference's command lines and unused: sheets are written at the "
                                    "native resolution of the tensors")),
            ("--grid_size", dict(type=int, nargs=2, default=[2, 5], help="rows and columns of samples in the grid")),
            *extra,
            # build-only
            ("--precision", dict(type=str, default="fp32", choices=["fp32", "bf16"])),
            ("--synthetic", dict(action="store_true"))]


def collect(model, batches, num_samples, want_conf=True):
    """Eval-mode pass over ``batches`` of (images, masks, paths) device batches until ``num_samples`` samples are held
    (reference visualize.py:351-373).  Returns device tensors ``images`` (n, 3, H, W), ``masks`` int64, ``labels`` uint8,
    ``conf`` float32 or None, ``confusion`` int64 (n, C, C), ``conf_mean`` / ``conf_std`` float64 (n,), and ``paths``;
    None when the split is empty."""
    from . import sheets
    from .metrics import per_image_stats
    model.eval()
    keys = ("images", "masks", "labels", "conf", "confusion", "conf_mean", "conf_std")
    parts, paths = {k: [] for k in keys}, []
    with torch.no_grad():
        for images, masks, batch_paths in batches:
            if len(paths) >= num_samples:
                break
            outputs = model(images)
            labels, conf = sheets.seg_confidence(outputs, labels=True, conf=want_conf)
            st = per_image_stats(outputs, masks)
            take = min(images.shape[0], num_samples - len(paths))
            for k, t in (("images", images), ("masks", masks), ("labels", labels), ("conf", conf),
                         ("confusion", st["confusion"]), ("conf_mean", st["conf_mean"]), ("conf_std", st["conf_std"])):
                if t is not None:
                    parts[k].append(t[:take])
            paths.extend(batch_paths[:take])
    if not paths:
        return None
    out = {k: (torch.cat(v) if v else None) for k, v in parts.items()}
    out["images"] = out["images"].float()
    out["paths"] = paths
    return out


def sample_slice(samples, lo, hi):
    return {k: (v[lo:hi] if v is not None else None) for k, v in samples.items()}


def sheet(samples, panels, palette, per_row=1, alpha=OVERLAY_ALPHA):
    """One ``sheets.render_seg_sheet`` launch: the named ``panels`` of every sample of ``samples``, a device tensor."""
    from . import sheets
    return sheets.render_seg_sheet(samples["images"], [_COLUMNS[p](samples, alpha) for p in panels], gutter=GUTTER,
                                per_row=per_row, palette=palette)


def save_png(sheet_u8, path):
    from PIL import Image
    Image.fromarray(sheet_u8.cpu().numpy()).save(path)


def run(args, title, split_loader, batches, class_names_of, style, log=print):
    """The visualiser body.  split_loader(args) -> (loader of the --split, num_classes); batches(loader, device) ->
    iterable of (images, masks, paths) device batches; class_names_of(dataset, num_classes) -> names; style:
    ``palette`` (the sheets.class_palette mode), ``individual`` / ``grid`` (panel names), ``save_individual`` /
    ``save_grid`` (bools)."""
    from . import sheets
    from .metrics import image_prediction_stats
    from .train_gear import build_seg_model
    from .utils import load_checkpoint

    random.seed(args.seed)
    torch.manual_seed(args.seed)
    log(f"{title} PREDICTION VISUALIZATION")
    log(f"Using device: {args.device_resolved}")
    log("Creating data loader...")
    loader, num_classes = split_loader(args)
    class_names = class_names_of(loader.dataset, num_classes)
    log(f"Visualizing {args.split} set ({len(loader.dataset)} samples)")
    log(f"Number of classes: {num_classes}")
    log(f"Class names: {class_names}")

    device = args.device_resolved
    model = build_seg_model(args, num_classes, device)
    log(f"Loading checkpoint from: {args.checkpoint}")
    epoch, loss = load_checkpoint(model, None, args.checkpoint, device)
    log(f"Loaded checkpoint from epoch {epoch} with loss {loss:.4f}")

    log("Generating predictions...")
    samples = collect(model, batches(loader, device), args.num_samples, want_conf="confidence" in style["individual"])
    if samples is None:
        raise SystemExit(f"the {args.split} split of {args.data_root} has no samples")
    n = len(samples["paths"])
    log(f"Collected {n} samples for visualization")

    host_palette = sheets.class_palette(num_classes, style["palette"])
    palette = host_palette.to(device)
    stats = [image_prediction_stats(cm, mu, sd, class_names)
             for cm, mu, sd in zip(samples["confusion"].cpu().numpy(), samples["conf_mean"].tolist(),
                                   samples["conf_std"].tolist())]
    entries = [{"index": i, "image_path": p, "file": None, "stats": s} for i, (p, s) in enumerate(zip(samples["paths"], stats))]

    if style["save_individual"]:
        log("Generating individual visualizations...")
        for i, e in enumerate(entries):
            e["file"] = f"prediction_{i:03d}_{os.path.basename(e['image_path']).split('.')[0]}.png"
            save_png(sheet(sample_slice(samples, i, i + 1), style["individual"], palette),
                     os.path.join(args.save_dir, e["file"]))
            log(f"Sample {i + 1}: Accuracy={e['stats']['accuracy']:.3f}, "
                f"Confidence={e['stats']['confidence_mean']:.3f}+/-{e['stats']['confidence_std']:.3f}")

    grid = None
    if style["save_grid"]:
        log("Generating grid visualization...")
        rows, cols = args.grid_size
        shown = min(rows * cols, n)
        save_png(sheet(sample_slice(samples, 0, shown), style["grid"], palette, per_row=cols),
                 os.path.join(args.save_dir, "predictions_grid.png"))
        grid = {"file": "predictions_grid.png", "grid_size": [rows, cols], "samples": shown}

    colours = host_palette[:num_classes].tolist()
    summary = {"split": args.split, "checkpoint": args.checkpoint,
               "classes": [{"index": i, "name": name, "rgb": colours[i]} for i, name in enumerate(class_names[:num_classes])],
               "palette_mode": style["palette"], "overlay_alpha": OVERLAY_ALPHA, "gutter": GUTTER,
               "panels": {"individual": list(style["individual"]), "grid": list(style["grid"])},
               "image_size": list(samples["images"].shape[2:]), "grid": grid, "samples": entries}
    with open(os.path.join(args.save_dir, "visualizations.json"), "w") as f:
        json.dump(summary, f, indent=2)

    total = samples["confusion"].sum(0).cpu().numpy()
    names = [class_names[i] if i < len(class_names) else f"class_{i}" for i in range(num_classes)]
    dist = {"samples": n,
            "note": "pixel counts over the collected samples; pixels whose truth is outside 0..C-1 are in neither list",
            "class_names": names,
            "ground_truth": [int(v) for v in total.sum(axis=1)],
            "prediction": [int(v) for v in total.sum(axis=0)]}
    dist_path = os.path.join(args.save_dir, "class_distribution.json")
    with open(dist_path, "w") as f:
        json.dump(dist, f, indent=2)
    log(f"Class distribution saved to: {dist_path}")
    log(f"All visualizations saved to: {args.save_dir}")
    return args.save_dir


def prepare(args, write_synthetic, prefix):
    """What both CLIs do before anything is logged or computed: refuse a CPU device and a --grid_size or --num_samples
    below 1, make the --synthetic tree."""
    from .train_gear import require_gpu
    args.device_resolved = require_gpu(args)
    rows, cols = args.grid_size
    if rows < 1 or cols < 1:
        raise SystemExit(f"--grid_size {rows} {cols}: rows and columns are at least 1")
    if args.num_samples < 1:
        raise SystemExit(f"--num_samples {args.num_samples}: at least 1")
    if args.synthetic:
        args.data_root = write_synthetic(tempfile.mkdtemp(prefix=prefix), seed=args.seed)
    return args
