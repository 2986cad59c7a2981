#!/usr/bin/env python3
"""``predict`` at the image's own resolution (no reference counterpart): every image is cut into overlapping tiles of the
size the model was trained at, and the tile logits are blended into one label map and one confidence map on the GPU.

    python -m tiaozhanbei_unet_amd.predict_tiled --task gear --checkpoint best_model.pth --input photos/
    python -m tiaozhanbei_unet_amd.predict_tiled --task gear --checkpoint best_model.pth --input photos/ --scale 0.5

``predict`` squeezes a 1920 x 1080 Gear image into one 512 x 512 frame; here the working frame of an image of H0 x W0
is (round(H0 S), round(W0 S)) for ``--scale S`` (default 1: the image itself, only normalised; otherwise resized on the
device with the Pillow-exact bilinear path).  ``tiling.TiledPredictor`` covers the frame with tiles of ``--tile H W``
(default: the task's trainer frame) whose neighbours overlap by at least ``--min_overlap`` pixels, runs the model on
``--batch_size`` tiles per call and blends the logits (csrc/tiles.hip); the regions, the records and the decision are
``predict``'s (``evaluation.describe_class_regions``, ``defects.defect_entries``).  Images are processed one at a time.

A checkpoint trained on squeezed frames sees objects at another scale at ``--scale 1`` than it was trained on; ``--scale``
exists for that (for Gear, 512 / 1920 ~ 0.27 horizontally reproduces the training scale along x).  Whether tiling finds
more real defects than ``predict`` has not been measured.

Writes into ``--output_dir`` what ``predict`` writes, with these differences: in ``predictions.json`` ``frame_size`` sits in
each image's entry, beside a ``tiling`` block ``{"tile": [th, tw], "origins_y", "origins_x", "ramp": [by, bx]}``;
``masks/<name>.png`` is the frame's label map, which at ``--scale 1`` already has the image's size and is otherwise
upsampled to it (NEAREST).  Boxes and centroids are reported in the frame and in the image's own pixels.
"""
from __future__ import annotations

import argparse
import json
import os

from . import defects
from .predict import FLAGS as PREDICT_FLAGS
from .predict import HEAD_WEIGHT, TASKS

FLAGS = [(name, kw) for name, kw in PREDICT_FLAGS if name not in ("--image_size", "--mask_size")] + [
    ("--tile", dict(type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="the tile the model runs at; default: the task's trainer frame")),
    ("--min_overlap", dict(type=int, default=64, help="pixels neighbouring tiles share at least")),
    ("--scale", dict(type=float, default=1.0, help="the working frame is the image scaled by this (0 < S <= 4)"))]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="predict at full resolution: overlapping tiles blended on the GPU")
    for name, kw in FLAGS:
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    if args.tile is None:
        args.tile = list(TASKS[args.task]["image_size"])
    if min(args.tile) < 1:
        ap.error("--tile must be positive")
    if not 0 <= args.min_overlap < min(args.tile):
        ap.error("--min_overlap must be at least 0 and smaller than both tile sides")
    if not 0.0 < args.scale <= 4.0:
        ap.error("--scale must lie in (0, 4]")
    if args.min_region_pixels < 1:
        ap.error("--min_region_pixels must be at least 1")
    if not 0.0 <= args.min_confidence <= 1.0:
        ap.error("--min_confidence must lie in 0..1")
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    return args


def working_frame(original_hw, scale):
    """(round(H0 S), round(W0 S)), at least 1 x 1"""
    return tuple(max(1, int(round(v * scale))) for v in original_hw)


def load_frame(image_u8, frame_hw, device):
    """The normalised float32 frame (3, H, W) of a decoded uint8 (H0, W0, 3) image: resized (Pillow's bilinear) only
    when the frame differs from the image."""
    from . import augment
    x = image_u8.to(device, non_blocking=True).unsqueeze(0)
    if tuple(x.shape[1:3]) != tuple(frame_hw):
        x = augment.resize_bilinear_u8(x, *frame_hw)
    return augment.color_jitter_normalize_u8(x)[0]


def main(argv=None):
    args = parse_args(argv)
    from .train_gear import build_seg_model, require_gpu
    device = require_gpu(args)
    import torch
    from torch.utils.data import DataLoader
    from . import augment, sheets
    from .evaluation import describe_class_regions
    from .predict import ImageFiles, _save_mask, collate_images
    from .seg_visualize import GUTTER, OVERLAY_ALPHA, save_png
    from .tiling import TiledPredictor

    task = TASKS[args.task]
    paths = defects.list_images(args.input)
    if not paths:
        raise SystemExit(f"no image files below {args.input}")
    names = defects.output_names(paths, args.input)
    ckpt = torch.load(args.checkpoint, map_location=device, weights_only=True)
    state = ckpt["model_state_dict"]
    if args.num_classes is None:
        if HEAD_WEIGHT not in state:
            raise SystemExit(f"{args.checkpoint} has no {HEAD_WEIGHT}: pass --num_classes")
        args.num_classes = int(state[HEAD_WEIGHT].shape[0])
    num_classes = args.num_classes
    if not 2 <= num_classes <= 8:
        raise SystemExit(f"{num_classes} classes: the blend kernel takes 2 to 8")
    class_names = defects.class_names_for(task["class_names"], num_classes, args.class_names)
    unknown = sorted(set(args.reject_classes or ()) - set(class_names))
    if unknown:
        raise SystemExit(f"--reject_classes {unknown}: the classes are {class_names}")
    print("=" * 60 + f"\n{args.task.upper()} TILED PREDICTION\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nImages: {len(paths)}")
    print(f"Number of classes: {num_classes}\nClass names: {class_names}")
    print(f"Tile: {args.tile}  min overlap: {args.min_overlap}  scale: {args.scale}")
    model = build_seg_model(args, num_classes, device)
    model.load_state_dict(state)
    predictor = TiledPredictor(model, args.tile, args.min_overlap, args.batch_size)

    mask_dir = os.path.join(args.output_dir, "masks")
    os.makedirs(mask_dir, exist_ok=True)
    overlay_dir = os.path.join(args.output_dir, "overlays")
    if args.save_overlays:
        os.makedirs(overlay_dir, exist_ok=True)
    host_palette = sheets.class_palette(num_classes, task["palette"])
    palette, palette_bytes = host_palette.to(device), host_palette.numpy().tobytes()
    loader = DataLoader(ImageFiles(paths), batch_size=1, shuffle=False, num_workers=args.num_workers, pin_memory=True,
                        collate_fn=collate_images)
    images = [None] * len(paths)
    for batch, idx in loader:
        image, i = batch[0], idx[0]
        original = (int(image.shape[0]), int(image.shape[1]))
        frame_hw = working_frame(original, args.scale)
        x = load_frame(image, frame_hw, device)
        labels, conf, plan = predictor(x)
        records = describe_class_regions(labels[None], num_classes, conf[None], args.min_region_pixels)
        (entry,) = defects.defect_entries(records, class_names, frame_hw, [original], args.min_confidence,
                                          args.reject_classes)
        pixels = {name: 0 for name in class_names[1:]}
        for d in entry["defects"]:
            pixels[d["class_name"]] += d["pixels"]
        images[i] = {"image_path": paths[i], "name": names[i], "original_size": list(original),
                     "frame_size": list(frame_hw), "tiling": plan, "mean_confidence": float(conf.double().mean()),
                     "defect_pixels": pixels, **entry}
        mask = labels if frame_hw == original else augment.resize_nearest_u8(labels[None, :, :, None], *original)[0, :, :, 0]
        _save_mask(mask.cpu().numpy(), palette_bytes, os.path.join(mask_dir, names[i] + ".png"))
        if args.save_overlays:
            sheet = sheets.render_seg_sheet(x[None], [("image",), ("overlay", labels[None], OVERLAY_ALPHA)], gutter=GUTTER,
                                            palette=palette)
            save_png(sheet, os.path.join(overlay_dir, names[i] + ".png"))

    summary = defects.summarize(images, class_names)
    out_path = os.path.join(args.output_dir, "predictions.json")
    with open(out_path, "w") as f:
        json.dump({"args": vars(args), "class_names": class_names, "images": images, "summary": summary}, f, indent=2)
    for im in images:
        found = ", ".join(f"{d['class_name']} {d['pixels']} px @ {d['mean_confidence']:.2f}" for d in im["defects"][:4])
        more = f" (+{len(im['defects']) - 4} more)" if len(im["defects"]) > 4 else ""
        tiles = len(im["tiling"]["origins_y"]) * len(im["tiling"]["origins_x"])
        print(f"{im['decision']:>6}  {im['name']} {im['frame_size'][0]}x{im['frame_size'][1]} in {tiles} tiles: "
              f"{found or 'no defects'}{more}")
    print(f"Images: {summary['images']}  rejected: {summary['rejected']}  defects: {summary['defects']}")
    print(f"Predictions saved to: {out_path}")
    return out_path


if __name__ == "__main__":
    main()
