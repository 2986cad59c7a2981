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

from . import seg_cli
from .predict import FLAGS as PREDICT_FLAGS
from .predict import TASKS

FLAGS = [(name, kw) for name, kw in PREDICT_FLAGS if name not in ("--image_size", "--mask_size")] + [
    ("--tile", dict(type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="the tile the model runs at; default: the task's trainer frame")),
    ("--min_overlap", dict(type=int, default=64, help="pixels neighbouring tiles share at least")),
    ("--scale", dict(type=float, default=1.0, help="the working frame is the image scaled by this (0 < S <= 4)"))]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="predict at full resolution: overlapping tiles blended on the GPU")
    for name, kw in FLAGS + seg_cli.BUILD_FLAGS:
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    seg_cli.check_tile_scale(ap, args, TASKS[args.task]["image_size"])
    seg_cli.check_predict_flags(ap, args)
    seg_cli.check_shape_flags(ap, args)
    seg_cli.check_polygon_flags(ap, args)
    seg_cli.check_group_flags(ap, args)
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
    task = TASKS[args.task]
    device, paths, names, num_classes, class_names, model = seg_cli.open_prediction(args, task, "TILED PREDICTION",
                                                                                    "blend")
    from .predict import image_loader
    from .tiling import TiledPredictor

    print(f"Tile: {args.tile}  min overlap: {args.min_overlap}  scale: {args.scale}")
    predictor = TiledPredictor(model, args.tile, args.min_overlap, args.batch_size)
    outputs = seg_cli.prediction_outputs(args, task, num_classes, device)
    images = [None] * len(paths)
    for batch, idx in image_loader(paths, 1, args.num_workers):
        image, i = batch[0], idx[0]
        original = (int(image.shape[0]), int(image.shape[1]))
        x = load_frame(image, working_frame(original, args.scale), device)
        labels, conf, plan = predictor(x)
        records, shapes, traced, fragments = seg_cli.describe_regions(args, labels[None], num_classes, conf[None])
        images[i] = seg_cli.save_frame_prediction(args, outputs, paths[i], names[i], original, labels, conf, records,
                                                  class_names, {"tiling": plan}, frame=x, shapes=shapes, traced=traced,
                                                  fragments=fragments)

    def tiles(im):
        return f"in {len(im['tiling']['origins_y']) * len(im['tiling']['origins_x'])} tiles"

    return seg_cli.write_predictions(args, class_names, images, middle=tiles)


if __name__ == "__main__":
    main()
