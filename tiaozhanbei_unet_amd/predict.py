#!/usr/bin/env python3
"""Run a trained Gear or KolektorSDD segmentation checkpoint on images that have NO labels (no reference counterpart):
which defects the model sees in each, where, how large and how sure it is, and whether the part would be rejected.

    python -m tiaozhanbei_unet_amd.predict --task gear --checkpoint best_model.pth --input photos/ [--save_overlays]
    python -m tiaozhanbei_unet_amd.predict --task kolektorsdd --checkpoint best_model.pth --input part.jpg

``--input`` is one image or a directory, walked recursively in sorted order (jpg / jpeg / png / bmp; ``*_label.bmp`` is
skipped).  Workers decode to RGB uint8; per batch ``augment.DeviceTransform`` resizes and normalises on the GPU (images
of different sizes are grouped as the loaders' raw batches are), the model runs in eval mode, ``sheets.seg_confidence``
gives the label map and the per-pixel confidence, and ``evaluation.describe_class_regions`` (csrc/defects.hip) one record
per predicted 8-connected class region of at least ``--min_region_pixels`` pixels.  Writes into ``--output_dir``:

``predictions.json``   ``args``, ``class_names``, ``frame_size`` [H, W], ``images`` (input order: ``image_path``, ``name``,
                       ``original_size`` [H0, W0], ``mean_confidence`` of the whole frame, ``defect_pixels`` per class name
                       over the listed defects, ``defects`` and ``decision``: defects.defect_entries) and ``summary``
``masks/<name>.png``   the label map, Pillow mode P with the ``sheets.class_palette`` colours; ``--mask_size original``
                       (default) upsamples it to the image's own size on the device (NEAREST), ``frame`` keeps the frame
``overlays/<name>.png``  with ``--save_overlays``: image | image with the prediction overlaid, as ``visualize_gear`` draws it

``<name>`` is the image's path relative to ``--input`` with the separators replaced by ``__``.  An image is rejected iff
it has a defect of one of ``--reject_classes`` (default: every class but the background) whose mean confidence is at
least ``--min_confidence``; defects below it stay listed with ``"counted": false``.  Nothing here claims any accuracy:
the numbers are what the given checkpoint predicts.

Build-only, off by default (``seg_cli.SHAPE_FLAGS``, shared with ``predict_tiled`` and ``predict_views``):
``--measure_shapes`` adds a ``shape`` dict to every defect (``defects.shape_measures`` of the integer records of
``evaluation.measure_class_regions``, csrc/shapes.hip: Feret length / width / angle, equivalent ellipse, perimeter,
circularity, holes; lengths in the image's own pixels, and with ``--pixel_size MM`` in millimetres too);
``--min_defect_length X`` / ``--min_defect_area X`` (mm and mm2 with ``--pixel_size``, image pixels otherwise; either implies
``--measure_shapes``) make ``counted`` also require that length and that area, and a ``size_rules`` block records them.
With none of the four nothing new is launched and every output byte is as before.

Build-only, off by default too (``seg_cli.POLYGON_FLAGS``, shared likewise): ``--save_polygons`` traces every defect's
outline on the GPU (``evaluation.trace_class_regions``, csrc/contours.hip, on the labelling the records come from) and
writes ``labels/<name>.txt`` beside ``masks/``: the defects with ``"counted": true`` as polygons in the Gear label format
(``class - 1`` then ``(x + 0.5) / W (y + 0.5) / H`` per point: ``polygons.gear_label_lines``), which ``gear_dataset``, the
trainers, ``analyze_gear_overlaps`` and the ``eval_*`` tools read and a labelling tool can correct.  Pillow's polygon of a
written outline is the predicted region with its holes filled.  Every defect of ``predictions.json`` gains ``outline``
([[x, y], ...] in frame pixels), ``outline_original`` and ``hole_outlines``, and a ``polygon_rules`` block records
``--polygon_tolerance T`` (frame pixels, default 0; implies ``--save_polygons``), by which ``polygons.simplify_closed`` thins
every outline.  Two limits come with the format: it has no holes, so a hole is filled when the file is loaded, and the
loader resolves overlaps by class priority (spalling > pitting > scrape), not by nesting, so a lower-priority defect
inside a higher one's hole is overwritten.  The GPU mask kernel of the loader takes at most 512 points a polygon: thin
longer outlines with ``--polygon_tolerance``.

Build-only, off by default too (``seg_cli.GROUP_FLAGS``, shared likewise): ``--merge_gap PX`` (2..32 FRAME pixels, which
this tool squeezes anisotropically from the image) counts the regions of one class that come within PX pixels of each
other as ONE defect (``evaluation.group_class_regions``, csrc/groups.hip; regions below ``--min_region_pixels`` are dropped
first and bridge nothing).  ``pixels``, ``bbox``, the confidences, ``shape`` and the size rules are then those of the
whole group; every defect gains ``fragments`` ([{"root": [x, y], "pixels": s}] in root order) and, with the polygon flags,
``fragment_outlines``, and ``labels/<name>.txt`` holds one line per fragment.  ``shape.perimeter`` is the sum over the
fragments and ``shape.circularity`` of several fragments is not a roundness.  A ``grouping_rules`` block records the gap.
"""
from __future__ import annotations

import argparse
import os

from . import defects, polygons, seg_cli
from .seg_cli import HEAD_WEIGHT  # noqa: F401  (its home; importable from here as before)

TASKS = {"gear": {"image_size": (512, 512), "class_names": ["background", "pitting", "spalling", "scrape"],
                  "palette": "index"},
         "kolektorsdd": {"image_size": (1024, 512), "class_names": ["background", "defect_type_1", "defect_type_2"],
                         "palette": "scaled"}}

FLAGS = [("--task", dict(type=str, required=True, choices=sorted(TASKS))),
         ("--checkpoint", dict(type=str, required=True)),
         ("--input", dict(type=str, required=True, help="an image file or a directory of images")),
         ("--output_dir", dict(type=str, default="predictions")),
         ("--image_size", dict(type=int, nargs=2, default=None, metavar=("H", "W"),
                               help="the frame the model runs at; default: the task's trainer default")),
         ("--model", dict(type=str, default="seg_unet", choices=["unet", "seg_unet"])),
         ("--bilinear", dict(action="store_true")),
         ("--dropout", dict(type=float, default=0.1)),
         ("--precision", dict(type=str, default="fp32", choices=["fp32", "bf16"])),
         ("--batch_size", dict(type=int, default=8)),
         ("--num_workers", dict(type=int, default=4)),
         ("--device", dict(type=str, default="auto")),
         ("--num_classes", dict(type=int, default=None, help="default: the rows of the checkpoint's head weight")),
         ("--class_names", dict(type=str, nargs="+", default=None)),
         ("--min_region_pixels", dict(type=int, default=1)),
         ("--min_confidence", dict(type=float, default=0.0)),
         ("--reject_classes", dict(type=str, nargs="+", default=None, help="default: every class but the background")),
         ("--mask_size", dict(type=str, default="original", choices=["original", "frame"])),
         ("--save_overlays", dict(action="store_true"))]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Defects with boxes and confidence from unlabelled images (MI355X HIP path)")
    for name, kw in FLAGS + seg_cli.BUILD_FLAGS:
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    if args.image_size is None:
        args.image_size = list(TASKS[args.task]["image_size"])
    if min(args.image_size) < 1:
        ap.error("--image_size must be positive")
    seg_cli.check_predict_flags(ap, args)
    seg_cli.check_shape_flags(ap, args)
    seg_cli.check_polygon_flags(ap, args)
    seg_cli.check_group_flags(ap, args)
    return args


class ImageFiles:
    """A map-style dataset over image paths: (decoded RGB uint8 [H, W, 3] tensor, index)."""

    def __init__(self, paths):
        self.paths = list(paths)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, idx):
        import numpy as np
        import torch
        from PIL import Image
        with Image.open(self.paths[idx]) as im:
            return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)), idx


def collate_images(samples):
    """(images, indices): images stacked when they share a size, a list otherwise (gear_dataset.collate_raw's rule)."""
    import torch
    imgs, idx = zip(*samples)
    same = len({tuple(t.shape) for t in imgs}) == 1
    return (torch.stack(imgs) if same else list(imgs)), list(idx)


def predict_batches(model, loader, size, num_classes, min_pixels, device, directions=None, contours=False, merge_gap=0):
    """Eval-mode pass over ``collate_images`` batches.  Yields per batch (indices, original sizes [(H0, W0)], normalised
    images, labels uint8 [N, H, W], frame mean confidence list, the batch's ``evaluation.RegionRecords``).  The records
    and the means are the batch's host reads.  ``.records`` is always there; ``directions`` (a number of Feret directions)
    fills ``.shapes``, ``contours`` fills ``.loops`` and ``.points``, and ``merge_gap`` fills ``.fragments`` and makes the
    records and shapes those of the groups: one labelling, the same reads, None for what was not asked for.  ``image`` is
    the dataset index in every member that has the column: records, shapes, loops and fragments."""
    import numpy as np
    import torch
    from . import sheets
    from .augment import DeviceTransform
    from .evaluation import class_region_records
    from .metrics import per_image_stats
    tf = DeviceTransform(tuple(size), train=False)
    model.eval()
    with torch.no_grad():
        for images, idx in loader:
            sizes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
            x = tf(images, None, device=device)
            logits = model(x)
            labels, conf = sheets.seg_confidence(logits)
            means = per_image_stats(logits)["conf_mean"]
            got = class_region_records(labels, num_classes, conf, min_pixels, directions=directions, contours=contours,
                                       merge_gap=merge_gap)
            for rec in (got.records, got.shapes, got.loops, got.fragments):      # ``points`` has no image column
                if rec is not None:
                    rec[:, 0] = np.asarray(idx, np.int64)[rec[:, 0]]
            yield idx, sizes, x, labels, means.tolist(), got


def image_loader(paths, batch_size, num_workers):
    """``collate_images`` batches of ``ImageFiles(paths)``, in order"""
    from torch.utils.data import DataLoader
    return DataLoader(ImageFiles(paths), batch_size=batch_size, shuffle=False, num_workers=num_workers, pin_memory=True,
                      collate_fn=collate_images)


def main(argv=None):
    args = parse_args(argv)
    task = TASKS[args.task]
    device, paths, names, num_classes, class_names, model = seg_cli.open_prediction(args, task, "PREDICTION", "confidence")
    import numpy as np
    from . import augment

    mask_dir, overlay_dir, palette, palette_bytes = seg_cli.prediction_outputs(args, task, num_classes, device)
    loader = image_loader(paths, args.batch_size, args.num_workers)
    originals, frame_means, records, shapes, traced = [None] * len(paths), [None] * len(paths), [], [], {}
    rules, polygon_rules = seg_cli.size_rules_of(args), seg_cli.polygon_rules_of(args)
    merge_gap, fragments = getattr(args, "merge_gap", 0), []
    for idx, sizes, x, labels, means, got in predict_batches(model, loader, args.image_size, num_classes,
                                                             args.min_region_pixels, device,
                                                             None if rules is None else seg_cli.DIRECTIONS,
                                                             polygon_rules is not None, merge_gap):
        records.append(got.records)
        if rules is not None:
            shapes.append(got.shapes)
        if polygon_rules is not None:
            traced.update(polygons.outlines(got.loops, got.points, got.fragments))
        if merge_gap:
            fragments.append(got.fragments)
        if args.mask_size == "frame":
            host = labels.cpu().numpy()
        for k, i in enumerate(idx):
            originals[i], frame_means[i] = sizes[k], means[k]
            if args.mask_size == "frame":
                mask = host[k]
            else:
                mask = augment.resize_nearest_u8(labels[k:k + 1].unsqueeze(-1), *sizes[k])[0, :, :, 0].cpu().numpy()
            seg_cli.save_mask(mask, palette_bytes, os.path.join(mask_dir, names[i] + ".png"))
            if args.save_overlays:
                seg_cli.save_overlay(x[k:k + 1].float(), labels[k:k + 1], palette,
                                     os.path.join(overlay_dir, names[i] + ".png"))

    entries = defects.defect_entries(np.concatenate(records), class_names, args.image_size, originals,
                                     args.min_confidence, args.reject_classes,
                                     np.concatenate(shapes) if shapes else None, rules,
                                     **({"fragments": np.concatenate(fragments)} if merge_gap else {}))
    if polygon_rules is not None:
        polygons.attach_outlines(entries, np.concatenate(records), traced, args.image_size, originals,
                                 args.polygon_tolerance)
        for i, e in enumerate(entries):
            seg_cli.save_label_file(args, names[i], e, args.image_size)
    images = []
    for i, e in enumerate(entries):
        pixels = {name: 0 for name in class_names[1:]}
        for d in e["defects"]:
            pixels[d["class_name"]] += d["pixels"]
        images.append({"image_path": paths[i], "name": names[i], "original_size": list(originals[i]),
                       "mean_confidence": frame_means[i], "defect_pixels": pixels, **e})
    return seg_cli.write_predictions(args, class_names, images, frame_size=args.image_size)


if __name__ == "__main__":
    main()
