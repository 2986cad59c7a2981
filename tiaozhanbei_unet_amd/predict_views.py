#!/usr/bin/env python3
"""``predict_tiled`` over several views of every image (no reference counterpart): the model sees the working frame at
each of ``--view_scales``, plain and mirrored as ``--view_flips`` says, and the views' logits are averaged on the GPU.

    python -m tiaozhanbei_unet_amd.predict_views --task gear --checkpoint best_model.pth --input photos/
    python -m tiaozhanbei_unet_amd.predict_views --task gear --checkpoint best_model.pth --input photos/ \
        --view_scales 0.75 1 1.5 --view_flips all

Takes ``predict_tiled``'s flags plus ``--view_scales S [S ...]`` (default 1; each in [0.5, 2] and relative to ``--scale``:
the product must stay in (0, 4]) and ``--view_flips {none,h,v,all}`` (default h: plain and mirrored left / right).  The
output frame of an image is ``predict_tiled``'s working frame; ``views.ViewEnsemble`` resizes the image to every view's
frame, runs ``tiling.TiledPredictor`` on it and merges the logits (csrc/views.hip).  The cost is one ``predict_tiled``
per view.

Writes into ``--output_dir`` what ``predict_tiled`` writes (``tiling`` is the tile plan of the first view); each image's
entry also carries ``views``, the plan (per view: scale, flips, frame size and its tile plan), and each defect
``mean_view_agreement`` in 0..1: the share of the views whose own label at a pixel is the merged one, averaged over the
defect's pixels in the fixed point of ``mean_confidence``.  With ``--view_scales 1 --view_flips none`` the labels, the
confidences, the masks and the defect records are ``predict_tiled``'s.  Whether an ensemble finds more real defects has
not been measured: ``eval_views`` is the tool for that.
"""
from __future__ import annotations

import argparse
import json
import os

from . import defects
from . import views as V
from .predict import HEAD_WEIGHT, TASKS
from .predict_tiled import FLAGS as TILED_FLAGS
from .predict_tiled import working_frame

VIEW_FLAGS = [
    ("--view_scales", dict(type=float, nargs="+", default=[1.0], metavar="S",
                           help="the views' scales relative to --scale, each in [0.5, 2]")),
    ("--view_flips", dict(choices=sorted(V.FLIP_SETS), default="h",
                          help="none; h: plain + mirrored left / right; v: plain + up / down; all: the four of them"))]
FLAGS = TILED_FLAGS + VIEW_FLAGS


def check_views(ap, args, scale=1.0):
    """``args.views`` from the two view flags, or ap.error; ``scale``: the factor the views' scales multiply"""
    try:
        args.views = V.plan_views(args.view_scales, args.view_flips)
    except ValueError as e:
        ap.error(str(e))
    if any(not 0.0 < scale * s <= 4.0 for s in args.view_scales):
        ap.error("--scale times every --view_scales must lie in (0, 4]")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="predict at full resolution from several views merged on the GPU")
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
    check_views(ap, args, args.scale)
    return args


def agreement_means(labels, agreement, n_views, num_classes, min_pixels, records):
    """Per record of ``records`` (``describe_class_regions`` of ``labels`` [N, H, W], sorted by image and root) the mean of
    agreement / n_views over its region, conf_sum_q / (65536 size): one more ``describe_class_regions`` with that ratio
    in the confidence slot, which yields the same regions in the same order."""
    from .evaluation import describe_class_regions
    again = describe_class_regions(labels, num_classes, agreement.float() / float(n_views), min_pixels)
    if again.shape != records.shape or (again[:, :4] != records[:, :4]).any():
        raise RuntimeError("agreement_means: the regions of the two passes differ")
    return [int(r[10]) / (defects.Q_ONE * int(r[3])) for r in again]


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
        raise SystemExit(f"{num_classes} classes: the merge kernel takes 2 to 8")
    class_names = defects.class_names_for(task["class_names"], num_classes, args.class_names)
    unknown = sorted(set(args.reject_classes or ()) - set(class_names))
    if unknown:
        raise SystemExit(f"--reject_classes {unknown}: the classes are {class_names}")
    views = args.views
    print("=" * 60 + f"\n{args.task.upper()} VIEW-ENSEMBLE PREDICTION\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nImages: {len(paths)}")
    print(f"Number of classes: {num_classes}\nClass names: {class_names}")
    print(f"Tile: {args.tile}  min overlap: {args.min_overlap}  scale: {args.scale}")
    print(f"Views: {len(views)} (scales {args.view_scales}, flips {args.view_flips})")
    model = build_seg_model(args, num_classes, device)
    model.load_state_dict(state)
    ensemble = V.ViewEnsemble(TiledPredictor(model, args.tile, args.min_overlap, args.batch_size), views)

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
        image, i = batch[0].to(device, non_blocking=True), idx[0]
        original = (int(image.shape[0]), int(image.shape[1]))
        frame_hw = working_frame(original, args.scale)
        labels, conf, agreement, plan = ensemble(image, frame_hw)
        records = describe_class_regions(labels[None], num_classes, conf[None], args.min_region_pixels)
        (entry,) = defects.defect_entries(records, class_names, frame_hw, [original], args.min_confidence,
                                          args.reject_classes)
        agree = agreement_means(labels[None], agreement[None], len(views), num_classes, args.min_region_pixels, records)
        pixels = {name: 0 for name in class_names[1:]}
        for d, share in zip(entry["defects"], agree):           # defect_entries keeps the records' order: by root
            d["mean_view_agreement"] = share
            pixels[d["class_name"]] += d["pixels"]
        images[i] = {"image_path": paths[i], "name": names[i], "original_size": list(original),
                     "frame_size": list(frame_hw), "tiling": plan[0]["tiling"], "views": plan, "mean_confidence": float(conf.double().mean()),
                     "defect_pixels": pixels, **entry}
        mask = labels if frame_hw == original else augment.resize_nearest_u8(labels[None, :, :, None], *original)[0, :, :, 0]
        _save_mask(mask.cpu().numpy(), palette_bytes, os.path.join(mask_dir, names[i] + ".png"))
        if args.save_overlays:
            from .predict_tiled import load_frame
            x = load_frame(image, frame_hw, device)
            sheet = sheets.render_seg_sheet(x[None], [("image",), ("overlay", labels[None], OVERLAY_ALPHA)], gutter=GUTTER,
                                            palette=palette)
            save_png(sheet, os.path.join(overlay_dir, names[i] + ".png"))

    summary = defects.summarize(images, class_names)
    out_path = os.path.join(args.output_dir, "predictions.json")
    with open(out_path, "w") as f:
        json.dump({"args": vars(args), "class_names": class_names, "images": images, "summary": summary}, f, indent=2)
    for im in images:
        found = ", ".join(f"{d['class_name']} {d['pixels']} px @ {d['mean_confidence']:.2f} (views {d['mean_view_agreement']:.2f})"
                          for d in im["defects"][:4])
        more = f" (+{len(im['defects']) - 4} more)" if len(im["defects"]) > 4 else ""
        print(f"{im['decision']:>6}  {im['name']} {im['frame_size'][0]}x{im['frame_size'][1]} in {len(im['views'])} views: "
              f"{found or 'no defects'}{more}")
    print(f"Images: {summary['images']}  rejected: {summary['rejected']}  defects: {summary['defects']}")
    print(f"Predictions saved to: {out_path}")
    return out_path


if __name__ == "__main__":
    main()
