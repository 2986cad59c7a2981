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

from . import defects, seg_cli
from . import views as V
from .predict import TASKS
from .predict_tiled import FLAGS as TILED_FLAGS
from .predict_tiled import load_frame, working_frame

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
    for name, kw in FLAGS + seg_cli.BUILD_FLAGS:
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    seg_cli.check_tile_scale(ap, args, TASKS[args.task]["image_size"])
    seg_cli.check_predict_flags(ap, args)
    seg_cli.check_shape_flags(ap, args)
    seg_cli.check_polygon_flags(ap, args)
    seg_cli.check_group_flags(ap, args)
    check_views(ap, args, args.scale)
    return args


def agreement_means(labels, agreement, n_views, num_classes, min_pixels, records, merge_gap=0):
    """Per record of ``records`` (``describe_class_regions`` of ``labels`` [N, H, W], sorted by image and root) the mean of
    agreement / n_views over its region, conf_sum_q / (65536 size): one more ``describe_class_regions`` with that ratio
    in the confidence slot, which yields the same regions in the same order.  ``merge_gap``: the gap the records were
    grouped with (0: not grouped), so that the rows still align."""
    from .evaluation import describe_class_regions
    again = describe_class_regions(labels, num_classes, agreement.float() / float(n_views), min_pixels, merge_gap=merge_gap)
    if merge_gap:
        again = again[0]
    if again.shape != records.shape or (again[:, :4] != records[:, :4]).any():
        raise RuntimeError("agreement_means: the regions of the two passes differ")
    return [int(r[10]) / (defects.Q_ONE * int(r[3])) for r in again]


def main(argv=None):
    args = parse_args(argv)
    task, views = TASKS[args.task], args.views
    device, paths, names, num_classes, class_names, model = seg_cli.open_prediction(args, task, "VIEW-ENSEMBLE PREDICTION",
                                                                                    "merge")
    from .predict import image_loader
    from .tiling import TiledPredictor

    print(f"Tile: {args.tile}  min overlap: {args.min_overlap}  scale: {args.scale}")
    print(f"Views: {len(views)} (scales {args.view_scales}, flips {args.view_flips})")
    ensemble = V.ViewEnsemble(TiledPredictor(model, args.tile, args.min_overlap, args.batch_size), views)
    outputs = seg_cli.prediction_outputs(args, task, num_classes, device)
    images = [None] * len(paths)
    for batch, idx in image_loader(paths, 1, args.num_workers):
        image, i = batch[0].to(device, non_blocking=True), idx[0]
        original = (int(image.shape[0]), int(image.shape[1]))
        frame_hw = working_frame(original, args.scale)
        labels, conf, agreement, plan = ensemble(image, frame_hw)
        records, shapes, traced, fragments = seg_cli.describe_regions(args, labels[None], num_classes, conf[None])
        agree = agreement_means(labels[None], agreement[None], len(views), num_classes, args.min_region_pixels, records,
                                getattr(args, "merge_gap", 0))
        frame = load_frame(image, frame_hw, device) if args.save_overlays else None
        images[i] = seg_cli.save_frame_prediction(args, outputs, paths[i], names[i], original, labels, conf, records,
                                                  class_names, {"tiling": plan[0]["tiling"], "views": plan}, frame=frame,
                                                  defect_extras={"mean_view_agreement": agree}, shapes=shapes, traced=traced,
                                                  fragments=fragments)
    return seg_cli.write_predictions(args, class_names, images, middle=lambda im: f"in {len(im['views'])} views")


if __name__ == "__main__":
    main()
