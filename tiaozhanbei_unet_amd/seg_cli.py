"""What the command-line tools over a Gear / KolektorSDD segmentation checkpoint share (no reference counterpart).  The
tools keep what is their own -- their extra flags, their meter, their host-side summary and their output files -- and take
the rest from here, as plain functions and generators:

the ``eval_*`` side   ``parse_dataset_args`` (``--dataset`` first, then that data set's flags: ``cli_of``, ``base_flags``),
                      ``TILING_FLAGS`` with ``frame_of`` / ``mode_of``, the refusals ``check_tiling`` and
                      ``check_region_flags``, ``open_checkpoint_session`` (device, banner, loader, class names, model,
                      checkpoint), ``tiled_predictor``, the full-resolution walk ``full_resolution_images`` /
                      ``normalized_frame``, and the labelled-prediction sources ``frame_predictions`` /
                      ``tiled_predictions`` (``labelled_predictions`` picks one by ``--tiled``)
the ``predict*`` side the refusals ``check_predict_flags`` and ``check_tile_scale``, the build-only flags ``BUILD_FLAGS``:
                      the shape flags (``SHAPE_FLAGS``, ``check_shape_flags``, ``size_rules_of``) and the polygon flags
                      (``POLYGON_FLAGS``, ``check_polygon_flags``, ``polygon_rules_of``, ``save_label_file``), both served
                      by ``describe_regions``; ``open_prediction`` (images, state dict, classes, banner, model),
                      ``prediction_outputs`` (``masks/``, ``overlays/``, ``labels/``, palettes), ``save_mask`` /
                      ``save_overlay``, ``save_frame_prediction`` (one image's entry, mask, overlay and label file) and
                      ``write_predictions`` (``predictions.json`` and the printed lines)

``torch`` and the kernels are imported inside the functions: parsing flags and ``--help`` need neither them nor a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

DATASETS = ("gear", "kolektorsdd")
HEAD_WEIGHT = "outc.conv.weight"                         # [num_classes, 64, 1, 1] of UNet and SegmentationUNet
_NOT_HERE = ("--save_predictions", "--save_confusion_matrix", "--debug", "--debug_samples")
TILING_FLAGS = [("--tiled", dict(action="store_true", help="Gear: predict every image at its own size, in tiles")),
                ("--tile", dict(type=int, nargs=2, default=None, metavar=("H", "W"), help="default: the frame flags")),
                ("--min_overlap", dict(type=int, default=64, help="pixels neighbouring tiles share at least"))]


# ----------------------------------------------------------------------------------------- flags of the eval_* tools
def cli_of(dataset):
    """the ``eval_gear`` / ``eval_kolektorsdd`` module: its FLAGS, _split_loader, _class_names and _batches"""
    from . import eval_gear, eval_kolektorsdd
    return {"gear": eval_gear, "kolektorsdd": eval_kolektorsdd}[dataset]


def base_flags(dataset):
    """the flags of ``eval_gear`` / ``eval_kolektorsdd`` for data, model, split, batch, workers, device, precision and
    save_dir"""
    return [(n, kw) for n, kw in cli_of(dataset).FLAGS if n not in _NOT_HERE]


def parse_dataset_args(argv, description, flags_of, epilog=None):
    """(parser, args): ``--dataset`` is parsed first, since the other flags, ``flags_of(dataset)``, depend on it.  A
    ``flags_of`` that has no flags for a data set raises ValueError, and the parser exits with its words.  The caller runs
    its own checks on ``args`` with ``parser.error``."""
    argv = list(sys.argv[1:] if argv is None else argv)
    first = argparse.ArgumentParser(add_help=False)
    first.add_argument("--dataset", required=True, choices=DATASETS)
    dataset = first.parse_known_args(argv)[0].dataset
    ap = argparse.ArgumentParser(description=description, epilog=epilog)
    ap.add_argument("--dataset", required=True, choices=DATASETS)
    try:
        flags = flags_of(dataset)
    except ValueError as e:
        ap.error(str(e))
    for name, kw in flags:
        ap.add_argument(name, **kw)
    return ap, ap.parse_args(argv)


def frame_of(args):
    if args.dataset == "gear":
        return [args.image_size, args.image_size]
    return [args.image_height, args.image_width]


def mode_of(args):
    return "tiled" if args.tiled else "frame"


def check_tiling(ap, args):
    """The rules of ``TILING_FLAGS``; ``args.tile`` defaults to the frame flags here."""
    if args.tiled and args.dataset != "gear":
        ap.error("--tiled needs --dataset gear: KolektorSDD's masks are bitmaps, there is no full-resolution loader")
    if args.tile is None:
        args.tile = frame_of(args)
    if min(args.tile) < 1:
        ap.error("--tile sides must be positive")
    if args.min_overlap < 0 or (args.tiled and args.min_overlap >= min(args.tile)):
        ap.error("--min_overlap must be at least 0 and, with --tiled, smaller than both tile sides")


def check_region_flags(ap, args):
    if args.min_region_pixels < 1:
        ap.error("--min_region_pixels must be at least 1")
    if any(not 0.0 <= t <= 1.0 for t in args.coverage_thresholds):
        ap.error("--coverage_thresholds must lie in 0..1")


# ----------------------------------------------------------------------------------------- an eval_* tool's session
def open_checkpoint_session(args, title, mode=None):
    """What an ``eval_*`` tool does between its flags and its pass: the device, the banner ``<DATASET> DATASET <title>
    [(mode)]``, ``--save_dir``, the loader of ``--split``, the class names, the model with the checkpoint loaded.
    Returns (device, cli, loader, num_classes, class_names, model)."""
    from .train_gear import build_seg_model, require_gpu
    from .utils import load_checkpoint

    device = require_gpu(args)
    cli = cli_of(args.dataset)
    said = f" ({mode})" if mode else ""
    print("=" * 60 + f"\n{args.dataset.upper()} DATASET {title}{said}\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nDataset: {args.split} split")
    os.makedirs(args.save_dir, exist_ok=True)
    loader, num_classes = cli._split_loader(args)
    class_names = cli._class_names(loader.dataset, num_classes)
    print(f"Number of classes: {num_classes}\nClass names: {class_names}\nSamples: {len(loader.dataset)}")
    model = build_seg_model(args, num_classes, device)
    epoch, loss = load_checkpoint(model, None, args.checkpoint, device)
    print(f"Loaded checkpoint from epoch {epoch} with loss {loss:.4f}")
    return device, cli, loader, num_classes, class_names, model


def tiled_predictor(args, loader, model):
    """The ``tiling.TiledPredictor`` of ``--tile``, ``--min_overlap`` and ``--batch_size``, once every image of the
    loader's data set is known to fit the full-resolution mask kernel."""
    from .tiling import TiledPredictor
    from .train_gear_crops import check_image_sizes
    check_image_sizes([loader.dataset])
    print(f"Tile: {args.tile}  min overlap: {args.min_overlap}")
    return TiledPredictor(model, args.tile, args.min_overlap, args.batch_size)


# ----------------------------------------------------------------------------------------- passes over a split
def full_resolution_images(loader, device):
    """Every image of a raw Gear loader at its own size, in data-set order: (the decoded uint8 DEVICE image (H0, W0, 3),
    its uint8 class mask (H0, W0) from ``crops.full_resolution_masks``, its path)."""
    from .crops import full_resolution_masks
    for images, polys, sizes, paths in loader:
        masks = full_resolution_masks(polys, sizes, device=device)
        for i in range(len(sizes)):
            yield images[i].to(device, non_blocking=True), masks[i], paths[i]


def normalized_frame(image_u8):
    """the normalised float32 frame (3, H0, W0) of a uint8 DEVICE image (H0, W0, 3), at its own size"""
    from .augment import color_jitter_normalize_u8
    return color_jitter_normalize_u8(image_u8[None])[0]


def frame_predictions(model, batches):
    """Per (images, masks, paths) device batch (labels uint8 (N, H, W), conf float32 (N, H, W), masks, paths): the
    model in eval mode under ``no_grad``, ``sheets.seg_confidence`` of its logits."""
    import torch
    from .sheets import seg_confidence
    model.eval()
    with torch.no_grad():
        for images, masks, paths in batches:
            labels, conf = seg_confidence(model(images))
            yield labels, conf, masks, paths


def tiled_predictions(predictor, loader, device):
    """``frame_predictions``' tuples with N = 1 from every image of a raw Gear loader at its own size, the way
    ``predict_tiled`` predicts; the truth is the full-resolution mask."""
    import torch
    with torch.no_grad():
        for image, mask, path in full_resolution_images(loader, device):
            labels, conf, _plan = predictor(normalized_frame(image))
            yield labels[None], conf[None], mask[None], [path]


def labelled_predictions(args, cli, loader, model, device):
    """``tiled_predictions`` with ``--tiled``, else ``frame_predictions`` over the data set's device batches"""
    if args.tiled:
        return tiled_predictions(tiled_predictor(args, loader, model), loader, device)
    return frame_predictions(model, cli._batches(args, loader, device))


# ----------------------------------------------------------------------------------------- flags of the predict* tools
def check_predict_flags(ap, args):
    if args.min_region_pixels < 1:
        ap.error("--min_region_pixels must be at least 1")
    if not 0.0 <= args.min_confidence <= 1.0:
        ap.error("--min_confidence must lie in 0..1")
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")


# build-only: length, width, orientation, perimeter and holes of every defect (csrc/shapes.hip, defects.shape_measures).
# Their default is "absent": a run that gives none of them has the ``args`` of before and launches nothing new.
DIRECTIONS = 32                                          # Feret directions over half a turn: the length is low by < 0.12 %
SHAPE_FLAGS = [("--measure_shapes", dict(action="store_true", default=argparse.SUPPRESS,
                                         help="add a shape block (Feret length / width, axes, perimeter, holes) per defect")),
               ("--pixel_size", dict(type=float, default=argparse.SUPPRESS, metavar="MM",
                                     help="millimetres per pixel of the original image: adds *_mm fields")),
               ("--min_defect_length", dict(type=float, default=argparse.SUPPRESS, metavar="X",
                                            help="count only defects at least this long (mm with --pixel_size, else "
                                                 "image pixels); implies --measure_shapes")),
               ("--min_defect_area", dict(type=float, default=argparse.SUPPRESS, metavar="X",
                                          help="count only defects of at least this area (mm2 with --pixel_size, else "
                                               "image pixels); implies --measure_shapes"))]


def check_shape_flags(ap, args):
    """The rules of ``SHAPE_FLAGS``.  With none of them given ``args`` stays as it is; otherwise all four are set
    (``measure_shapes`` True, ``pixel_size`` None or > 0, the thresholds 0 or what was given)."""
    given = {name[2:] for name, _ in SHAPE_FLAGS if hasattr(args, name[2:])}
    if not given:
        return
    if given == {"pixel_size"}:
        ap.error("--pixel_size needs --measure_shapes, --min_defect_length or --min_defect_area")
    args.measure_shapes = True
    args.pixel_size = getattr(args, "pixel_size", None)
    if args.pixel_size is not None and not 0.0 < args.pixel_size < float("inf"):
        ap.error("--pixel_size must be positive")
    for name in ("min_defect_length", "min_defect_area"):
        setattr(args, name, getattr(args, name, 0.0))
        if not 0.0 <= getattr(args, name) < float("inf"):
            ap.error(f"--{name} must be at least 0")


def size_rules_of(args):
    """``defects.size_rules`` of the shape flags, or None when shapes are not measured"""
    if not getattr(args, "measure_shapes", False):
        return None
    from . import defects
    return defects.size_rules(args.pixel_size, args.min_defect_length, args.min_defect_area)


# build-only: every defect's outline as a polygon in the Gear label format (csrc/contours.hip, polygons.py).  Absent by
# default, like the shape flags: a run that gives neither has the ``args`` of before and launches nothing new.
_POLYGON_LIMITS = ("the format has no holes (a hole is filled when the file is loaded) and the loader resolves overlaps by "
                   "class priority, spalling > pitting > scrape, not by nesting (a lower class inside a higher one's hole "
                   "is overwritten)")
POLYGON_FLAGS = [("--save_polygons", dict(action="store_true", default=argparse.SUPPRESS,
                                          help="write labels/<name>.txt, the counted defects' outlines as Gear label "
                                               "polygons, and add outline / hole_outlines to every defect; "
                                               + _POLYGON_LIMITS)),
                 ("--polygon_tolerance", dict(type=float, default=argparse.SUPPRESS, metavar="T",
                                              help="thin every outline (Douglas-Peucker) by at most T frame pixels, "
                                                   "default 0: every corner; implies --save_polygons"))]
# build-only: nearby fragments of one class count as one defect (csrc/groups.hip).  Absent by default, like the flags
# above: a run without it has the ``args`` of before and launches nothing new.
GROUP_FLAGS = [("--merge_gap", dict(type=int, default=argparse.SUPPRESS, metavar="PX",
                                    help="regions of one class whose pixels come within PX frame pixels (2..32, "
                                         "Euclidean) of each other are one defect: its size, box, confidence, shape "
                                         "and the size rules are those of the whole group; regions below "
                                         "--min_region_pixels are dropped first and bridge nothing"))]
BUILD_FLAGS = SHAPE_FLAGS + POLYGON_FLAGS + GROUP_FLAGS


def check_polygon_flags(ap, args):
    """The rules of ``POLYGON_FLAGS``.  With neither given ``args`` stays as it is; otherwise both are set."""
    if not any(hasattr(args, name[2:]) for name, _ in POLYGON_FLAGS):
        return
    args.save_polygons = True
    args.polygon_tolerance = getattr(args, "polygon_tolerance", 0.0)
    if not 0.0 <= args.polygon_tolerance < float("inf"):
        ap.error("--polygon_tolerance must be at least 0")


def check_group_flags(ap, args):
    """The rule of ``GROUP_FLAGS``.  Without the flag ``args`` stays as it is."""
    if hasattr(args, "merge_gap") and not 2 <= args.merge_gap <= 32:
        ap.error("--merge_gap must lie in 2..32 (frame pixels)")


def grouping_rules_of(args):
    """the ``grouping_rules`` block of ``predictions.json``, or None when regions are not grouped"""
    gap = getattr(args, "merge_gap", 0)
    if not gap:
        return None
    return {"merge_gap": gap,
            "units": "frame pixels: the frame the model ran at, which predict squeezes anisotropically from the image "
                     "(predict_tiled and predict_views scale both axes alike)",
            "rule": "regions of one class in one image with pixels p, q at (py - qy)^2 + (px - qx)^2 <= merge_gap^2 are "
                    "one defect, transitively; its fragments are listed per defect",
            "dropped": f"regions below --min_region_pixels ({args.min_region_pixels}) are dropped before grouping: they "
                       "link nothing and join nothing"}


def polygon_rules_of(args):
    """the ``polygon_rules`` block of ``predictions.json``, or None when no polygons are written"""
    if not getattr(args, "save_polygons", False):
        return None
    return {"tolerance": args.polygon_tolerance, "labels": "labels/<name>.txt: one line per counted defect, class - 1 then "
            "(x + 0.5) / W (y + 0.5) / H of its outline's pixel centres", "limits": _POLYGON_LIMITS}


def describe_regions(args, labels, num_classes, conf):
    """(records, shape records or None, outlines or None, fragment table or None) of label maps (N, H, W) for a predict
    tool: ``describe_class_regions``; with the shape flags ``measure_class_regions`` and with the polygon flags
    ``trace_class_regions`` (as ``polygons.outlines``) on the same labelling: the maps are labelled once.  With
    ``--merge_gap`` the records are those of the groups, and the outlines are keyed by group."""
    from . import evaluation, polygons
    shaped, traced = size_rules_of(args) is not None, polygon_rules_of(args) is not None
    got = evaluation.class_region_records(labels, num_classes, conf, args.min_region_pixels,
                                          directions=DIRECTIONS if shaped else None, contours=traced,
                                          merge_gap=getattr(args, "merge_gap", 0))
    outlines = polygons.outlines(got.loops, got.points, got.fragments) if traced else None
    return got.records, got.shapes, outlines, got.fragments


def save_label_file(args, name, entry, frame_hw):
    """``labels/<name>.txt`` of one image entry whose defects carry their outlines: its counted defects"""
    from . import polygons
    with open(os.path.join(args.output_dir, "labels", name + ".txt"), "w") as f:
        f.write("".join(line + "\n" for line in polygons.entry_label_lines(entry, frame_hw)))


def check_tile_scale(ap, args, default_tile):
    """The ``--tile``, ``--min_overlap`` and ``--scale`` rules of ``predict_tiled`` and ``predict_views``."""
    if args.tile is None:
        args.tile = list(default_tile)
    if min(args.tile) < 1:
        ap.error("--tile must be positive")
    if not 0 <= args.min_overlap < min(args.tile):
        ap.error("--min_overlap must be at least 0 and smaller than both tile sides")
    if not 0.0 < args.scale <= 4.0:
        ap.error("--scale must lie in (0, 4]")


# ----------------------------------------------------------------------------------------- a predict* tool's session
def open_prediction(args, task, title, kernel):
    """What a ``predict*`` tool does between its flags and its pass: the device, the images below ``--input`` and their
    output names, the checkpoint's state dict, ``--num_classes`` (default: the rows of the head weight; 2 to 8, the range
    of the ``kernel`` named in the refusal), the class names, ``--reject_classes`` against them, the banner ``<TASK>
    <title>``, the model with the state loaded.  Returns (device, paths, names, num_classes, class_names, model)."""
    from .train_gear import build_seg_model, require_gpu
    device = require_gpu(args)
    import torch
    from . import defects

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
        raise SystemExit(f"{num_classes} classes: the {kernel} kernel takes 2 to 8")
    class_names = defects.class_names_for(task["class_names"], num_classes, args.class_names)
    unknown = sorted(set(args.reject_classes or ()) - set(class_names))
    if unknown:
        raise SystemExit(f"--reject_classes {unknown}: the classes are {class_names}")
    print("=" * 60 + f"\n{args.task.upper()} {title}\n" + "=" * 60)
    print(f"Device: {device}\nCheckpoint: {os.path.basename(args.checkpoint)}\nImages: {len(paths)}")
    print(f"Number of classes: {num_classes}\nClass names: {class_names}")
    model = build_seg_model(args, num_classes, device)
    model.load_state_dict(state)
    return device, paths, names, num_classes, class_names, model


def prediction_outputs(args, task, num_classes, device):
    """``{output_dir}/masks`` and, with ``--save_overlays``, ``{output_dir}/overlays`` and, with the polygon flags,
    ``{output_dir}/labels``, made; the task's class palette on the device and as the bytes of a Pillow palette.  Returns
    (mask_dir, overlay_dir, palette, palette_bytes)."""
    from . import sheets
    mask_dir = os.path.join(args.output_dir, "masks")
    os.makedirs(mask_dir, exist_ok=True)
    if polygon_rules_of(args) is not None:
        os.makedirs(os.path.join(args.output_dir, "labels"), exist_ok=True)
    overlay_dir = os.path.join(args.output_dir, "overlays")
    if args.save_overlays:
        os.makedirs(overlay_dir, exist_ok=True)
    host_palette = sheets.class_palette(num_classes, task["palette"])
    return mask_dir, overlay_dir, host_palette.to(device), host_palette.numpy().tobytes()


def save_mask(labels_u8, palette_bytes, path):
    from PIL import Image
    im = Image.fromarray(labels_u8)                    # mode L; the palette makes it P
    im.putpalette(palette_bytes)
    im.save(path)


def save_overlay(frame, labels, palette, path):
    """image | image with the prediction overlaid, of normalised frames (N, 3, H, W) and their labels (N, H, W)"""
    from . import sheets
    from .seg_visualize import GUTTER, OVERLAY_ALPHA, save_png
    sheet = sheets.render_seg_sheet(frame, [("image",), ("overlay", labels, OVERLAY_ALPHA)], gutter=GUTTER, palette=palette)
    save_png(sheet, path)


def save_frame_prediction(args, outputs, path, name, original, labels, conf, records, class_names, plans, frame=None,
                          defect_extras=None, shapes=None, traced=None, fragments=None):
    """One image of ``predict_tiled`` / ``predict_views``: its ``predictions.json`` entry from the ``records`` of its
    label map (H, W) and confidence, ``masks/<name>.png`` at the image's ``original`` size (NEAREST when the frame
    differs), and with ``--save_overlays`` the overlay on ``frame``, the normalised (3, H, W) frame.  ``plans``: the keys
    that follow ``frame_size`` in the entry; ``defect_extras``: {key: one value per listed defect, in the records' order}.
    ``outputs``: what ``prediction_outputs`` returned; ``shapes``: the records' shape records from ``describe_regions``
    (None unless the shape flags are given); ``traced``: its outlines (None unless the polygon flags are given), which
    go into the defects and, for the counted ones, into ``labels/<name>.txt``; ``fragments``: its fragment table (None
    unless ``--merge_gap`` is given).  Returns the entry."""
    from . import augment, defects
    mask_dir, overlay_dir, palette, palette_bytes = outputs
    frame_hw = (int(labels.shape[0]), int(labels.shape[1]))
    (entry,) = defects.defect_entries(records, class_names, frame_hw, [original], args.min_confidence, args.reject_classes,
                                      shapes, size_rules_of(args), **({} if fragments is None else {"fragments": fragments}))
    pixels = {cls: 0 for cls in class_names[1:]}
    for k, d in enumerate(entry["defects"]):                # defect_entries keeps the records' order: by root
        for key, values in (defect_extras or {}).items():
            d[key] = values[k]
        pixels[d["class_name"]] += d["pixels"]
    if traced is not None:
        from . import polygons
        polygons.attach_outlines([entry], records, traced, frame_hw, [original], args.polygon_tolerance)
        save_label_file(args, name, entry, frame_hw)
    mask = labels if frame_hw == original else augment.resize_nearest_u8(labels[None, :, :, None], *original)[0, :, :, 0]
    save_mask(mask.cpu().numpy(), palette_bytes, os.path.join(mask_dir, name + ".png"))
    if args.save_overlays:
        save_overlay(frame[None], labels[None], palette, os.path.join(overlay_dir, name + ".png"))
    return {"image_path": path, "name": name, "original_size": list(original), "frame_size": list(frame_hw), **plans,
            "mean_confidence": float(conf.double().mean()), "defect_pixels": pixels, **entry}


def write_predictions(args, class_names, images, middle=None, frame_size=None):
    """``{output_dir}/predictions.json`` (args, class_names, [frame_size,] [size_rules,] [polygon_rules,] [grouping_rules,]
    images, summary)
    and the printed
    lines: one per image -- decision, name, then the frame size and ``middle(entry)`` (such as "in 4 tiles") when
    ``middle`` is given, then its first four defects, with their Feret length when shapes were measured -- and the
    totals.  ``size_rules`` (``size_rules_of``) is there only with the shape flags, ``polygon_rules`` (``polygon_rules_of``)
    only with the polygon flags.  Returns the file's path."""
    from . import defects
    summary = defects.summarize(images, class_names)
    shared = {} if frame_size is None else {"frame_size": list(frame_size)}
    rules = size_rules_of(args)
    if rules is not None:
        shared["size_rules"] = rules
    if polygon_rules_of(args) is not None:
        shared["polygon_rules"] = polygon_rules_of(args)
    if grouping_rules_of(args) is not None:
        shared["grouping_rules"] = grouping_rules_of(args)
    unit = "mm" if rules and rules["pixel_size"] is not None else "px"
    length = "feret_length_mm" if unit == "mm" else "feret_length"
    out_path = os.path.join(args.output_dir, "predictions.json")
    with open(out_path, "w") as f:
        json.dump({"args": vars(args), "class_names": class_names, **shared, "images": images, "summary": summary}, f,
                  indent=2)
    for im in images:
        found = ", ".join(f"{d['class_name']} {d['pixels']} px @ {d['mean_confidence']:.2f}"
                          + (f" in {len(d['fragments'])} fragments" if len(d.get("fragments", ())) > 1 else "")
                          + (f" length {d['shape'][length]:.1f} {unit}" if "shape" in d else "")
                          + (f" (views {d['mean_view_agreement']:.2f})" if "mean_view_agreement" in d else "")
                          for d in im["defects"][:4])
        more = f" (+{len(im['defects']) - 4} more)" if len(im["defects"]) > 4 else ""
        where = "" if middle is None else f" {im['frame_size'][0]}x{im['frame_size'][1]} {middle(im)}"
        print(f"{im['decision']:>6}  {im['name']}{where}: {found or 'no defects'}{more}")
    print(f"Images: {summary['images']}  rejected: {summary['rejected']}  defects: {summary['defects']}")
    print(f"Predictions saved to: {out_path}")
    return out_path
