#!/usr/bin/env python3
"""Evaluate a Gear segmentation checkpoint on the test or val split (reference test.py), on the HIP
path: workers decode and parse, ``gear_dataset.GearPreprocess`` makes images and masks on the GPU, the statistics come
from ``metrics.per_image_stats`` (seg_eval.py).

    python -m tiaozhanbei_unet_amd.eval_gear --checkpoint best_model.pth --data_root datasets/Gear [--split val]

Same flags as the reference (test.py:20-64) plus --precision.  Class names are ``['background'] +
dataset.class_names``.  Writes ``{save_dir}/evaluation_results.json``: the reference's script defines that file
(test.py:192-223) but stops with a NameError (an undefined ``logger``, test.py:262) before writing it; this CLI
writes it.  Build-only: ``per_image_results.json``.
"""
from . import seg_eval

FLAGS = seg_eval.eval_flags([("--image_size", dict(type=int, default=512))], "datasets/Gear")


def parse_args(argv=None):
    return seg_eval.parse_args(FLAGS, "Test UNet on Gear dataset (MI355X HIP path)", argv)


def _split_loader(args):
    from .gear_dataset import get_gear_dataloaders
    _train, val, test, num_classes = get_gear_dataloaders(args.data_root, args.batch_size,
                                                          (args.image_size, args.image_size), args.num_workers)
    return (test if args.split == "test" else val), num_classes


def _class_names(dataset, num_classes):
    if hasattr(dataset, "class_names"):
        return ["background"] + list(dataset.class_names)
    return ["background", "pitting", "spalling", "scrape"][:num_classes]       # reference test.py:289 (Subset)


def _batches(args, loader, device):
    """(images, masks, paths) device batches of a raw loader"""
    from .gear_dataset import GearPreprocess
    pre = GearPreprocess((args.image_size, args.image_size), train=False)
    for images, polys, sizes, paths in loader:
        x, m = pre(images, polys, sizes, device=device)
        yield x, m, paths


def main(argv=None):
    args = parse_args(argv)
    return seg_eval.run(args, "GEAR", _split_loader, lambda loader, device: _batches(args, loader, device),
                        _class_names)


if __name__ == "__main__":
    main()
