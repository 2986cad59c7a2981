#!/usr/bin/env python3
"""Evaluate a KolektorSDD segmentation checkpoint on the test or val split (reference test_kolektorsdd.py), on the
HIP path: workers only decode, ``kolektorsdd_dataset.GpuPreprocess``
makes images and masks on the GPU, the statistics come from ``metrics.per_image_stats`` (seg_eval.py).

    python -m tiaozhanbei_unet_amd.eval_kolektorsdd --checkpoint best_model.pth --data_root datasets/KolektorSDD

Same flags as the reference (test_kolektorsdd.py:20-72) plus --precision.  Class names are ``dataset.class_names``.
Writes ``{save_dir}/evaluation_results.json`` with the reference's schema; build-only: ``per_image_results.json``.
"""
from . import seg_eval

FLAGS = seg_eval.eval_flags([("--image_height", dict(type=int, default=1024)),
                             ("--image_width", dict(type=int, default=512))], "datasets/KolektorSDD",
                            extra=[("--train_split", dict(type=float, default=0.7)),
                                   ("--val_split", dict(type=float, default=0.15))])


def parse_args(argv=None):
    return seg_eval.parse_args(FLAGS, "Test UNet on KolektorSDD dataset (MI355X HIP path)", argv)


def _split_loader(args):
    from .kolektorsdd_dataset import get_kolektorsdd_dataloaders
    _train, val, test, num_classes = get_kolektorsdd_dataloaders(
        args.data_root, args.batch_size, (args.image_height, args.image_width), args.num_workers, args.train_split,
        args.val_split, raw=True)
    return (test if args.split == "test" else val), num_classes


def _class_names(dataset, num_classes):
    if hasattr(dataset, "class_names"):
        return list(dataset.class_names)
    return ["background", "defect_type_1", "defect_type_2"][:num_classes]      # reference test_kolektorsdd.py (Subset)


def _batches(args, loader, device):
    """(images, masks, paths) device batches of a raw loader"""
    from .kolektorsdd_dataset import GpuPreprocess
    pre = GpuPreprocess((args.image_height, args.image_width), train=False)
    for images, masks, paths in loader:
        x, m = pre(images, masks, device=device)
        yield x, m, paths


def main(argv=None):
    args = parse_args(argv)
    return seg_eval.run(args, "KOLEKTORSDD", _split_loader, lambda loader, device: _batches(args, loader, device),
                        _class_names)


if __name__ == "__main__":
    main()
