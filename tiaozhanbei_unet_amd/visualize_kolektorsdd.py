#!/usr/bin/env python3
"""Draw a KolektorSDD segmentation checkpoint's predictions (reference visualize_kolektorsdd.py), on the HIP path:
workers only decode, ``kolektorsdd_dataset.GpuPreprocess`` makes images and masks on the GPU, label maps and the
confidence map come from ``sheets.seg_confidence`` and every picture from one ``sheets.render_seg_sheet`` launch
(seg_visualize.py).

    python -m tiaozhanbei_unet_amd.visualize_kolektorsdd --checkpoint best_model.pth --save_individual --save_grid

Same flags and defaults as the reference (visualize_kolektorsdd.py:21-73) plus --precision and --synthetic.  --figsize
is accepted and unused: sheets are at the native resolution of the tensors.  --save_individual writes one picture per
sample: image | truth | prediction [| confidence through viridis over [0, 1] under --show_confidence]; --save_grid
writes the grid of image | truth | prediction.  Class i takes the tab10 entry imshow(vmin=0, vmax=C-1) gives it.  Class
names are ``dataset.class_names``, as in ``eval_kolektorsdd``.  Titles and colour bars are in ``visualizations.json``;
``class_distribution.json`` stands in for the bar chart and is always written.
"""
import os

from . import seg_visualize

FLAGS = seg_visualize.vis_flags([("--image_height", dict(type=int, default=1024)),
                                 ("--image_width", dict(type=int, default=512))], "datasets/KolektorSDD",
                                "visualizations")
PANELS = ("image", "truth", "prediction")                 # reference visualize_kolektorsdd.py:111-126, :168-183


def parse_args(argv=None):
    from .seg_eval import parse_args as parse
    return parse(FLAGS, "Visualize UNet predictions on KolektorSDD dataset (MI355X HIP path)", argv)


def _split_loader(args):
    from .kolektorsdd_dataset import get_kolektorsdd_dataloaders
    train, val, test, num_classes = get_kolektorsdd_dataloaders(
        args.data_root, args.batch_size, (args.image_height, args.image_width), args.num_workers, raw=True)
    return {"test": test, "val": val, "train": train}[args.split], num_classes


def main(argv=None):
    from .eval_kolektorsdd import _class_names
    from .kolektorsdd_dataset import GpuPreprocess, write_synthetic_kolektorsdd

    args = seg_visualize.prepare(parse_args(argv), write_synthetic_kolektorsdd, "kolektorsdd_syn_")
    os.makedirs(args.save_dir, exist_ok=True)

    def batches(loader, device):
        pre = GpuPreprocess((args.image_height, args.image_width), train=False)
        for images, masks, paths in loader:
            x, m = pre(images, masks, device=device)
            yield x, m, paths

    style = {"palette": "scaled", "individual": PANELS + (("confidence",) if args.show_confidence else ()),
             "grid": PANELS, "save_individual": args.save_individual, "save_grid": args.save_grid}
    return seg_visualize.run(args, "KOLEKTORSDD", _split_loader, batches, _class_names, style)


if __name__ == "__main__":
    main()
