#!/usr/bin/env python3
"""Draw a Gear segmentation checkpoint's predictions (reference visualize.py), on the HIP path: workers decode and
parse, ``gear_dataset.GearPreprocess`` makes images and masks on the GPU, label maps come from ``sheets.seg_confidence``
and every picture from one ``sheets.render_seg_sheet`` launch (seg_visualize.py).

    python -m tiaozhanbei_unet_amd.visualize_gear --checkpoint best_model.pth --data_root datasets/Gear [--split val]

Same flags and defaults as the reference (visualize.py:20-72) plus --precision and --synthetic; --save_dir defaults to
``<checkpoint dir>/visualizations`` and --always_save to true, so the per-sample pictures and the grid are always
written.  --figsize is accepted and unused: sheets are at the native resolution of the tensors.  Panels: the image with
the truth overlaid | the image with the prediction overlaid, alpha 0.4, class i in tab10 entry i, nothing drawn on the
background.  The overlay is this package's integer blend, not Agg's compositing of an RGBA layer; titles and the legend
are in ``visualizations.json``, and ``class_distribution.json`` stands in for the bar chart.  Logs go through
``utils.setup_logging`` into --save_dir, as in the reference.
"""
import os

from . import seg_visualize

FLAGS = seg_visualize.vis_flags([("--image_size", dict(type=int, default=512))], "datasets/Gear", None,
                                extra=[("--always_save", dict(action="store_true", default=True))])
PANELS = ("overlay_truth", "overlay_prediction")         # reference visualize.py:141-151, :202-214


def parse_args(argv=None):
    from .seg_eval import parse_args as parse
    return parse(FLAGS, "Visualize UNet predictions on Gear dataset (MI355X HIP path)", argv)


def _split_loader(args):
    from .gear_dataset import get_gear_dataloaders
    train, val, test, num_classes = get_gear_dataloaders(args.data_root, args.batch_size,
                                                         (args.image_size, args.image_size), args.num_workers)
    return {"test": test, "val": val, "train": train}[args.split], num_classes


def main(argv=None):
    from .eval_gear import _class_names
    from .gear_dataset import GearPreprocess, write_synthetic_gear
    from .utils import setup_logging

    args = seg_visualize.prepare(parse_args(argv), write_synthetic_gear, "gear_syn_")
    if args.save_dir is None:                              # reference visualize.py:274-283
        args.save_dir = os.path.join(os.path.dirname(args.checkpoint), "visualizations")
    os.makedirs(args.save_dir, exist_ok=True)
    logger = setup_logging(args.save_dir, "visualization")

    def batches(loader, device):
        pre = GearPreprocess((args.image_size, args.image_size), train=False)
        for images, polys, sizes, paths in loader:
            x, m = pre(images, polys, sizes, device=device)
            yield x, m, paths

    always = args.always_save
    style = {"palette": "index", "individual": PANELS, "grid": PANELS,
             "save_individual": args.save_individual or always, "save_grid": args.save_grid or always}
    try:
        return seg_visualize.run(args, "GEAR", _split_loader, batches, _class_names, style, log=logger.info)
    finally:
        for h in list(logger.handlers):
            logger.removeHandler(h)
            h.close()


if __name__ == "__main__":
    main()
