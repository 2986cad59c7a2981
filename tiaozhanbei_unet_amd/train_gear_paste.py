#!/usr/bin/env python3
"""``train_gear_crops`` with copy-paste augmentation (no reference counterpart; Ghiasi et al., CVPR 2021): labelled defects
of any image of a batch are pasted, with their own scale, rotation and flip, into the crops of the others, and their
labels with them.

    python -m tiaozhanbei_unet_amd.train_gear_paste --data_root datasets/Gear --epochs 50 [--copy_paste 0.5] [--synthetic]

Gear's defects are rare and unevenly spread over the three classes; ``--defect_fraction`` only re-centres crops on the
defects an image has.  Here a crop takes pastes with probability ``--copy_paste``: 1..``--max_pastes`` of them, each a
polygon of a uniformly drawn CLASS of the batch (so a rare class is pasted as often as a common one), at the crop's own
scale times a log-uniform factor in ``--paste_scale_range``, rotated within +-``--paste_degrees``, flipped or not, at a
uniform place of the crop (``crops.PasteSampler``, host arithmetic from a generator of its own: the crops are the ones
``train_gear_crops`` draws).  The images, the full-resolution class masks, the polygon boxes and the crop matrices are on
the device every batch anyway; ``crops.paste_crops_u8`` (csrc/paste.hip) writes the image crops and the mask crops
together in ONE launch, the pastes applied on the way out, in place of ``train_gear_crops``' two crop launches.  The
ColorJitter runs on the composite.

Everything else -- validation, checkpoints, ``training_results.json`` -- is ``train_gear_crops``', under
``{save_dir}/gear_paste_{model}_{ts}``.  Once per epoch the pastes drawn per class are printed (host counts).
"""
import argparse

from . import train_gear_crops
from .train_gear_crops import FLAGS as CROP_FLAGS

FLAGS = CROP_FLAGS + [
    ("--copy_paste", dict(type=float, default=0.5, metavar="P", help="share of crops that take pastes (0..1)")),
    ("--max_pastes", dict(type=int, default=2, metavar="N", help="a crop that takes pastes takes 1..N (1..8)")),
    ("--paste_scale_range", dict(type=float, nargs=2, default=[0.75, 1.33], metavar=("LO", "HI"),
                                 help="a paste's scale relative to its crop's, log-uniform (0 < LO <= HI <= 4)")),
    ("--paste_degrees", dict(type=float, default=180.0, metavar="D", help="a paste's rotation within +-D (0..180)")),
]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Train UNet for Gear segmentation on native-resolution crops with copy-paste "
                                             "defect augmentation (MI355X HIP path)")
    for name, kw in FLAGS:
        ap.add_argument(name, **kw)
    args = ap.parse_args(argv)
    train_gear_crops.check_args(ap, args)
    if not 0.0 <= args.copy_paste <= 1.0:
        ap.error("--copy_paste must lie in 0..1")
    if not 1 <= args.max_pastes <= 8:
        ap.error("--max_pastes must lie in 1..8")
    if not 0.0 < args.paste_scale_range[0] <= args.paste_scale_range[1] <= 4.0:
        ap.error("--paste_scale_range needs 0 < LO <= HI <= 4")
    if not 0.0 <= args.paste_degrees <= 180.0:
        ap.error("--paste_degrees must lie in 0..180")
    return args


def paste_preprocess(args, crop):
    """``train_gear_crops``' training preprocess with a ``PasteSampler`` of this trainer's flags"""
    from .crops import GearCropPreprocess, PasteSampler
    print(f"Copy-paste: {args.copy_paste:.2f} of the crops, up to {args.max_pastes} pastes, relative scale "
          f"{args.paste_scale_range}, +-{args.paste_degrees} degrees")
    paste = PasteSampler(crop, args.copy_paste, args.max_pastes, tuple(args.paste_scale_range), args.paste_degrees,
                         seed=args.seed)
    return GearCropPreprocess(crop, train=True, crops_per_image=args.crops_per_image, scale_range=tuple(args.scale_range),
                              degrees=args.degrees, defect_fraction=args.defect_fraction, seed=args.seed, paste=paste)


def main(argv=None):
    return train_gear_crops.run(parse_args(argv), "gear_paste", paste_preprocess)


if __name__ == "__main__":
    main()
