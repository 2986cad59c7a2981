"""GPU checks of what the checkpoint tools share (seg_cli.py): the full-resolution image walk and the tiled
labelled-prediction source against the calls they are made of, image by image, and train_gear_crops.validate_tiled, which
is built on the walk, against the predictor's blended logits.  One synthetic Gear tree (images of three sizes) and one
model of random weights serve all of them."""
import numpy as np
import pytest
import torch

from tiaozhanbei_unet_amd import SegmentationUNet, crops, eval_detection, seg_cli, sheets, train_gear_crops
from tiaozhanbei_unet_amd.augment import color_jitter_normalize_u8
from tiaozhanbei_unet_amd.gear_dataset import collate_raw, get_gear_dataloaders, write_synthetic_gear
from tiaozhanbei_unet_amd.metrics import CombinedSegmentationLoss

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """(the test split's raw loader in batches of 3, the parsed flags of a tiled tool, a model of random weights)"""
    root = write_synthetic_gear(str(tmp_path_factory.mktemp("gear")))
    _train, _val, loader, num_classes = get_gear_dataloaders(root, 3, (64, 64), 0)
    args = eval_detection.parse_args(["--dataset", "gear", "--checkpoint", "none.pth", "--data_root", root, "--tiled",
                                      "--tile", "64", "64", "--min_overlap", "8", "--batch_size", "3"])
    torch.manual_seed(5)
    return loader, args, SegmentationUNet(3, num_classes, precision="fp32").to(DEV)


def test_the_image_walk_and_the_tiled_source(split, capsys):
    loader, args, model = split
    ds = loader.dataset
    walked = list(seg_cli.full_resolution_images(loader, DEV))
    assert len(walked) == len(ds) == 4 and [path for _i, _m, path in walked] == list(ds.image_paths)
    assert len({tuple(image.shape) for image, _m, _p in walked}) > 1           # the images differ in size
    frames = []
    for i, (image, mask, _path) in enumerate(walked):
        own, polys, sizes, _paths = collate_raw([ds[i]])                       # the image alone, not within its batch
        assert image.dtype == torch.uint8 and image.is_cuda and torch.equal(image.cpu(), own[0])
        (want,) = crops.full_resolution_masks(polys, sizes, device=DEV)
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == sizes[0] and torch.equal(mask, want)
        frames.append(seg_cli.normalized_frame(image))
        assert torch.equal(frames[i], color_jitter_normalize_u8(own[0].to(DEV)[None])[0])
    assert any(int(mask.max()) > 0 for _i, mask, _p in walked)                 # there are defects in the truth

    predictor = seg_cli.tiled_predictor(args, loader, model)
    assert "Tile: [64, 64]  min overlap: 8" in capsys.readouterr().out
    assert (predictor.tile_hw, predictor.min_overlap, predictor.batch_size) == ((64, 64), 8, 3)
    got = list(seg_cli.tiled_predictions(predictor, loader, DEV))
    assert len(got) == len(ds)
    tiles = 0
    for (labels, conf, masks, paths), frame, (_image, mask, path) in zip(got, frames, walked):
        want_labels, want_conf, plan = predictor(frame)
        tiles = max(tiles, len(plan["origins_y"]) * len(plan["origins_x"]))
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (1,) + tuple(frame.shape[1:])
        assert torch.equal(labels, want_labels[None]) and torch.equal(conf, want_conf[None])
        assert torch.equal(masks, mask[None]) and paths == [path]
    assert tiles > 1                                                           # some image needs more than one tile


def test_validate_tiled_is_the_blended_logits_image_by_image(split):
    loader, args, model = split
    num_classes = 4
    predictor = seg_cli.tiled_predictor(args, loader, model)
    criterion = CombinedSegmentationLoss(ignore_index=crops.IGNORE_INDEX)
    got = train_gear_crops.validate_tiled(model, criterion, loader, predictor, num_classes, torch.device(DEV))

    ds = loader.dataset
    total, confusion = torch.zeros((), dtype=torch.float64, device=DEV), np.zeros((num_classes, num_classes), np.int64)
    for i in range(len(ds)):
        own, polys, sizes, _paths = collate_raw([ds[i]])
        (mask,) = crops.full_resolution_masks(polys, sizes, device=DEV)
        logits, _plan = predictor.blended_logits(color_jitter_normalize_u8(own[0].to(DEV)[None])[0])
        labels, _conf = sheets.seg_confidence(logits[None])
        with torch.no_grad():
            total += criterion(logits[None], mask[None].long()).double()
        np.add.at(confusion, (mask.cpu().numpy().ravel(), labels[0].cpu().numpy().ravel()), 1)
    assert got["loss"] == float(total) / len(ds) and got["loss"] > 0
    assert np.array_equal(got["metrics"]["confusion_matrix"], confusion) and confusion.sum() == sum(
        h * w for h, w in (ds[i][0].shape[:2] for i in range(len(ds))))
