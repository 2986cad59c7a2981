"""GPU tests of the predict tools' ``--merge_gap`` end to end (seg_cli.GROUP_FLAGS -> csrc/groups.hip -> defects.py,
polygons.py): the defects of ``predictions.json`` must be what the numpy reference (tests/_groups_ref.py) makes of the
saved ``masks/<name>.png``, and ``labels/<name>.txt`` redrawn with Pillow must give that mask with the holes filled.  The
model is randomly initialised, as in test_gpu_polygons_cli.py: its predictions are speckle, where nearly everything has
a neighbour within a few pixels."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

import _groups_ref as G
from tiaozhanbei_unet_amd import predict, predict_tiled, predict_views
from tiaozhanbei_unet_amd.gear_dataset import PRIORITY, RAW_TO_FINAL, mask_from_polygons_pil, parse_labelme_txt

pytestmark = pytest.mark.gpu
FOUR = ndimage.generate_binary_structure(2, 1)
GAP, MIN_PIXELS, FRAME = 4, 2, (64, 48)
NEW_DEFECT_KEYS = {"fragments", "fragment_outlines"}


@functools.lru_cache(maxsize=None)
def _tree(tmp):
    """(image directory, checkpoint) of a synthetic Gear tree and a randomly initialised model whose head biases are
    centred on the logits of noise, so that the argmax is speckle of all four classes"""
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd import gear_dataset
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    root = gear_dataset.write_synthetic_gear(os.path.join(tmp, "gear"))
    ckpt = os.path.join(tmp, "model.pth")
    torch.manual_seed(1)
    model = SegmentationUNet(3, 4, precision="fp32").to("cuda:0")
    model.eval()
    with torch.no_grad():
        noise = (torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(2)) - 0.45) / 0.226
        model.outc.conv.bias -= model(noise.to("cuda:0")).float().mean((0, 2, 3))
    save_checkpoint(model, get_optimizer(model), 0, 0.0, ckpt)
    return os.path.join(root, "images", "test"), ckpt


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _tree(str(tmp_path_factory.mktemp("groups")))


@pytest.fixture(scope="module")
def grouped(tree, tmp_path_factory):
    """predict --merge_gap with masks in the frame, shapes and polygons"""
    out = tmp_path_factory.mktemp("grouped")
    source, ckpt = tree
    predict.main(["--task", "gear", "--checkpoint", ckpt, "--input", source, "--image_size", str(FRAME[0]), str(FRAME[1]),
                  "--batch_size", "3", "--num_workers", "0", "--mask_size", "frame", "--output_dir", str(out),
                  "--min_region_pixels", str(MIN_PIXELS), "--merge_gap", str(GAP), "--save_polygons", "--measure_shapes"])
    return out, json.load(open(out / "predictions.json"))


def test_defects_are_the_references_groups_of_the_saved_masks(grouped):
    out, res = grouped
    h, w = FRAME
    rules = res["grouping_rules"]
    assert res["args"]["merge_gap"] == GAP and rules["merge_gap"] == GAP and "frame pixels" in rules["units"]
    assert str(MIN_PIXELS) in rules["dropped"]
    listed = joined = 0
    for e in res["images"]:
        mask = np.array(Image.open(out / "masks" / (e["name"] + ".png")))
        assert mask.shape == FRAME
        rec, frag = G.describe_groups(mask[None], 4, GAP, None, MIN_PIXELS)
        region = G.class_regions64(mask[None], 4)[0][0]
        assert len(e["defects"]) == len(rec)
        for d, r in zip(e["defects"], rec.tolist()):
            mine = frag[frag[:, 3] == r[2]]
            assert d["class"] == r[1] and d["pixels"] == r[3] and d["bbox"] == r[4:8]
            assert d["centroid"] == [r[8] / r[3], r[9] / r[3]]
            assert d["fragments"] == [{"root": [f[2] % w, f[2] // w], "pixels": f[4]} for f in mine.tolist()]
            assert d["shape"]["area"] == r[3] and len(d["fragment_outlines"]) == len(mine)
            for o, f in zip(d["fragment_outlines"], mine.tolist()):              # in root order, each on its own fragment
                assert all(region[y, x] == f[2] + 1 for x, y in o)
            assert d["outline"] in d["fragment_outlines"]
            joined += len(mine) > 1
        listed += len(rec)
    assert listed > 10 and joined > 3


def test_written_labels_redraw_the_mask_with_holes_filled(grouped):
    out, res = grouped
    h, w = FRAME
    for e in res["images"]:
        mask = np.array(Image.open(out / "masks" / (e["name"] + ".png")))
        region = G.class_regions64(mask[None], 4)[0][0]
        sizes = G.class_regions64(mask[None], 4)[1][0]
        want = np.zeros((h, w), np.uint8)
        for raw in reversed(PRIORITY):                   # the loader's order: the highest priority is drawn last
            cls = RAW_TO_FINAL[raw]
            for number in np.unique(region[(mask == cls) & (sizes >= MIN_PIXELS)]):
                want[ndimage.binary_fill_holes(region == number, structure=FOUR)] = cls
        parsed = parse_labelme_txt(str(out / "labels" / (e["name"] + ".txt")), w, h)
        assert all(d["counted"] for d in e["defects"])
        assert len(parsed) == sum(len(d["fragments"]) for d in e["defects"])      # one line per fragment
        assert np.array_equal(mask_from_polygons_pil(parsed, w, h), want), e["name"]


def test_without_the_flag_there_are_no_new_keys(tree, tmp_path):
    source, ckpt = tree
    argv = ["--task", "gear", "--checkpoint", ckpt, "--input", source, "--image_size", str(FRAME[0]), str(FRAME[1]),
            "--batch_size", "3", "--num_workers", "0", "--mask_size", "frame", "--min_region_pixels", str(MIN_PIXELS)]
    predict.main(argv + ["--output_dir", str(tmp_path / "plain")])
    plain = json.load(open(tmp_path / "plain" / "predictions.json"))
    assert "grouping_rules" not in plain and set(plain["args"]) == {name[2:] for name, _ in predict.FLAGS}
    assert not any(NEW_DEFECT_KEYS & set(d) for e in plain["images"] for d in e["defects"])
    # the flag alone, without shapes or polygons, adds the fragment lists and nothing else
    predict.main(argv + ["--output_dir", str(tmp_path / "gap"), "--merge_gap", str(GAP)])
    gap = json.load(open(tmp_path / "gap" / "predictions.json"))
    assert set(gap) - set(plain) == {"grouping_rules"} and set(gap["args"]) - set(plain["args"]) == {"merge_gap"}
    for e, p in zip(gap["images"], plain["images"]):
        assert sum(len(d["fragments"]) for d in e["defects"]) == len(p["defects"])
        assert all(set(d) - set(b) == {"fragments"} for d in e["defects"] for b in p["defects"][:1])
        assert e["defect_pixels"] == p["defect_pixels"]


def test_the_tiled_and_the_view_tools_group_alike(tree, tmp_path):
    source, ckpt = tree
    argv = ["--task", "gear", "--checkpoint", ckpt, "--input", source, "--tile", "32", "32", "--min_overlap", "8",
            "--batch_size", "8", "--num_workers", "0", "--min_region_pixels", str(MIN_PIXELS), "--merge_gap", str(GAP)]
    predict_tiled.main(argv + ["--output_dir", str(tmp_path / "tiled"), "--save_polygons"])
    # the second pass of predict_views, which averages the agreement, must group with the same gap or its rows differ
    predict_views.main(argv + ["--output_dir", str(tmp_path / "views"), "--view_scales", "1", "--view_flips", "h"])
    for name, keys in (("tiled", {"fragments", "fragment_outlines"}), ("views", {"fragments", "mean_view_agreement"})):
        res = json.load(open(tmp_path / name / "predictions.json"))
        assert res["grouping_rules"]["merge_gap"] == GAP
        joined = 0
        for e in res["images"]:
            mask = np.array(Image.open(tmp_path / name / "masks" / (e["name"] + ".png")))
            assert list(mask.shape) == e["frame_size"]
            rec, frag = G.describe_groups(mask[None], 4, GAP, None, MIN_PIXELS)
            assert [(d["class"], d["pixels"], d["bbox"]) for d in e["defects"]] == [(r[1], r[3], r[4:8]) for r in rec.tolist()]
            assert [len(d["fragments"]) for d in e["defects"]] == [int((frag[:, 3] == r[2]).sum()) for r in rec]
            assert all(keys <= set(d) for d in e["defects"])
            joined += sum(len(d["fragments"]) > 1 for d in e["defects"])
        assert joined > 0
