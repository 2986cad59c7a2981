"""GPU tests of the predict tools' polygon flags end to end (seg_cli.POLYGON_FLAGS -> csrc/contours.hip -> polygons.py): the
written ``labels/<name>.txt`` is read back with the loader's own parser and drawn with Pillow, the way the reference's
loader makes its masks, and must give the predicted map with the holes filled and the classes resolved by priority.  The
model is randomly initialised: its predictions are speckle with thin parts, saddles and holes, the hard case."""
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

from tiaozhanbei_unet_amd import predict, predict_tiled
from tiaozhanbei_unet_amd.gear_dataset import PRIORITY, RAW_TO_FINAL, mask_from_polygons_pil, parse_labelme_txt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EIGHT = np.ones((3, 3), int)
FOUR = ndimage.generate_binary_structure(2, 1)
OUTLINE_KEYS = {"outline", "outline_original", "hole_outlines"}


@functools.lru_cache(maxsize=None)
def _tree(tmp):
    """(image directory, checkpoint) of a synthetic Gear tree and a randomly initialised model"""
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd import gear_dataset as G
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    root = G.write_synthetic_gear(os.path.join(tmp, "gear"))
    ckpt = os.path.join(tmp, "model.pth")
    torch.manual_seed(1)
    model = SegmentationUNet(3, 4, precision="fp32").to(DEV)
    # a random head prefers one class everywhere (its biases differ by more than a pixel moves the logits): centre the
    # biases on the logits of noise like the tree's images, and the argmax becomes speckle of all four classes
    model.eval()
    with torch.no_grad():
        noise = (torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(2)) - 0.45) / 0.226
        model.outc.conv.bias -= model(noise.to(DEV)).float().mean((0, 2, 3))
    save_checkpoint(model, get_optimizer(model), 0, 0.0, ckpt)
    return os.path.join(root, "images", "test"), ckpt


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _tree(str(tmp_path_factory.mktemp("polygons")))


def _tiled(tree, out, *extra):
    source, ckpt = tree
    predict_tiled.main(["--task", "gear", "--checkpoint", ckpt, "--input", source, "--tile", "32", "32", "--min_overlap", "8",
                        "--batch_size", "8", "--num_workers", "0", "--scale", "1", "--output_dir", str(out), *extra])
    with open(os.path.join(out, "predictions.json"), "rb") as f:
        raw = f.read()
    return json.loads(raw), raw


@pytest.fixture(scope="module")
def traced(tree, tmp_path_factory):
    """predict_tiled --save_polygons with a size rule, so that some defects are listed and not counted"""
    out = tmp_path_factory.mktemp("traced")
    return out, _tiled(tree, out, "--save_polygons", "--min_defect_area", "3")[0]


def _regions_by_root(mask):
    """[(root, class, region mask)] of a label map, by root: the order of the listed defects"""
    out = []
    for cls in (1, 2, 3):
        lab, k = ndimage.label(mask == cls, structure=EIGHT)
        for i in range(1, k + 1):
            out.append((int(np.flatnonzero(lab.ravel() == i)[0]), cls, lab == i))
    return sorted(out, key=lambda r: r[0])


def test_written_labels_load_as_the_predicted_map_with_holes_filled(traced):
    out, res = traced
    assert res["polygon_rules"]["tolerance"] == 0.0 and res["args"]["save_polygons"] is True
    assert sorted(os.listdir(out / "labels")) == sorted(e["name"] + ".txt" for e in res["images"])
    listed = uncounted = holes = 0
    for e in res["images"]:
        mask = np.array(Image.open(out / "masks" / (e["name"] + ".png")))
        h, w = mask.shape
        assert [h, w] == e["original_size"] == e["frame_size"]
        regions = _regions_by_root(mask)
        assert len(regions) == len(e["defects"])
        want = np.zeros((h, w), np.uint8)
        for raw in reversed(PRIORITY):
            for (root, cls, member), d in zip(regions, e["defects"]):
                assert d["class"] == cls and d["pixels"] == int(member.sum()) and set(d) >= OUTLINE_KEYS
                if cls == RAW_TO_FINAL[raw] and d["counted"]:
                    want[ndimage.binary_fill_holes(member, structure=FOUR)] = cls
        parsed = parse_labelme_txt(str(out / "labels" / (e["name"] + ".txt")), w, h)
        assert len(parsed) == sum(d["counted"] for d in e["defects"])
        assert np.array_equal(mask_from_polygons_pil(parsed, w, h), want), e["name"]      # exact
        listed += len(e["defects"])
        uncounted += sum(not d["counted"] for d in e["defects"])
        holes += sum(len(d["hole_outlines"]) for d in e["defects"])
        for d in e["defects"]:
            assert d["outline_original"] == [[float(x), float(y)] for x, y in d["outline"]]      # scale 1
    assert listed > 20 and 0 < uncounted < listed                                 # the counted filter was at work
    assert holes > 0                                                              # and there were holes to fill


def test_predict_outlines_touch_all_four_sides_of_their_boxes(tree, tmp_path):
    source, ckpt = tree
    predict.main(["--task", "gear", "--checkpoint", ckpt, "--input", source, "--image_size", "64", "48", "--batch_size", "3",
                  "--num_workers", "0", "--mask_size", "frame", "--output_dir", str(tmp_path), "--save_polygons"])
    res = json.load(open(tmp_path / "predictions.json"))
    assert res["frame_size"] == [64, 48] and res["polygon_rules"]["tolerance"] == 0.0
    total = 0
    for e in res["images"]:
        mask = np.array(Image.open(tmp_path / "masks" / (e["name"] + ".png")))
        assert mask.shape == (64, 48)
        h0, w0 = e["original_size"]
        for (root, cls, member), d in zip(_regions_by_root(mask), e["defects"]):
            xs, ys = zip(*d["outline"])
            assert [min(xs), min(ys), max(xs), max(ys)] == d["bbox"]
            assert all(member[y, x] for x, y in d["outline"])                     # every point is a pixel of the region
            assert d["outline_original"][0] == [(xs[0] + 0.5) * w0 / 48 - 0.5, (ys[0] + 0.5) * h0 / 64 - 0.5]
            total += 1
        parsed = parse_labelme_txt(str(tmp_path / "labels" / (e["name"] + ".txt")), 48, 64)
        assert len(parsed) == len(e["defects"])                                   # every defect is counted here
    assert total > 0


def test_without_the_flags_nothing_changes(tree, tmp_path, traced):
    out = tmp_path / "plain"
    first, raw = _tiled(tree, out)
    assert not os.path.exists(out / "labels") and "polygon_rules" not in first
    assert set(first["args"]) == {name[2:] for name, _ in predict_tiled.FLAGS}
    assert not any(OUTLINE_KEYS & set(d) for e in first["images"] for d in e["defects"])
    shutil.rmtree(out)
    assert _tiled(tree, out)[1] == raw                                            # the same bytes again
    # and the traced run lists the same defects: what it adds are the new keys (and the size rule's shape and count)
    for e, p in zip(traced[1]["images"], first["images"]):
        assert len(e["defects"]) == len(p["defects"])
        for d, b in zip(e["defects"], p["defects"]):
            assert {k: v for k, v in d.items() if k not in OUTLINE_KEYS | {"shape", "counted"}} == \
                {k: v for k, v in b.items() if k != "counted"}


def test_a_tolerance_keeps_a_subsequence_of_every_outline(tree, tmp_path, traced):
    res, _ = _tiled(tree, tmp_path / "thin", "--polygon_tolerance", "1.5", "--min_defect_area", "3")
    assert res["polygon_rules"]["tolerance"] == 1.5 and res["args"]["save_polygons"] is True
    fewer = 0
    for e, full in zip(res["images"], traced[1]["images"]):
        assert len(e["defects"]) == len(full["defects"])
        for d, f in zip(e["defects"], full["defects"]):
            for thin, whole in zip([d["outline"]] + d["hole_outlines"], [f["outline"]] + f["hole_outlines"]):
                it = iter(whole)
                assert all(p in it for p in thin) and thin[0] == whole[0]         # a subsequence, in order
                fewer += len(whole) - len(thin)
            assert len(d["hole_outlines"]) == len(f["hole_outlines"])
    assert fewer > 0
