"""CPU checks of the per-defect records and the predict CLI: the numpy reference of the device kernel against a map
whose records are written out by hand, the host report (defects.py) on hand-made records and file trees, the CLI's
flags, and the exports and host-side refusals of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

import _defects_ref as D
from tiaozhanbei_unet_amd import _lib, defects, evaluation, ops, predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unet_describe_class_regions_workspace", "unet_describe_class_regions")


# ------------------------------------------------------------------------------------------------ exports
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert handle.unet_abi_version() == 1
    assert ops.describe_class_regions is evaluation.describe_class_regions
    assert ops.DEFECT_FIELDS is evaluation.DEFECT_FIELDS and ops.DEFECT_FIELDS == defects.FIELDS
    assert len(ops.DEFECT_FIELDS) == D.FIELDS == 12


BAD_SHAPES = [(65536, 1, 1, 3), (2, 64, 64, 1), (2, 64, 64, 256), (2, 32768, 32768, 3), (1, 1 << 16, 1 << 15, 3)]


def test_workspace_query_and_refusals_on_the_host():
    """decided before anything reaches the device: the workspace query returns 0 and the entry point the unsupported
    status for n = 65536, 1 and 256 classes and n h w = 2^31; min_pixels = 0 is a bad argument"""
    lib = _lib.lib()
    assert lib.unet_describe_class_regions_workspace(8, 512, 512, 4) == 8 * 512 * 512 * 4
    assert lib.unet_describe_class_regions_workspace(1, 1, 1, 2) == 16
    assert lib.unet_describe_class_regions_workspace(1, 1, (1 << 31) - 1, 255) > 0
    dummy = ctypes.c_void_p(16)                        # only checked for NULL: the shape is refused first
    for n, h, w, c in BAD_SHAPES:
        assert lib.unet_describe_class_regions_workspace(n, h, w, c) == 0, (n, h, w, c)
        rc = lib.unet_describe_class_regions(dummy, dummy, dummy, None, n, h, w, c, 1, 0, dummy, 16, dummy, dummy, 1 << 40,
                                             None)
        assert rc == -2, (n, h, w, c)
        assert b"2..255 classes" in lib.unet_last_error()
    call = lambda min_pixels, base, cap: lib.unet_describe_class_regions(              # noqa: E731
        dummy, dummy, dummy, None, 2, 8, 8, 3, min_pixels, base, dummy, cap, dummy, dummy, 1 << 40, None)
    assert call(0, 0, 16) == -1 and call(-5, 0, 16) == -1 and call(1, -1, 16) == -1 and call(1, 0, -1) == -1
    assert call(1, (1 << 31) - 2, 16) == -2            # image indices stay below 2^31
    assert call(1, 0, 1 << 31) == -2                   # a slot is an int32
    assert lib.unet_describe_class_regions(None, dummy, dummy, None, 2, 8, 8, 3, 1, 0, dummy, 16, dummy, dummy, 1 << 40,
                                           None) == -1
    assert lib.unet_describe_class_regions(dummy, dummy, dummy, None, 2, 8, 8, 3, 1, 0, dummy, 16, dummy, dummy, 15,
                                           None) == -3  # workspace too small


# ------------------------------------------------------------------------------------------------ the reference
HAND = np.array([[[1, 1, 0, 0, 2, 2, 0],
                  [1, 0, 0, 0, 0, 2, 0],
                  [0, 1, 0, 3, 0, 0, 0],               # (2, 1) touches (1, 0) by a corner: one region
                  [0, 0, 0, 3, 3, 0, 7],               # 7 is no class of 4: background
                  [2, 0, 0, 0, 3, 0, 0],
                  [2, 2, 0, 0, 0, 0, 1]]], np.uint8)
HAND_CONF = np.broadcast_to((np.arange(7, dtype=np.float32) + 1) / 8, (1, 6, 7))       # q = (x + 1) * 8192
#            image class root size x0 y0 x1 y1 sum_x sum_y conf_sum_q conf_max_q
HAND_REC = [[0, 1, 0, 4, 0, 0, 1, 2, 2, 3, 6 * 8192, 2 * 8192],
            [0, 2, 4, 3, 4, 0, 5, 1, 14, 1, 17 * 8192, 6 * 8192],
            [0, 3, 17, 4, 3, 2, 4, 4, 14, 12, 18 * 8192, 5 * 8192],
            [0, 2, 28, 3, 0, 4, 1, 5, 1, 14, 4 * 8192, 2 * 8192],
            [0, 1, 41, 1, 6, 5, 6, 5, 6, 5, 7 * 8192, 7 * 8192]]


def test_reference_against_records_written_out_by_hand():
    assert D.describe_records(HAND, 4, HAND_CONF).tolist() == HAND_REC
    no_conf = [r[:10] + [0, 0] for r in HAND_REC]
    assert D.describe_records(HAND, 4).tolist() == no_conf
    kept = D.describe_records(HAND, 4, HAND_CONF, min_pixels=4, image_base=9)
    assert kept.tolist() == [[9] + HAND_REC[0][1:], [9] + HAND_REC[2][1:]]
    assert D.describe_records(HAND, 4, min_pixels=5).shape == (0, 12)
    # with 3 classes the 3s are background too; with 8 the 7 is a region of its own
    assert D.describe_records(HAND, 3)[:, 1].tolist() == [1, 2, 2, 1]
    assert D.describe_records(HAND, 8)[:, 2].tolist() == [0, 4, 17, 27, 28, 41]
    two = D.describe_records(np.concatenate([HAND, HAND]), 4, np.concatenate([HAND_CONF, HAND_CONF]))
    assert two[:5].tolist() == HAND_REC and two[5:, 0].tolist() == [1] * 5 and two[5:, 1:].tolist() == [r[1:] for r in HAND_REC]


def test_reference_fixed_point_rounds_ties_to_even_and_clamps():
    v = np.array([0.0, 1.0, 0.5 / 65536, 1.5 / 65536, 2.5 / 65536, 65534.5 / 65536, 65535.5 / 65536, 1.2, -3.0, 0.25],
                 np.float32)
    assert D.q16(v).tolist() == [0, 65536, 0, 2, 2, 65534, 65536, 65536, 0, 16384]


# ------------------------------------------------------------------------------------------------ host report
NAMES = ["background", "pitting", "spalling", "scrape"]


def _rec(image, cls, size, box, sum_x, sum_y, conf_sum, conf_max, root=0):
    return [image, cls, root, size, *box, sum_x, sum_y, conf_sum, conf_max]


def test_defect_entries_scale_boxes_and_centroids_to_the_original_image():
    rec = [_rec(0, 2, 20, (10, 20, 19, 21), 290, 410, 20 * 49152, 65536), _rec(0, 1, 1, (0, 0, 0, 0), 0, 0, 16384, 16384, 1),
           _rec(0, 3, 1, (63, 63, 63, 63), 63, 63, 65536, 65536, 4095)]
    (entry,) = defects.defect_entries(rec, NAMES, (64, 64), [(96, 160)])
    d = entry["defects"][0]
    assert d["class"] == 2 and d["class_name"] == "spalling" and d["pixels"] == 20 and d["counted"] is True
    assert d["bbox"] == [10, 20, 19, 21]
    assert d["bbox_original"] == [25, 30, 49, 32]      # [10*160//64, 20*96//64, ceil(20*160/64) - 1, ceil(22*96/64) - 1]
    assert d["centroid"] == [14.5, 20.5] and d["centroid_original"] == [37.0, 31.0]
    assert d["mean_confidence"] == 0.75 and d["peak_confidence"] == 1.0
    corner, far = entry["defects"][1], entry["defects"][2]
    assert corner["bbox_original"] == [0, 0, 2, 1]     # pixel 0 covers [0, 2.5) x [0, 1.5) of the image
    assert corner["centroid_original"] == [0.75, 0.25] and corner["mean_confidence"] == 0.25
    assert far["bbox_original"] == [157, 94, 159, 95] and far["centroid_original"] == [158.25, 94.75]
    assert entry["decision"] == "reject"
    # a frame larger than the image: the box shrinks to the pixels it touches
    (small,) = defects.defect_entries([_rec(0, 1, 4, (2, 2, 3, 3), 10, 10, 0, 0)], NAMES, (64, 64), [(32, 32)])
    assert small["defects"][0]["bbox_original"] == [1, 1, 1, 1]
    assert small["defects"][0]["mean_confidence"] == 0.0 and small["defects"][0]["counted"] is True      # 0 >= 0


def test_decision_rules():
    rec = [_rec(0, 1, 10, (0, 0, 4, 1), 20, 5, 10 * 32768, 40000),       # pitting, mean 0.5
           _rec(1, 3, 2, (5, 5, 6, 5), 11, 10, 2 * 58982, 60000, 7),     # scrape, mean ~0.9
           _rec(3, 2, 5, (1, 1, 5, 1), 15, 5, 5 * 13107, 20000),         # spalling, mean ~0.2
           _rec(3, 1, 5, (1, 3, 5, 3), 15, 15, 5 * 39322, 40000, 9)]     # pitting, mean ~0.6
    sizes = [(64, 64)] * 4
    got = defects.defect_entries(rec, NAMES, (64, 64), sizes)
    assert [e["decision"] for e in got] == ["reject", "reject", "accept", "reject"]
    assert got[2] == {"defects": [], "decision": "accept"}                # no defects: accept
    assert [d["class_name"] for d in got[3]["defects"]] == ["spalling", "pitting"]   # by root index
    got = defects.defect_entries(rec, NAMES, (64, 64), sizes, min_confidence=0.55)
    assert [e["decision"] for e in got] == ["accept", "reject", "accept", "reject"]
    assert got[0]["defects"][0]["counted"] is False and len(got[0]["defects"]) == 1        # listed, not counted
    assert [d["counted"] for d in got[3]["defects"]] == [False, True]
    got = defects.defect_entries(rec, NAMES, (64, 64), sizes, min_confidence=0.5, reject_classes=["scrape"])
    assert [e["decision"] for e in got] == ["accept", "reject", "accept", "accept"]
    assert got[0]["defects"][0]["counted"] is True                         # mean == min_confidence counts
    got = defects.defect_entries(rec, NAMES, (64, 64), sizes, reject_classes=[])
    assert [e["decision"] for e in got] == ["accept"] * 4
    summary = defects.summarize(defects.defect_entries(rec, NAMES, (64, 64), sizes), NAMES)
    assert summary == {"images": 4, "rejected": 3, "defects": {"pitting": 2, "spalling": 1, "scrape": 1}}
    with pytest.raises(ValueError):
        defects.defect_entries(rec, NAMES, (64, 64), sizes[:2])
    assert defects.defect_entries(np.zeros((0, 12), np.int64), NAMES, (64, 64), sizes[:1]) == [
        {"defects": [], "decision": "accept"}]


def test_class_names_are_cut_or_extended():
    assert defects.class_names_for(NAMES, 3) == NAMES[:3]
    assert defects.class_names_for(NAMES, 6) == NAMES + ["class_4", "class_5"]
    assert defects.class_names_for(NAMES, 3, ["ok", "dent"]) == ["ok", "dent", "class_2"]


def test_list_images(tmp_path):
    for rel in ("b/x.PNG", "a/x.png", "a/x_label.bmp", "a/sub/y.bmp", "c.JPeG", "notes.txt", "a/X_LABEL.BMP", "a__x.jpg",
                "a/x.jpg", "a/z.tiff"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    root = str(tmp_path)
    got = defects.list_images(root)
    assert got == sorted(got)
    assert [os.path.relpath(p, root) for p in got] == ["a/sub/y.bmp", "a/x.jpg", "a/x.png", "a__x.jpg", "b/x.PNG", "c.JPeG"]
    names = defects.output_names(got, root)
    assert names[0] == "a__sub__y" and names[1] == "a__x" and names[4] == "b__x" and names[5] == "c"
    assert len(set(names)) == len(names)               # a/x.jpg, a/x.png and a__x.jpg stay apart
    assert defects.output_name(str(tmp_path / "b" / "x.PNG"), root) == "b__x"
    one = str(tmp_path / "a" / "x.png")
    assert defects.list_images(one) == [one] and defects.output_names([one], one) == ["x"]
    assert defects.list_images(str(tmp_path / "a" / "sub")) == [str(tmp_path / "a" / "sub" / "y.bmp")]
    for bad in ("notes.txt", "a/x_label.bmp", "missing"):
        with pytest.raises(ValueError):
            defects.list_images(str(tmp_path / bad))


# ------------------------------------------------------------------------------------------------ CLI flags
def test_predict_flags():
    gear = vars(predict.parse_args(["--task", "gear", "--checkpoint", "c.pth", "--input", "photos"]))
    assert gear["image_size"] == [512, 512]
    assert set(gear) == {"task", "checkpoint", "input", "output_dir", "image_size", "model", "bilinear", "dropout",
                         "precision", "batch_size", "num_workers", "device", "num_classes", "class_names",
                         "min_region_pixels", "min_confidence", "reject_classes", "mask_size", "save_overlays"}
    assert set(gear) == {name[2:] for name, _ in predict.FLAGS}
    assert (gear["output_dir"], gear["model"], gear["precision"], gear["batch_size"], gear["num_workers"],
            gear["device"], gear["dropout"], gear["bilinear"]) == ("predictions", "seg_unet", "fp32", 8, 4, "auto", 0.1, False)
    assert (gear["num_classes"], gear["class_names"], gear["reject_classes"]) == (None, None, None)
    assert (gear["min_region_pixels"], gear["min_confidence"], gear["mask_size"], gear["save_overlays"]) == (
        1, 0.0, "original", False)
    kol = vars(predict.parse_args(["--task", "kolektorsdd", "--checkpoint", "c.pth", "--input", "p.jpg"]))
    assert kol["image_size"] == [1024, 512]
    own = vars(predict.parse_args(["--task", "kolektorsdd", "--checkpoint", "c.pth", "--input", "p.jpg", "--image_size",
                                   "64", "32", "--mask_size", "frame", "--save_overlays", "--reject_classes", "a", "b",
                                   "--min_confidence", "0.5", "--min_region_pixels", "7"]))
    assert own["image_size"] == [64, 32] and own["mask_size"] == "frame" and own["save_overlays"]
    assert own["reject_classes"] == ["a", "b"] and own["min_confidence"] == 0.5 and own["min_region_pixels"] == 7
    base = {"--task": "gear", "--checkpoint": "c.pth", "--input": "photos"}
    for missing in base:                               # all three are required
        with pytest.raises(SystemExit):
            predict.parse_args([v for k, val in base.items() if k != missing for v in (k, val)])
    full = [v for kv in base.items() for v in kv]
    for extra in (["--task", "mvtec"], ["--min_region_pixels", "0"], ["--min_confidence", "1.5"],
                  ["--mask_size", "half"], ["--image_size", "64"], ["--data_root", "x"]):
        with pytest.raises(SystemExit):
            predict.parse_args(full + extra)


@pytest.mark.parametrize("task", ["gear", "kolektorsdd"])
def test_predict_refuses_cpu(task):
    with pytest.raises(SystemExit) as e:
        predict.main(["--task", task, "--device", "cpu", "--checkpoint", "ckpt.pth", "--input", "photos"])
    assert "no CPU path" in str(e.value)
