"""GPU tests of the Gear path: the polygon-mask kernel (csrc/polygon.hip through augment.polygon_masks_u8) bit-exact
against the reference's own masks (tests/golden/gear_masks.npz) except the known-divergent
``diverge_*`` cases, pinned as strict xfails; GearPreprocess against the PIL oracle; and the
train_gear CLI end to end on a synthetic tree."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import pil_oracle as PO
from test_cpu_gear import DIVERGENT, class_mask
from tiaozhanbei_unet_amd import augment as A
from tiaozhanbei_unet_amd import gear_dataset as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gear_masks.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _polys(gold, i):
    return [(int(c), [tuple(v) for v in gold[f"{i}_verts"][gold[f"{i}_offsets"][p]:gold[f"{i}_offsets"][p + 1]].tolist()])
            for p, c in enumerate(gold[f"{i}_classes"])]


def _groups(gold):
    """fixture case indices grouped by source size: one kernel batch per group"""
    out = {}
    for i in range(len(gold["names"])):
        out.setdefault(tuple(int(v) for v in gold[f"{i}_size"]), []).append(i)
    return out


def _kernel_masks(gold, divergent):
    """{(case index, key): kernel mask} for key in full / the fixture's resize keys, one kernel batch per source size"""
    keys = [str(k) for k in gold["resize_keys"]]
    outs = {"full": None, **{k: tuple(int(v) for v in s) for k, s in zip(keys, gold["resize_sizes"])}}
    res = {}
    for size, idx in _groups(gold).items():
        idx = [i for i in idx if str(gold["names"][i]).startswith(DIVERGENT) == divergent]
        if not idx:
            continue
        polys = G.flatten_polygons([_polys(gold, i) for i in idx])
        for key, out in outs.items():
            oh, ow = size if out is None else out
            got = A.polygon_masks_u8(polys, [size] * len(idx), oh, ow, device=DEV).cpu().numpy()
            for j, i in enumerate(idx):
                res[(i, key)] = got[j]
    return res


def test_kernel_bit_exact_against_every_fixture(gold):
    for (i, key), got in _kernel_masks(gold, divergent=False).items():
        want = gold[f"{i}_{key}"]
        assert np.array_equal(got, want), f"{gold['names'][i]} {key}: {int((got != want).sum())} pixels differ"


def test_kernel_follows_the_documented_rule_on_divergent_cases(gold):
    """Where the reconstructed rule differs from Pillow, the kernel still computes exactly that rule (test_cpu_gear)."""
    for (i, key), got in _kernel_masks(gold, divergent=True).items():
        if key == "full":
            h, w = (int(v) for v in gold[f"{i}_size"])
            want = class_mask(gold[f"{i}_verts"], gold[f"{i}_offsets"], gold[f"{i}_classes"], w, h)
            assert np.array_equal(got, want), gold["names"][i]


@pytest.mark.xfail(strict=True, reason="corner fix-up condition of Pillow's polygon fill not fully reconstructed")
def test_kernel_matches_pillow_on_known_divergent_cases(gold):
    for (i, key), got in _kernel_masks(gold, divergent=True).items():
        assert np.array_equal(got, gold[f"{i}_{key}"]), f"{gold['names'][i]} {key}"


def test_mixed_batch_and_determinism(gold):
    """One batch of differently sized images with 0, 1 and many polygons, incl. a full 1920 x 1080 -> 512 x 512 case."""
    names = [str(n) for n in gold["names"]]
    pick = [names.index(n) for n in ("empty", "square", "medium_blobs", "labelme_1920x1080_0", "malformed")]
    sizes = [tuple(int(v) for v in gold[f"{i}_size"]) for i in pick]
    polys = G.flatten_polygons([_polys(gold, i) for i in pick])
    a = A.polygon_masks_u8(polys, sizes, 512, 512, device=DEV)
    b = A.polygon_masks_u8(polys, sizes, 512, 512, device=DEV)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    got = a.cpu().numpy()
    for j, i in enumerate(pick):
        assert np.array_equal(got[j], gold[f"{i}_r512"]), names[i]
    assert not got[0].any() and not got[4].any()


def test_preprocess_eval_images_match_pil_oracle(tmp_path):
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ds = G.GearDataset(root, "val", (48, 64), raw=True)
    images, polys, sizes, _ = G.collate_raw([ds[i] for i in range(len(ds))])
    pre = G.GearPreprocess((48, 64), train=False)
    x, m = pre(images, polys, sizes, device=DEV)
    assert x.dtype == torch.float32 and m.dtype == torch.int64 and tuple(m.shape) == (len(ds), 48, 64)
    for j, img in enumerate(images):
        want = PO.to_tensor_normalize(PO.resize_bilinear(img.numpy(), 48, 64))
        assert np.array_equal(x[j].cpu().numpy(), want)
        ref = G.mask_from_polygons_pil(ds[j][1], sizes[j][1], sizes[j][0])
        assert np.array_equal(m[j].cpu().numpy(), PO.resize_nearest(ref[..., None], 48, 64)[..., 0])


def test_sync_mask_applies_the_image_flip_and_rotation(tmp_path):
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ds = G.GearDataset(root, "train", (40, 56), raw=True)
    images, polys, sizes, _ = G.collate_raw([ds[i] for i in range(len(ds))])
    plain = G.GearPreprocess((40, 56), train=True, seed=3)
    synced = G.GearPreprocess((40, 56), train=True, sync_mask=True, seed=3)
    params = plain.tf.draw(len(sizes))
    params["flips"][0], params["angles"][0] = True, 7.5               # make sure both transforms act
    x0, m0 = plain(images, polys, sizes, device=DEV, params=params)
    x1, m1 = synced(images, polys, sizes, device=DEV, params=params)
    assert torch.equal(x0, x1)
    want = A.flip_rotate_u8(m0.to(torch.uint8).unsqueeze(-1), params["flips"], params["angles"])[..., 0].long()
    assert torch.equal(m1, want)
    assert torch.equal(m0, A.polygon_masks_u8(polys, sizes, 40, 56, device=DEV).long())   # default: mask untouched


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_gear_cli_writes_reference_tree(tmp_path, precision):
    save = tmp_path / "out"
    cmd = [sys.executable, "-m", "tiaozhanbei_unet_amd.train_gear", "--synthetic", "--epochs", "2", "--val_freq", "1",
           "--save_freq", "1", "--batch_size", "4", "--image_size", "64", "--num_workers", "0", "--precision", precision,
           "--save_dir", str(save)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    (exp,) = glob.glob(str(save / "gear_seg_seg_unet_*"))
    for sub in ("checkpoints", "results", "visualizations", "logs"):
        assert os.path.isdir(os.path.join(exp, sub))
    args = json.load(open(os.path.join(exp, "args.json")))
    assert args["precision"] == precision and args["model"] == "seg_unet"
    for e in (0, 1):
        assert os.path.exists(os.path.join(exp, "checkpoints", f"checkpoint_epoch_{e}.pth"))
    res_json = json.load(open(os.path.join(exp, "results", "training_results.json")))
    assert set(res_json) == {"train_losses", "val_losses", "best_val_miou", "total_epochs", "total_params",
                             "num_classes", "args"}
    assert len(res_json["train_losses"]) == 2 and len(res_json["val_losses"]) == 2 and res_json["num_classes"] == 4
    assert all(np.isfinite(res_json["train_losses"])) and all(np.isfinite(res_json["val_losses"]))

    best = os.path.join(exp, "checkpoints", "best_model.pth")
    if res_json["best_val_miou"] > 0:
        assert os.path.exists(best)
    else:                                   # the reference saves only on an improvement over 0
        best = os.path.join(exp, "checkpoints", "checkpoint_epoch_1.pth")
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd.metrics import SegmentationMetrics
    from tiaozhanbei_unet_amd.utils import load_checkpoint
    model = SegmentationUNet(3, 4, precision=precision).to(DEV)
    load_checkpoint(model, None, best, DEV)
    model.eval()
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ds = G.GearDataset(root, "val", (64, 64), raw=True)
    images, polys, sizes, _ = G.collate_raw([ds[i] for i in range(len(ds))])
    x, m = G.GearPreprocess((64, 64), train=False)(images, polys, sizes, device=DEV)
    metrics = SegmentationMetrics(4)
    with torch.no_grad():
        metrics.update(model(x), m)
    assert np.isfinite(metrics.compute_all_metrics()["mean_iou"])
