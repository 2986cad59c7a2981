"""GPU checks of crop training: unet_affine_crop_u8 byte for byte against tests/_crops_ref.py over a ragged batch, both
modes, both channel counts and every store path; its guards; crops.GearCropPreprocess against the reference with
replayed parameters; and the train_gear_crops -> predict_tiled round trip."""
import ctypes
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import _crops_ref as R
from tiaozhanbei_unet_amd import _lib, augment, crops, predict_tiled, train_gear_crops
from tiaozhanbei_unet_amd.gear_dataset import GearDataset, collate_raw, write_synthetic_gear

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(5, 7), (12, 9), (1, 1), (33, 40)]             # the ragged batch
ONE = 65536


def _images(c, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in SIZES]


def _shift(dy, dx):
    """centre to centre: output (y, x) <- source (y + dy, x + dx)"""
    return [ONE, 0, dx * ONE + ONE // 2, 0, ONE, dy * ONE + ONE // 2]


def _descs(oh, ow):
    """every kind of crop the issue lists, over images 0, 1 and 3 (image 2 has no crop here)"""
    m = lambda *a: R.crop_matrix(*a, oh, ow)            # noqa: E731
    d = [(3, _shift(2, 3)),                                             # an identity slice
         (3, m(3 + ow / 2, 2 + oh / 2, 1.0, 0.0, True)),                # the same slice, flipped
         (3, m(20.0, 16.0, 1.0, 10.0, False)), (3, m(20.0, 16.0, 1.0, 90.0, False)), (3, m(20.3, 16.7, 1.0, -37.0, True)),
         (3, m(20.0, 16.0, 0.5, 0.0, False)), (3, m(19.6, 16.2, 2.0, 5.0, False)), (3, m(20.0, 16.0, 4.0, -8.0, True)),
         (1, _shift(-2, 0)), (1, _shift(12 - oh + 3, 0)), (1, _shift(0, -3)), (1, _shift(0, 9 - ow + 2)),   # off each edge
         (1, m(4.5, 6.0, 1.3, 200.0, False)),
         (0, _shift(0, 0)), (0, m(3.5, 2.5, 0.75, 15.0, False)),       # (for 16 x 12 and 8 x 8) an image smaller than the crop
         (3, m(33.1, 8.4, 1.0, 45.0, False)), (1, _shift(0, 0)), (3, _shift(33 - oh, 40 - ow))]
    return d


def _pack(images):
    sizes = [im.shape[:2] for im in images]
    nbytes = [im.size for im in images]
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    return np.concatenate([im.reshape(-1) for im in images]), offsets, sizes


def _launch(src, src_bytes, offsets, sizes, n_images, c, descs, oh, ow, mode, fill, misalign=0):
    """the library itself, on tables of the test's making"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    table = np.zeros(len(descs), dtype=crops.CROP_DTYPE)
    for k, (image, a) in enumerate(descs):
        table[k]["image"], table[k]["a"] = image, a
    s_d, o_d = dev(src), dev(np.asarray(offsets, dtype=np.int64))
    h_d, t_d = dev(np.asarray(sizes, dtype=np.int32).reshape(-1, 2)), dev(table.view(np.uint8))
    n = len(descs) * oh * ow * c
    buf = torch.full((n + 8,), 77, dtype=torch.uint8, device=DEV)
    out = buf[misalign:misalign + n]
    rc = _lib.lib().unet_affine_crop_u8(s_d.data_ptr(), src_bytes, o_d.data_ptr(), h_d.data_ptr(), n_images, c,
                                        t_d.data_ptr(), len(descs), oh, ow, mode, fill, out.data_ptr(), None)
    assert rc == 0, _lib.lib().unet_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:misalign] == 77).all()) and bool((buf[misalign + n:] == 77).all())       # nothing written around it
    return out.cpu().numpy().reshape(len(descs), oh, ow, c)


# (4, 5): rows of 15 / 5 bytes, the byte path; (16, 12) and (8, 8): rows of 36 / 12 and 24 / 8 bytes, the dword path
@pytest.mark.parametrize("oh,ow", [(4, 5), (16, 12), (8, 8)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 1])
def test_kernel_equals_the_restatement(c, mode, oh, ow):
    images = _images(c)
    descs = _descs(oh, ow)
    assert {i for i, _ in descs} == {0, 1, 3} and sum(i == 3 for i, _ in descs) >= 3
    for fill in (0, 255):
        want = R.crops(images, descs, oh, ow, mode, fill)
        got = crops.affine_crops_u8([torch.from_numpy(im) for im in images], descs, (oh, ow), mode, fill, device=DEV)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(descs), oh, ow, c) and got.is_cuda
        bad = np.argwhere(got.cpu().numpy() != want)
        assert len(bad) == 0, (fill, bad[:5])
        # device images take the other packing to the same bytes
        again = crops.affine_crops_u8([torch.from_numpy(im).to(DEV) for im in images], descs, (oh, ow), mode, fill)
        assert torch.equal(again, got)
    # the crops off an edge of image 1 hold pixels of both kinds, inside and fill
    for k in (8, 9, 10, 11):
        inside = R.inside_mask(SIZES[1], descs[k][1], oh, ow)
        assert 0 < inside.sum() < inside.size, k


@pytest.mark.parametrize("c", [3, 1])
def test_centre_to_centre_is_the_torch_slice(c):
    images = [torch.from_numpy(im).to(DEV) for im in _images(c, seed=4)]
    for oh, ow in ((4, 5), (16, 12), (8, 8)):
        for mode in ("nearest", "bilinear"):
            descs = [(3, _shift(2, 3)), (3, _shift(33 - oh, 40 - ow)), (3, R.crop_matrix(3 + ow / 2, 2 + oh / 2, 1, 0, True, oh, ow))]
            got = crops.affine_crops_u8(images, descs, (oh, ow), mode, 9)
            assert torch.equal(got[0], images[3][2:2 + oh, 3:3 + ow])
            assert torch.equal(got[1], images[3][33 - oh:, 40 - ow:])
            assert torch.equal(got[2], images[3][2:2 + oh, 3:3 + ow].flip(1))
    # the 1 x 1 image and the smallest one, the others without a crop; a stacked batch
    got = crops.affine_crops_u8(images, [(2, _shift(0, 0)), (0, _shift(-1, -1))], (4, 5), 1, 200)
    want = R.crops([im.cpu().numpy() for im in images], [(2, _shift(0, 0)), (0, _shift(-1, -1))], 4, 5, 1, 200)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(got[0, 0, 0, 0]) == int(images[2][0, 0, 0]) and bool((got[0, 1:] == 200).all())
    stack = torch.stack([images[3], images[3].flip(0)])
    got = crops.affine_crops_u8(stack, [(1, _shift(2, 3))], (8, 8), 0, 0)
    assert torch.equal(got[0], stack[1][2:10, 3:11])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [3, 1])
def test_guards_write_fill_and_stay_inside(c, mode):
    """tables the wrapper would refuse, given to the library itself: a defined result, all fill"""
    images = _images(c, seed=2)
    src, offsets, sizes = _pack(images)
    total, oh, ow = len(src), 16, 12
    descs = _descs(oh, ow)[:8] + [(-1, _shift(0, 0)), (4, _shift(0, 0)), (1 << 20, _shift(0, 0)), (1, _shift(0, 0)), (0, _shift(0, 0))]
    for fill in (0, 255):
        # as packed: only the image indices outside 0..3 are fill
        got = _launch(src, total, offsets, sizes, 4, c, descs, oh, ow, mode, fill)
        assert np.array_equal(got, R.crops(sizes, descs, oh, ow, mode, fill, c=c, offsets=offsets, src=src))
        assert np.all(got[8:11] == fill) and not np.all(got[0] == fill)
        # src_bytes one short: the last image runs past it -> its crops are all fill, the others as before
        short = _launch(src, total - 1, offsets, sizes, 4, c, descs, oh, ow, mode, fill)
        assert np.all(short[:8] == fill) and np.array_equal(short[8:], got[8:])
        # n_images = 3: image 3 is outside the table
        assert np.all(_launch(src, total, offsets, sizes, 3, c, descs, oh, ow, mode, fill)[:8] == fill)
        # a negative offset, an offset past the end, an empty side, a side that would overflow h w c
        for bad_off, bad_hw in ((-1, sizes[1]), (total, sizes[1]), (offsets[1], (0, 9)), (offsets[1], (12, -9)),
                                (offsets[1], (2 ** 31 - 1, 2 ** 31 - 1))):
            o2, s2 = list(offsets), list(sizes)
            o2[1], s2[1] = bad_off, bad_hw
            bad = _launch(src, total, o2, s2, 4, c, descs, oh, ow, mode, fill)
            assert np.all(bad[11] == fill) and np.array_equal(np.delete(bad, 11, 0), np.delete(got, 11, 0)), (bad_off, bad_hw)


def test_unaligned_output_wide_rows_and_many_rows():
    """the byte path on a dword-able shape (dst off by one byte); rows of more than one block segment on both paths
    (87 x 3 = 261 bytes; 344 x 3 = 1032 bytes = 258 dwords); more rows than the grid has blocks"""
    images = _images(3, seed=6)
    src, offsets, sizes = _pack(images)
    descs = _descs(16, 12)
    want = R.crops(images, descs, 16, 12, 1, 0)
    for mis in (1, 2, 3):
        assert np.array_equal(_launch(src, len(src), offsets, sizes, 4, 3, descs, 16, 12, 1, 0, misalign=mis), want), mis
    for oh, ow in ((3, 87), (2, 344)):
        d = [(3, R.crop_matrix(20.0, 16.0, 0.1, 12.0, False, oh, ow)), (1, R.crop_matrix(4.0, 6.0, 0.03, -20.0, True, oh, ow)),
             (3, _shift(1, -150))]
        for mode in (0, 1):
            got = crops.affine_crops_u8([torch.from_numpy(im) for im in images], d, (oh, ow), mode, 255, device=DEV)
            assert np.array_equal(got.cpu().numpy(), R.crops(images, d, oh, ow, mode, 255)), (oh, ow, mode)
    many = (descs * 62)[:1100]                          # 17600 rows of 16 x 12: past 16384 blocks they stride over the crops
    got = crops.affine_crops_u8([torch.from_numpy(im) for im in images], many, (16, 12), 1, 0, device=DEV).cpu().numpy()
    assert np.array_equal(got, np.concatenate([want] * 62)[:1100])


# ------------------------------------------------------------------------------------------------ Gear batches
@pytest.fixture(scope="module")
def gear_batch(tmp_path_factory):
    root = write_synthetic_gear(str(tmp_path_factory.mktemp("gear_crops")), seed=5)
    ds = GearDataset(root, "train", raw=True)
    images, polys, sizes, _paths = collate_raw([ds[i] for i in range(5)])
    assert len(set(sizes)) == 3 and len(polys["classes"]) > 0
    # the yardstick: every image's mask at its own size, one polygon launch per distinct size over the WHOLE batch
    by_size = {hw: augment.polygon_masks_u8(polys, sizes, hw[0], hw[1], device=DEV) for hw in set(sizes)}
    masks = [by_size[hw][i] for i, hw in enumerate(sizes)]
    return images, polys, sizes, masks


def test_nearest_crop_of_the_full_resolution_mask_is_its_slice(gear_batch):
    images, polys, sizes, masks = gear_batch
    full = crops.full_resolution_masks(polys, sizes, device=DEV)
    assert all(torch.equal(a, b) and tuple(a.shape) == hw for a, b, hw in zip(full, masks, sizes))
    assert sum(int(m.max()) > 0 for m in masks) >= 3
    oh, ow = 40, 48
    descs = [(i, _shift(h - oh - 3, w - ow - 5)) for i, (h, w) in enumerate(sizes)]
    got = crops.affine_crops_u8([m.unsqueeze(-1) for m in full], descs, (oh, ow), 0, 255)
    for i, (h, w) in enumerate(sizes):
        assert torch.equal(got[i, :, :, 0], masks[i][h - oh - 3:h - 3, w - ow - 5:w - 5]), i


@pytest.mark.parametrize("train", [True, False])
def test_gear_crop_preprocess_replays_to_the_reference(gear_batch, train):
    images, polys, sizes, masks = gear_batch
    crop_hw = (24, 32)
    pre = crops.GearCropPreprocess(crop_hw, train=train, crops_per_image=3, scale_range=(0.5, 3.0), degrees=25.0, seed=9)
    params = pre.draw(sizes, polys)
    k = 3 * len(sizes)
    assert len(params["image"]) == k and (("orders" in params) == train)
    if not train:
        assert set(params["scale"]) == {1.0} and set(params["angle"]) == {0.0} and not any(params["flip"])
    x, m = pre(images, polys, sizes, device=DEV, params=params)
    assert x.dtype == torch.float32 and tuple(x.shape) == (k, 3, 24, 32) and m.dtype == torch.long and tuple(m.shape) == (k, 24, 32)
    descs = [(i, R.crop_matrix(cx, cy, s, a, f, *crop_hw)) for i, cx, cy, s, a, f in
             zip(params["image"], params["cx"], params["cy"], params["scale"], params["angle"], params["flip"])]
    want_m = R.crops([t.cpu().numpy()[..., None] for t in masks], descs, 24, 32, 0, 255)[..., 0]
    assert np.array_equal(m.cpu().numpy(), want_m.astype(np.int64))
    want_bytes = torch.from_numpy(R.crops([t.numpy() for t in images], descs, 24, 32, 1, 0)).to(DEV)
    jitter = augment.jitter_table(params["orders"], params["brightness"], params["contrast"], params["saturation"],
                                  params["hue"]) if train else None
    assert torch.equal(x, augment.color_jitter_normalize_u8(want_bytes, jitter))
    # the mask is 255 exactly where the image crop is fill
    for j, (i, a) in enumerate(descs):
        assert np.array_equal(want_m[j] == 255, ~R.inside_mask(sizes[i], a, 24, 32)), j
    # drawing inside the call gives a batch of the same form, and a second object with the same seed the same batch
    x2, m2 = crops.GearCropPreprocess(crop_hw, train=train, crops_per_image=3, scale_range=(0.5, 3.0), degrees=25.0, seed=9)(
        images, polys, sizes, device=DEV)
    assert torch.equal(x2, x) and torch.equal(m2, m)


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_gear_crops_round_trip(tmp_path, precision):
    exp = train_gear_crops.main(["--synthetic", "--epochs", "2", "--val_freq", "1", "--crop_size", "64", "64",
                                 "--crops_per_image", "2", "--batch_size", "4", "--min_overlap", "16", "--num_workers", "0",
                                 "--precision", precision, "--save_dir", str(tmp_path / "runs")])
    assert os.path.basename(exp).startswith("gear_crops_seg_unet_") and os.path.dirname(exp) == str(tmp_path / "runs")
    for sub in ("checkpoints", "results", "visualizations", "logs"):
        assert os.path.isdir(os.path.join(exp, sub)), sub
    args = json.load(open(os.path.join(exp, "args.json")))
    assert args["crop_size"] == [64, 64] and args["crops_per_image"] == 2 and args["precision"] == precision
    assert "image_size" not in args and "sync_mask" not in args
    res = json.load(open(os.path.join(exp, "results", "training_results.json")))
    assert set(res) == {"train_losses", "val_losses", "best_val_miou", "total_epochs", "total_params", "num_classes", "args"}
    assert len(res["train_losses"]) == 2 and len(res["val_losses"]) == 2 and res["num_classes"] == 4
    assert all(math.isfinite(v) and v > 0 for v in res["train_losses"] + res["val_losses"])
    assert 0.0 <= res["best_val_miou"] <= 1.0
    ckpt = os.path.join(exp, "checkpoints", "checkpoint_epoch_1.pth")
    assert os.path.exists(ckpt) and os.path.exists(os.path.join(exp, "checkpoints", "checkpoint_epoch_0.pth"))
    state = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert {"model_state_dict", "optimizer_state_dict", "epoch"} <= set(state) and state["epoch"] == 1

    source = os.path.join(args["data_root"], "images", "test")
    out = tmp_path / "pred"
    predict_tiled.main(["--task", "gear", "--checkpoint", ckpt, "--input", source, "--tile", "64", "64", "--min_overlap", "16",
                        "--batch_size", "4", "--num_workers", "0", "--precision", precision, "--output_dir", str(out)])
    got = json.load(open(out / "predictions.json"))
    files = sorted(glob.glob(os.path.join(source, "*.png")))
    assert [e["image_path"] for e in got["images"]] == files and len(files) == 5
    assert got["class_names"] == ["background", "pitting", "spalling", "scrape"]
    assert all(e["tiling"]["tile"] == [min(64, e["frame_size"][0]), min(64, e["frame_size"][1])] for e in got["images"])
    assert all(os.path.exists(out / "masks" / (e["name"] + ".png")) for e in got["images"])
