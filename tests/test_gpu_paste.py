"""GPU checks of copy-paste augmentation: unet_paste_crop_u8 byte for byte against tests/_paste_ref.py over the ragged
batch of tests/test_gpu_crops.py, both store paths, every kind of paste; against the two unet_affine_crop_u8 launches it
replaces; its guards; crops.GearCropPreprocess with a PasteSampler against the restatement with replayed parameters;
and the train_gear_paste -> predict_tiled round trip."""
import functools
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import _crops_ref as R
import _paste_ref as P
from tiaozhanbei_unet_amd import _lib, augment, crops, predict_tiled, train_gear_paste
from tiaozhanbei_unet_amd.gear_dataset import GearDataset, collate_raw, write_synthetic_gear

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 77


@functools.lru_cache(maxsize=None)
def _batch(seed=0):
    images, masks = P.fixture(seed)
    return images, masks, P.pack(images), P.pack(masks)


def _tables(pastes, n_crops, oh, ow):
    return P.tables(pastes, n_crops, lambda b, box: crops.paste_dst_box(b, box, oh, ow))


@functools.lru_cache(maxsize=None)
def _want(oh, ow, fill=0, ignore=255):
    """the restatement of the whole fixture, once per shape"""
    _images, _masks, (src, off, sizes), (msrc, moff, _) = _batch()
    descs, pastes = P.cases(oh, ow)
    tab, start = _tables(pastes, len(descs), oh, ow)
    return P.paste_crops(src, off, sizes, 4, msrc, moff, descs, start, tab, oh, ow, fill, ignore)


def _launch(src, src_bytes, offsets, sizes, n_images, msrc, mask_bytes, moff, descs, start, tab, oh, ow, fill, ignore,
            misalign=0):
    """the library itself, on tables of the test's making; sentinel bytes around both outputs"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    table = np.zeros(len(descs), dtype=crops.CROP_DTYPE)
    for k, (image, a) in enumerate(descs):
        table[k]["image"], table[k]["a"] = image, a
    rec = np.zeros(len(tab), dtype=crops.PASTE_DTYPE)
    for j, (donor, b, box, dst) in enumerate(tab):
        rec[j]["image"], rec[j]["b"], rec[j]["box"], rec[j]["dst"] = donor, b, box, dst
    s_d, o_d, m_d, mo_d = dev(src), dev(np.asarray(offsets, dtype=np.int64)), dev(msrc), dev(np.asarray(moff, dtype=np.int64))
    h_d, t_d = dev(np.asarray(sizes, dtype=np.int32).reshape(-1, 2)), dev(table.view(np.uint8))
    st_d = dev(np.asarray(start, dtype=np.int32))
    p_d = dev(rec.view(np.uint8)) if len(rec) else None
    n = len(descs) * oh * ow
    buf_i = torch.full((3 * n + 8,), SENTINEL, dtype=torch.uint8, device=DEV)
    buf_m = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device=DEV)
    out_i, out_m = buf_i[misalign:misalign + 3 * n], buf_m[misalign:misalign + n]
    rc = _lib.lib().unet_paste_crop_u8(s_d.data_ptr(), src_bytes, o_d.data_ptr(), h_d.data_ptr(), n_images, m_d.data_ptr(),
                                       mask_bytes, mo_d.data_ptr(), t_d.data_ptr(), len(descs), st_d.data_ptr(),
                                       p_d.data_ptr() if len(rec) else None, len(rec), oh, ow, fill, ignore,
                                       out_i.data_ptr(), out_m.data_ptr(), None)
    assert rc == 0, _lib.lib().unet_last_error()
    torch.cuda.synchronize()
    for buf, size in ((buf_i, 3 * n), (buf_m, n)):      # nothing written around them
        assert bool((buf[:misalign] == SENTINEL).all()) and bool((buf[misalign + size:] == SENTINEL).all())
    return out_i.cpu().numpy().reshape(len(descs), oh, ow, 3), out_m.cpu().numpy().reshape(len(descs), oh, ow)


def _same(got, want, what=""):
    for g, w, name in zip(got, want[:2], ("image", "mask")):
        bad = np.argwhere(np.asarray(g) != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:5])


# (4, 5): the byte path; (16, 12) and (8, 8): out_w % 4 == 0, the dword path
@pytest.mark.parametrize("oh,ow", [(4, 5), (16, 12), (8, 8)])
def test_kernel_equals_the_restatement(oh, ow):
    images, masks, (src, off, sizes), (msrc, moff, _) = _batch()
    descs, pastes = P.cases(oh, ow)
    tab, start = _tables(pastes, len(descs), oh, ow)
    assert start[-1] - start[-2] == 9                   # the raw table's last crop owns nine: only eight count
    want = _want(oh, ow)
    _same(_launch(src, len(src), off, sizes, 4, msrc, len(msrc), moff, descs, start, tab, oh, ow, 0, 255), want)
    other = P.paste_crops(src, off, sizes, 4, msrc, moff, descs, start, tab, oh, ow, 255, 9)
    _same(_launch(src, len(src), off, sizes, 4, msrc, len(msrc), moff, descs, start, tab, oh, ow, 255, 9), other, "fill 255, ignore 9")
    assert (other[1] != want[1]).any()
    # the wrapper: the pastes in any order, host tensors and device tensors
    few = [p for p in pastes if p[0] < 8]
    shuffled = sorted(few, key=lambda p: -p[0])         # crops descending, the order within a crop kept
    host = ([torch.from_numpy(im) for im in images], [torch.from_numpy(m) for m in masks])
    got = crops.paste_crops_u8(host[0], host[1], descs[:8], shuffled, (oh, ow), device=DEV)
    assert got[0].dtype == got[1].dtype == torch.uint8 and got[0].is_cuda and got[1].is_cuda
    assert tuple(got[0].shape) == (8, oh, ow, 3) and tuple(got[1].shape) == (8, oh, ow)
    _same((got[0].cpu().numpy(), got[1].cpu().numpy()), (want[0][:8], want[1][:8]), "wrapper")
    again = crops.paste_crops_u8([t.to(DEV) for t in host[0]], [t.to(DEV) for t in host[1]], descs[:8], few, (oh, ow))
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    mixed = crops.paste_crops_u8(host[0], [t.to(DEV) for t in host[1]], descs[:8], few, (oh, ow), device=DEV)
    assert torch.equal(mixed[0], got[0]) and torch.equal(mixed[1], got[1])
    # the mask is 255 exactly where the base crop left its image, pasted or not (image 3's own mask holds 255s)
    for k in (4, 5, 6):
        assert np.array_equal(want[1][k] == 255, ~R.inside_mask(P.SIZES[descs[k][0]], descs[k][1], oh, ow)), k


@pytest.mark.parametrize("oh,ow", [(4, 5), (16, 12), (8, 8)])
def test_zero_pastes_are_the_two_crop_launches(oh, ow):
    images, masks, _, _ = _batch()
    descs, _pastes = P.cases(oh, ow)
    im = [torch.from_numpy(a).to(DEV) for a in images]
    mk = [torch.from_numpy(a).to(DEV) for a in masks]
    for fill, ignore in ((0, 255), (9, 0)):
        x, m = crops.paste_crops_u8(im, mk, descs, [], (oh, ow), fill, ignore)
        assert torch.equal(x, crops.affine_crops_u8(im, descs, (oh, ow), "bilinear", fill))
        assert torch.equal(m, crops.affine_crops_u8([t.unsqueeze(-1) for t in mk], descs, (oh, ow), "nearest", ignore)[..., 0])


@pytest.mark.parametrize("oh,ow", [(4, 5), (16, 12), (8, 8)])
def test_centre_to_centre_is_a_torch_slice_and_where(oh, ow):
    images, masks, _, _ = _batch()
    descs, pastes = P.cases(oh, ow)
    im, mk = torch.from_numpy(images[3]).to(DEV), torch.from_numpy(masks[3]).to(DEV)
    x0, y0, x1, y1 = P.BLOBS[3][1][1]
    in_box = torch.zeros_like(mk, dtype=torch.bool)
    in_box[y0:y1, x0:x1] = True
    member = in_box & (mk != 0) & (mk != 255)
    dy, dx = 19 - oh // 2, 24 - ow // 2
    base_i, base_m = im[2:2 + oh, 3:3 + ow], mk[2:2 + oh, 3:3 + ow]
    don_i, don_m, mem = im[dy:dy + oh, dx:dx + ow], mk[dy:dy + oh, dx:dx + ow], member[dy:dy + oh, dx:dx + ow]
    assert bool(mem.any()) and not bool(mem.all())
    got_i, got_m = crops.paste_crops_u8([torch.from_numpy(a) for a in images], [torch.from_numpy(a) for a in masks], descs[:2],
                                        pastes[:2], (oh, ow), device=DEV)
    assert torch.equal(got_i[0], torch.where(mem[..., None], don_i, base_i)) and torch.equal(got_m[0], torch.where(mem, don_m, base_m))
    assert torch.equal(got_i[1], torch.where(mem.flip(1)[..., None], don_i.flip(1), base_i))
    assert torch.equal(got_m[1], torch.where(mem.flip(1), don_m.flip(1), base_m))


def test_guards_give_the_restatements_result_and_stay_inside():
    """tables the wrapper would refuse or never make, given to the library itself"""
    _images, _masks, (src, off, sizes), (msrc, moff, _) = _batch()
    oh, ow = 16, 12
    descs, pastes = P.cases(oh, ow)
    tab, start = _tables(pastes, len(descs), oh, ow)
    want = _want(oh, ow)

    def check(what, differs=True, **kw):
        a = dict(src=src, src_bytes=len(src), offsets=off, sizes=sizes, n_images=4, msrc=msrc, mask_bytes=len(msrc), moff=moff,
                 descs=descs, start=start, tab=tab)
        a.update(kw)
        ref = P.paste_crops(a["src"], a["offsets"], a["sizes"], a["n_images"], a["msrc"], a["moff"], a["descs"], a["start"],
                            a["tab"], oh, ow, 0, 255, src_bytes=a["src_bytes"], mask_bytes=a["mask_bytes"])
        got = _launch(a["src"], a["src_bytes"], a["offsets"], a["sizes"], a["n_images"], a["msrc"], a["mask_bytes"], a["moff"],
                      a["descs"], a["start"], a["tab"], oh, ow, 0, 255)
        _same(got, ref, what)
        assert differs == bool((ref[0] != want[0]).any() or (ref[1] != want[1]).any()), what
        return ref

    check("as packed", differs=False)
    for donor in (-1, 4):                               # a bad donor index: those pastes are skipped, the others stay
        ref = check(f"donor {donor}", tab=[(donor if j % 2 else d, b, box, dst) for j, (d, b, box, dst) in enumerate(tab)])
        assert np.array_equal(ref[0][7], want[0][7])
    # a bad base image: the whole crop is fill / ignore
    ref = check("base image 4", descs=[(4, a) if k == 2 else (i, a) for k, (i, a) in enumerate(descs)])
    assert (ref[0][2] == 0).all() and (ref[1][2] == 255).all()
    # image 1's mask past the end: its crops are ignore (their image stays a crop), pastes from it are skipped
    bad_off = np.array(moff).copy()
    bad_off[1] = len(msrc)
    ref = check("mask offset past the end", moff=bad_off)
    assert (ref[1][4] == 255).all() and (ref[1][6] == 255).all() and np.array_equal(ref[0][6], R.crop(_images[1], descs[6][1], oh, ow, 1, 0))
    # mask_bytes one short: image 3's mask is not readable
    ref = check("mask_bytes one short", mask_bytes=len(msrc) - 1)
    assert (ref[1][0] == 255).all() and not (ref[1][6] == 255).all()
    # src_bytes one short: image 3 is not readable, neither as a base nor as a donor
    ref = check("src_bytes one short", src_bytes=len(src) - 1)
    assert (ref[0][0] == 0).all() and (ref[1][0] != 255).any()
    # paste_start: descending (owns nothing), out of order, pointing outside the table (clamped into it)
    ref = check("paste_start descending", start=start[::-1].copy())
    assert all(len(seen) == 0 for seen in ref[2])
    jumbled = start.copy()
    jumbled[3], jumbled[5] = start[5], start[3]
    check("paste_start out of order", start=jumbled)
    check("paste_start outside", start=(start.astype(np.int64) * 1000 + 5).astype(np.int32))
    check("paste_start negative", start=(start - 1000).astype(np.int32))


def test_unaligned_outputs_wide_rows_and_many_rows():
    """the byte path on a dword-able shape (both outputs off by 1, 2, 3 bytes); rows of more than one block segment on
    both paths (87 and 344 pixels); more rows than the grid has blocks"""
    images, masks, (src, off, sizes), (msrc, moff, _) = _batch()
    descs, pastes = P.cases(16, 12)
    tab, start = _tables(pastes, len(descs), 16, 12)
    want = _want(16, 12)
    for mis in (1, 2, 3):
        _same(_launch(src, len(src), off, sizes, 4, msrc, len(msrc), moff, descs, start, tab, 16, 12, 0, 255, misalign=mis), want, mis)
    host = ([torch.from_numpy(im) for im in images], [torch.from_numpy(m) for m in masks])
    box_a, box_b = P.BLOBS[3][0][1], P.BLOBS[3][1][1]
    for oh, ow in ((3, 87), (2, 344)):
        d = [(3, R.crop_matrix(20.0, 16.0, 0.1, 12.0, False, oh, ow)), (1, R.crop_matrix(4.0, 6.0, 0.03, -20.0, True, oh, ow)),
             (3, P.shift(1, -(ow // 2)))]                # inside for 40 columns from the middle on
        p = [(0, 3, P.paste_matrix(24.0, 19.0, 0.08, 20.0, False, ow / 2, oh / 2), box_b),
             (0, 1, P.paste_matrix(4.5, 6.0, 0.05, 0.0, True, ow / 4, oh / 2), P.BLOBS[1][0][1]),
             (1, 3, P.paste_matrix(10.0, 8.0, 0.1, -30.0, False, 3 * ow / 4, oh / 2), box_a),
             (2, 3, P.paste_matrix(10.0, 8.0, 0.2, 0.0, False, ow // 2 + 15.0, 1.0), box_a)]
        t, st = _tables(p, 3, oh, ow)
        ref = P.paste_crops(src, off, sizes, 4, msrc, moff, d, st, t, oh, ow, 0, 255)
        assert all(s["alpha"].any() for seen in ref[2] for s in seen) and sum(len(seen) for seen in ref[2]) == 4
        got = crops.paste_crops_u8(host[0], host[1], d, p, (oh, ow), device=DEV)
        _same((got[0].cpu().numpy(), got[1].cpu().numpy()), ref, (oh, ow))
    # 1100 crops of 16 x 12 = 17600 rows: past 16384 blocks they stride over the crops
    many_d = (descs[:8] * 138)[:1100]
    many_p = [(k, donor, b, box) for k in range(1100) for crop, donor, b, box in pastes if crop == k % 8]
    got = crops.paste_crops_u8(host[0], host[1], many_d, many_p, (16, 12), device=DEV)
    assert np.array_equal(got[0].cpu().numpy(), np.concatenate([want[0][:8]] * 138)[:1100])
    assert np.array_equal(got[1].cpu().numpy(), np.concatenate([want[1][:8]] * 138)[:1100])


# ------------------------------------------------------------------------------------------------ Gear batches
@pytest.fixture(scope="module")
def gear_batch(tmp_path_factory):
    root = write_synthetic_gear(str(tmp_path_factory.mktemp("gear_paste")), seed=5)
    ds = GearDataset(root, "train", raw=True)
    images, polys, sizes, _paths = collate_raw([ds[i] for i in range(5)])
    assert len(set(sizes)) == 3 and len(polys["classes"]) > 0
    by_size = {hw: augment.polygon_masks_u8(polys, sizes, hw[0], hw[1], device=DEV) for hw in set(sizes)}
    masks = [by_size[hw][i] for i, hw in enumerate(sizes)]
    return images, polys, sizes, masks


@pytest.mark.parametrize("train", [True, False])
def test_gear_crop_preprocess_with_pastes_replays_to_the_reference(gear_batch, train):
    images, polys, sizes, masks = gear_batch
    crop_hw = (24, 32)
    kw = dict(train=train, crops_per_image=3, scale_range=(0.5, 3.0), degrees=25.0, seed=9)
    sampler = crops.PasteSampler(crop_hw, paste_p=1.0, max_pastes=3, scale_range=(0.5, 2.0), degrees=180.0, seed=9)
    pre = crops.GearCropPreprocess(crop_hw, paste=sampler, **kw)
    params = pre.draw(sizes, polys)
    k = 3 * len(sizes)
    assert len(params["image"]) == k and {p[0] for p in params["pastes"]} == set(range(k))
    x, m = pre(images, polys, sizes, device=DEV, params=params)
    assert x.dtype == torch.float32 and tuple(x.shape) == (k, 3, 24, 32) and m.dtype == torch.long and tuple(m.shape) == (k, 24, 32)

    descs = [(i, R.crop_matrix(cx, cy, s, a, f, *crop_hw)) for i, cx, cy, s, a, f in
             zip(params["image"], params["cx"], params["cy"], params["scale"], params["angle"], params["flip"])]
    pastes = [(c, i, P.paste_matrix(cx, cy, s, a, f, tx, ty), box) for c, i, _cls, cx, cy, s, a, f, tx, ty, box in params["pastes"]]
    assert pastes == crops.PasteSampler.table(params["pastes"])
    src, off, sz = P.pack([t.numpy() for t in images])
    msrc, moff, _ = P.pack([t.cpu().numpy() for t in masks])
    tab, start = _tables(pastes, k, *crop_hw)
    want_i, want_m, info = P.paste_crops(src, off, sz, len(sz), msrc, moff, descs, start, tab, 24, 32, 0, 255)
    acted = sum(bool(s["label"].any() and s["image"].any()) for seen in info for s in seen)
    assert acted >= 5                                   # pastes do land
    assert np.array_equal(m.cpu().numpy(), want_m.astype(np.int64))
    jitter = augment.jitter_table(params["orders"], params["brightness"], params["contrast"], params["saturation"],
                                  params["hue"]) if train else None
    assert torch.equal(x, augment.color_jitter_normalize_u8(torch.from_numpy(want_i).to(DEV), jitter))
    # drawing inside the call: a second object with the same seeds makes the same batch
    again = crops.GearCropPreprocess(crop_hw, paste=crops.PasteSampler(crop_hw, paste_p=1.0, max_pastes=3, scale_range=(0.5, 2.0),
                                                                       degrees=180.0, seed=9), **kw)
    x2, m2 = again(images, polys, sizes, device=DEV)
    assert torch.equal(x2, x) and torch.equal(m2, m)
    # paste_p = 0 is no pasting at all: the batches of paste=None, byte for byte
    none = crops.GearCropPreprocess(crop_hw, **kw)
    zero = crops.GearCropPreprocess(crop_hw, paste=crops.PasteSampler(crop_hw, paste_p=0.0, seed=9), **kw)
    for _ in range(2):
        (xa, ma), (xb, mb) = none(images, polys, sizes, device=DEV), zero(images, polys, sizes, device=DEV)
        assert torch.equal(xa, xb) and torch.equal(ma, mb)


# ------------------------------------------------------------------------------------------------ CLI
def test_train_gear_paste_round_trip(tmp_path, capsys):
    exp = train_gear_paste.main(["--synthetic", "--epochs", "1", "--crop_size", "64", "64", "--crops_per_image", "2",
                                 "--batch_size", "4", "--min_overlap", "16", "--num_workers", "0", "--precision", "bf16",
                                 "--copy_paste", "1", "--save_dir", str(tmp_path / "runs")])
    assert os.path.basename(exp).startswith("gear_paste_seg_unet_") and os.path.dirname(exp) == str(tmp_path / "runs")
    for sub in ("checkpoints", "results", "visualizations", "logs"):
        assert os.path.isdir(os.path.join(exp, sub)), sub
    args = json.load(open(os.path.join(exp, "args.json")))
    assert set(args) == {name[2:] for name, _ in train_gear_paste.FLAGS}
    assert (args["copy_paste"], args["max_pastes"], args["paste_scale_range"], args["paste_degrees"]) == (1.0, 2, [0.75, 1.33], 180.0)
    assert args["crop_size"] == [64, 64] and args["precision"] == "bf16" and "image_size" not in args
    res = json.load(open(os.path.join(exp, "results", "training_results.json")))
    assert set(res) == {"train_losses", "val_losses", "best_val_miou", "total_epochs", "total_params", "num_classes", "args"}
    assert len(res["train_losses"]) == 1 and len(res["val_losses"]) == 1 and res["num_classes"] == 4
    assert all(math.isfinite(v) and v > 0 for v in res["train_losses"] + res["val_losses"])
    printed = capsys.readouterr().out
    drawn = [line for line in printed.splitlines() if line.startswith("Pastes drawn: ")]
    assert len(drawn) == 1 and int(drawn[0].split()[2]) >= 4 and "Copy-paste: 1.00 of the crops" in printed
    ckpt = os.path.join(exp, "checkpoints", "checkpoint_epoch_0.pth")
    assert os.path.exists(ckpt)

    source = os.path.join(args["data_root"], "images", "test")
    out = tmp_path / "pred"
    predict_tiled.main(["--task", "gear", "--checkpoint", ckpt, "--input", source, "--tile", "64", "64", "--min_overlap", "16",
                        "--batch_size", "4", "--num_workers", "0", "--precision", "bf16", "--output_dir", str(out)])
    got = json.load(open(out / "predictions.json"))
    files = sorted(glob.glob(os.path.join(source, "*.png")))
    assert [e["image_path"] for e in got["images"]] == files and len(files) == 5
    assert all(os.path.exists(out / "masks" / (e["name"] + ".png")) for e in got["images"])
