"""GPU tests of the per-defect records (csrc/defects.hip through ops.describe_class_regions) against the numpy
restatement of tests/_defects_ref.py (pinned by test_cpu_defects.py), and of the predict CLI end to end.  Everything is
integer arithmetic, the confidence included (16.16 fixed point): every field is compared for equality.  The frames are
the smallest at which the accumulation can go wrong: waves of many regions, waves and blocks of one region, regions
across rows, tiles and blocks, a root far from its box, one region per pixel, a record buffer that is too short."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import _defects_ref as D
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import defects, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _confidence(maps, C, seed):
    """random fp32 in [0, 1] with exact 0 and 1 and ties (k + 0.5) / 65536 on class pixels"""
    rng = np.random.default_rng(seed)
    conf = rng.random(maps.shape, dtype=np.float32)
    on = np.flatnonzero((maps >= 1) & (maps < C))
    k = np.array([0, 1, 2, 3, 100, 101, 32767, 32768, 65534, 65535], np.float32)
    special = np.concatenate([np.array([0.0, 1.0], np.float32), (k + np.float32(0.5)) / np.float32(65536)])
    spots = on[np.linspace(0, on.size - 1, 3 * special.size).astype(np.int64)]
    conf.reshape(-1)[spots] = np.tile(special, 3)
    return conf


@functools.lru_cache(maxsize=None)
def _case(name):
    """(maps uint8 [n, h, w], C, conf fp32 [n, h, w]); built once, never modified"""
    rng = np.random.default_rng(7)
    if name == "speckle":                              # p ~ 0.3 of three classes; 4, 200 and 255 are background
        maps = rng.choice(np.array([0] * 14 + [1, 1, 2, 2, 3, 3] + [4, 200, 255], np.uint8), (2, 37, 53))
        C = 4
    elif name == "blob":                               # every wave and every block shares one root
        maps, C = np.ones((1, 512, 512), np.uint8), 2
    elif name == "stripes":                            # every wave mixes roots; every region spans all rows
        maps, C = np.broadcast_to(np.where(np.arange(48) % 6 < 3, 1, 0).astype(np.uint8), (1, 40, 48)).copy(), 3
    elif name == "ushape":
        m = np.zeros((70, 130), np.uint8)
        m[5:61, 100:105] = 1                           # right arm: the root (5, 100) is far from the box corner (20, 5)
        m[56:61, 20:105] = 1
        m[30:61, 20:25] = 1
        m[10:31, 105:111] = 2                          # another class touching the right arm
        m[30:55, 26:41] = 1                            # the same class one background pixel away, diagonally too
        m[62:64, 106:108] = 1                          # ... and past the corner (60, 104): (61, 105) is background
        maps, C = m[None], 3
    elif name == "pixels":                             # one region per pixel
        yy, xx = np.mgrid[0:16, 0:24]
        maps, C = (1 + 2 * (yy % 2) + xx % 2).astype(np.uint8)[None], 5
    else:
        raise KeyError(name)
    maps.setflags(write=False)
    conf = np.ones(maps.shape, np.float32) if name == "blob" else _confidence(maps, C, len(name))
    conf.setflags(write=False)
    return maps, C, conf


@functools.lru_cache(maxsize=None)
def _want(name, with_conf=True, min_pixels=1, image_base=0):
    maps, C, conf = _case(name)
    rec = D.describe_records(maps, C, conf if with_conf else None, min_pixels, image_base)
    rec.setflags(write=False)
    return rec


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cases are read-only


def _got(name, with_conf=True, **kw):
    maps, C, conf = _case(name)
    return ops.describe_class_regions(_dev(maps), C, _dev(conf) if with_conf else None, **kw)


def _assert_equal(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: first difference at record {bad[0][0]} field {ops.DEFECT_FIELDS[bad[0][1]]}: " \
                          f"{got[bad[0][0]].tolist()} != {want[bad[0][0]].tolist()}"


@pytest.mark.parametrize("name", ["speckle", "blob", "stripes", "ushape", "pixels"])
def test_records_equal_the_reference(name):
    want = _want(name)
    _assert_equal(_got(name), want, name)
    maps = _case(name)[0]
    if name == "blob":
        assert want.tolist() == [[0, 1, 0, 1 << 18, 0, 0, 511, 511, 511 * (1 << 17), 511 * (1 << 17), 1 << 34, 1 << 16]]
    if name == "speckle":
        assert {4, 200, 255} <= set(np.unique(maps).tolist()) and set(want[:, 1].tolist()) == {1, 2, 3}
        assert len(want) > 200 and set(want[:, 0].tolist()) == {0, 1}
    if name == "stripes":
        assert len(want) == 8 and want[:, 3].tolist() == [120] * 8 and want[:, 7].tolist() == [39] * 8
    if name == "ushape":
        assert want[:, 1].tolist() == [1, 2, 1, 1]
        assert want[0, 2] == 5 * 130 + 100 and want[0, 4:8].tolist() == [20, 5, 104, 60]
    if name == "pixels":
        assert len(want) == 16 * 24 and want[:, 3].tolist() == [1] * 384


def test_two_runs_are_bitwise_equal():
    first = _got("speckle")
    for _ in range(2):
        assert _got("speckle").tobytes() == first.tobytes()


def test_options_min_pixels_image_base_and_no_confidence():
    _assert_equal(_got("speckle", min_pixels=5), _want("speckle", True, 5), "min_pixels 5")
    assert 0 < len(_want("speckle", True, 5)) < len(_want("speckle"))
    _assert_equal(_got("speckle", image_base=1000), _want("speckle", True, 1, 1000), "image_base 1000")
    got = _got("speckle", with_conf=False)
    _assert_equal(got, _want("speckle", False), "conf None")
    assert not got[:, 10:].any()
    _assert_equal(_got("speckle", with_conf=False, min_pixels=5, image_base=1000), _want("speckle", False, 5, 1000), "all")
    nothing = ops.describe_class_regions(torch.zeros((2, 9, 9), dtype=torch.uint8, device=DEV), 4)
    assert nothing.shape == (0, 12) and nothing.dtype == np.int64
    # the loaders' int64 masks and bf16 / fp64 confidences are taken as label_class_regions and seg_confidence give them
    maps, C, conf = _case("ushape")
    wide = ops.describe_class_regions(_dev(maps.astype(np.int64)), C, _dev(conf.astype(np.float64)))
    _assert_equal(wide, _want("ushape"), "int64 labels, fp64 conf")


MARGIN = 256    # bytes of sentinel on each side of every buffer
SENTINEL = 0xA5


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + MARGIN


@pytest.mark.parametrize("capacity", [16 * 24, 100], ids=["fits", "short"])
def test_one_region_per_pixel_and_a_short_record_buffer(capacity):
    maps, C, conf = _case("pixels")
    n, h, w = maps.shape
    want = _want("pixels")
    md, cd = _dev(maps), _dev(conf)
    region, sizes, _ = ops.label_class_regions(md, C)
    lib, vp = L.lib(), ctypes.c_void_p
    need = lib.unet_describe_class_regions_workspace(n, h, w, C)
    assert need == (n * h * w * 4 + 15) // 16 * 16
    bufs = {k: _guarded(b) for k, b in (("records", capacity * 12 * 8), ("count", 8), ("ws", need))}
    bufs["count"][0][MARGIN:-MARGIN] = 0
    L.check(lib.unet_describe_class_regions(vp(md.data_ptr()), vp(region.data_ptr()), vp(sizes.data_ptr()),
                                            vp(cd.data_ptr()), n, h, w, C, 1, 0, vp(bufs["records"][1]), capacity,
                                            vp(bufs["count"][1]), vp(bufs["ws"][1]), need, None),
            "unet_describe_class_regions")
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():                   # the guard behind (and before) every buffer is untouched
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all()), k
    assert bufs["count"][0][MARGIN:-MARGIN].view(torch.int64).tolist() == [h * w]      # counted, written or not
    kept = bufs["records"][0][MARGIN:-MARGIN].view(torch.int64).cpu().numpy().reshape(capacity, 12)
    kept = kept[np.lexsort((kept[:, 2], kept[:, 0]))]
    if capacity == h * w:
        _assert_equal(kept, want, "capacity h w")
    else:
        assert len(np.unique(kept[:, 2])) == capacity  # different records, each one of the reference's
        _assert_equal(kept, want[np.searchsorted(want[:, 2], kept[:, 2])], "the first 100 slots")


def test_count_is_added_to():
    maps, C, conf = _case("stripes")
    n, h, w = maps.shape
    md, cd = _dev(maps), _dev(conf)
    region, sizes, _ = ops.label_class_regions(md, C)
    lib, vp = L.lib(), ctypes.c_void_p
    records = torch.zeros((16, 12), dtype=torch.int64, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.unet_describe_class_regions_workspace(n, h, w, C), dtype=torch.uint8, device=DEV)
    for base in (0, 1):
        L.check(lib.unet_describe_class_regions(vp(md.data_ptr()), vp(region.data_ptr()), vp(sizes.data_ptr()),
                                                vp(cd.data_ptr()), n, h, w, C, 1, base, vp(records.data_ptr()), 16,
                                                vp(count.data_ptr()), vp(ws.data_ptr()), ws.numel(), None), "describe")
    assert count.tolist() == [16]
    got = records.cpu().numpy()
    _assert_equal(got[np.lexsort((got[:, 2], got[:, 0]))], np.concatenate([_want("stripes"), _want("stripes", True, 1, 1)]),
                  "two calls into one buffer")


def test_refused_shapes_raise_before_any_launch():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    for c in (1, 256):
        with pytest.raises(RuntimeError, match="2..255 classes"):
            ops.describe_class_regions(x, c)
    with pytest.raises(RuntimeError, match="2..255 classes"):         # n h w = 2^31: a view, no memory behind it
        ops.describe_class_regions(x[:1, :1, :1].expand(1, 1 << 16, 1 << 15), 4)
    with pytest.raises(RuntimeError, match="2..255 classes"):         # n = 65536
        ops.describe_class_regions(x[:1, :1, :1].expand(65536, 1, 1), 4)
    with pytest.raises(ValueError, match="min_pixels"):
        ops.describe_class_regions(x, 4, min_pixels=0)
    with pytest.raises(ValueError):
        ops.describe_class_regions(x, 4, conf=torch.zeros((2, 8, 9), device=DEV))
    with pytest.raises(ValueError):
        ops.describe_class_regions(x, 4, conf=x)                     # not a float tensor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.describe_class_regions(x.cpu(), 4)


# ------------------------------------------------------------------------------------------------ CLI
def _run(*argv):
    res = subprocess.run([sys.executable, "-m", "tiaozhanbei_unet_amd.predict", *argv], cwd=ROOT, capture_output=True,
                         text=True, timeout=400)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return res.stdout


def test_predict_cli_round_trip(tmp_path):
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd import gear_dataset as G
    from tiaozhanbei_unet_amd.augment import DeviceTransform
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    source = os.path.join(root, "images", "test")      # no label files beside the images
    paths = sorted(os.path.join(source, f) for f in os.listdir(source))
    assert len(paths) == 5 and len({Image.open(p).size for p in paths}) > 1
    ckpt = tmp_path / "model.pth"
    torch.manual_seed(1)
    model = SegmentationUNet(3, 4, precision="fp32").to(DEV)
    save_checkpoint(model, get_optimizer(model), 0, 0.0, str(ckpt))

    # the same files through an eval pass in this process, in the CLI's batches of three
    tf = DeviceTransform((64, 64), train=False)
    model.eval()
    expected = []
    with torch.no_grad():
        for i in range(0, len(paths), 3):
            batch = [torch.from_numpy(np.array(Image.open(p).convert("RGB"), dtype=np.uint8)) for p in paths[i:i + 3]]
            expected.append(ops.seg_confidence(model(tf(batch, None, device=DEV)), conf=False)[0].cpu().numpy())
    expected = np.concatenate(expected)

    out = tmp_path / "frame"
    common = ["--task", "gear", "--checkpoint", str(ckpt), "--input", source, "--image_size", "64", "64", "--batch_size",
              "3", "--num_workers", "0"]
    text = _run(*common, "--output_dir", str(out), "--mask_size", "frame", "--save_overlays")
    assert "Predictions saved to" in text
    res = json.load(open(out / "predictions.json"))
    assert set(res) == {"args", "class_names", "frame_size", "images", "summary"}
    names = ["background", "pitting", "spalling", "scrape"]
    assert res["class_names"] == names and res["frame_size"] == [64, 64] and res["args"]["num_classes"] == 4
    assert [e["image_path"] for e in res["images"]] == paths           # every image, in order
    palette = ops.class_palette(4, "index").numpy()
    total = {name: 0 for name in names[1:]}
    for k, e in enumerate(res["images"]):
        assert set(e) == {"image_path", "name", "original_size", "mean_confidence", "defect_pixels", "defects", "decision"}
        w0, h0 = Image.open(paths[k]).size
        assert e["original_size"] == [h0, w0] and e["name"] == os.path.splitext(os.path.basename(paths[k]))[0]
        png = Image.open(out / "masks" / (e["name"] + ".png"))
        assert png.mode == "P" and png.size == (64, 64)
        assert np.array_equal(np.array(png.getpalette()).reshape(-1, 3)[:5], palette[:5])
        mask = np.array(png)
        assert np.array_equal(mask, expected[k]), e["name"]            # the CLI's masks are the in-process pass's
        want = D.describe_records(mask[None], 4)
        assert [d["class"] for d in e["defects"]] == want[:, 1].tolist()
        assert [d["class_name"] for d in e["defects"]] == [names[c] for c in want[:, 1]]
        assert [d["pixels"] for d in e["defects"]] == want[:, 3].tolist()
        assert [d["bbox"] for d in e["defects"]] == want[:, 4:8].tolist()
        for d, r in zip(e["defects"], want.tolist()):
            assert d["centroid"] == [r[8] / r[3], r[9] / r[3]] and d["counted"] is True
            assert d["bbox_original"] == [r[4] * w0 // 64, r[5] * h0 // 64, -(-(r[6] + 1) * w0 // 64) - 1,
                                          -(-(r[7] + 1) * h0 // 64) - 1]
            assert 1 / 4 <= d["mean_confidence"] <= d["peak_confidence"] <= 1
        assert e["defect_pixels"] == {names[c]: int(want[want[:, 1] == c, 3].sum()) for c in (1, 2, 3)}
        assert e["defect_pixels"] == {names[c]: int((mask == c).sum()) for c in (1, 2, 3)}
        assert 1 / 4 - 1e-6 <= e["mean_confidence"] <= 1
        assert e["decision"] == ("reject" if len(want) else "accept")
        for d in e["defects"]:
            total[d["class_name"]] += 1
        sheet = Image.open(out / "overlays" / (e["name"] + ".png"))
        assert sheet.mode == "RGB" and sheet.size == (2 * 64 + 4, 64)
    assert res["summary"] == {"images": 5, "rejected": sum(e["decision"] == "reject" for e in res["images"]),
                              "defects": total}
    assert sum(total.values()) > 0                     # a random head predicts something

    full = tmp_path / "original"
    _run(*common, "--output_dir", str(full), "--min_confidence", "1.0", "--reject_classes", "scrape")
    again = json.load(open(full / "predictions.json"))
    assert not os.path.exists(full / "overlays")
    for k, (e, first) in enumerate(zip(again["images"], res["images"])):
        w0, h0 = Image.open(paths[k]).size
        png = Image.open(full / "masks" / (e["name"] + ".png"))
        assert png.mode == "P" and png.size == (w0, h0)
        want = Image.fromarray(expected[k]).resize((w0, h0), Image.NEAREST)
        assert np.array_equal(np.array(png), np.array(want)), e["name"]
        assert [d["bbox"] for d in e["defects"]] == [d["bbox"] for d in first["defects"]]
        assert e["decision"] == ("reject" if any(d["counted"] and d["class_name"] == "scrape" for d in e["defects"])
                                 else "accept")
        assert all(d["counted"] == (d["mean_confidence"] >= 1.0) for d in e["defects"])
