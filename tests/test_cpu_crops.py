"""CPU checks of crop training: the reference arithmetic of tests/_crops_ref.py on hand cases, crops.crop_matrix against
pinned ints, the export and host-side refusals of unet_affine_crop_u8, the wrapper's checks, the crop sampler's
guarantees, and the train_gear_crops CLI's flags and refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _crops_ref as R
from tiaozhanbei_unet_amd import _lib, crops, ops, train_gear, train_gear_crops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536


def _image(h, w, c, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [1, 3])
def test_reference_centre_to_centre_copies_and_flip_reverses(mode, c):
    img = _image(9, 11, c)
    a = [ONE, 0, 3 * ONE + ONE // 2, 0, ONE, 2 * ONE + ONE // 2]           # output (y, x) <- source (y + 2, x + 3)
    assert a == R.crop_matrix(3 + 6 / 2, 2 + 4 / 2, 1.0, 0.0, False, 4, 6)
    assert np.array_equal(R.crop(img, a, 4, 6, mode, 7), img[2:6, 3:9])
    f = R.crop_matrix(3 + 6 / 2, 2 + 4 / 2, 1.0, 0.0, True, 4, 6)
    assert f == [-ONE, 0, 8 * ONE + ONE // 2, 0, ONE, 2 * ONE + ONE // 2]
    assert np.array_equal(R.crop(img, f, 4, 6, mode, 7), img[2:6, 3:9][:, ::-1])


def test_reference_half_pixel_shift_is_the_rounded_mean_of_two_neighbours():
    row = np.array([10, 21, 30, 33, 255, 0], np.uint8).reshape(1, 6, 1)
    a = [ONE, 0, ONE, 0, ONE, ONE // 2]                                # u = x + 1.0: half way between pixels x and x + 1
    assert R.crop(row, a, 1, 5, 1, 0)[0, :, 0].tolist() == [16, 26, 32, 144, 128]
    assert R.crop(row, a, 1, 5, 0, 0)[0, :, 0].tolist() == [21, 30, 33, 255, 0]        # nearest: floor(u) = x + 1
    col = row.transpose(1, 0, 2)
    b = [ONE, 0, ONE // 2, 0, ONE, ONE]
    assert R.crop(col, b, 5, 1, 1, 0)[:, 0, 0].tolist() == [16, 26, 32, 144, 128]
    # a quarter: fx = 64 -> (192 p0 + 64 p1) / 256, rounded half up
    q = [ONE, 0, 3 * ONE // 4, 0, ONE, ONE // 2]
    assert R.crop(row, q, 1, 2, 1, 0)[0, :, 0].tolist() == [(192 * 10 + 64 * 21 + 128) // 256, (192 * 21 + 64 * 30 + 128) // 256]


@pytest.mark.parametrize("mode", [0, 1])
def test_reference_fills_exactly_where_the_nearest_pixel_is_outside(mode):
    img = _image(6, 7, 3, seed=1)
    for dy, dx in ((-2, 0), (3, 0), (0, -3), (0, 4), (-2, -3), (3, 4)):        # off the top, bottom, left, right, corners
        a = [ONE, 0, dx * ONE + ONE // 2, 0, ONE, dy * ONE + ONE // 2]
        out = R.crop(img, a, 6, 7, mode, 200)
        ys, xs = np.arange(6)[:, None] + dy, np.arange(7)[None, :] + dx
        inside = (ys >= 0) & (ys < 6) & (xs >= 0) & (xs < 7)
        assert np.array_equal(inside, R.inside_mask((6, 7), a, 6, 7)) and 0 < inside.sum() < inside.size
        assert np.all(out[~inside] == 200)
        assert np.array_equal(out[inside], img[np.clip(ys, 0, 5), np.clip(xs, 0, 6)][inside])
    # a rotated, enlarged footprint: fill and the inside test still agree, in both modes
    a = R.crop_matrix(3.0, 3.0, 2.0, 30.0, False, 8, 8)
    out, inside = R.crop(img, a, 8, 8, mode, 255), R.inside_mask((6, 7), a, 8, 8)
    assert 0 < inside.sum() < 64 and np.all(out[~inside] == 255)


def test_reference_guards():
    src = np.arange(100, dtype=np.uint8)
    assert R.readable(0, (5, 20), 1, 100) and R.readable(1, (11, 3), 3, 100) and not R.readable(2, (11, 3), 3, 100)
    assert not R.readable(-1, (2, 2), 1, 100) and not R.readable(0, (0, 4), 1, 100) and not R.readable(0, (4, -1), 1, 100)
    ident = [ONE, 0, ONE // 2, 0, ONE, ONE // 2]
    out = R.crops([(2, 3), (2, 3)], [(0, ident), (1, ident), (2, ident), (-1, ident)], 2, 3, 0, 9, c=1, offsets=[4, 95], src=src)
    assert out[0, :, :, 0].tolist() == [[4, 5, 6], [7, 8, 9]] and np.all(out[1:] == 9)


# ------------------------------------------------------------------------------------------------ crop_matrix
PINNED = [((10, 8, 1, 0, False, 4, 6), [65536, 0, 491520, 0, 65536, 425984]),
          ((10, 8, 1, 0, True, 4, 6), [-65536, 0, 819200, 0, 65536, 425984]),
          ((10, 8, 2, 90, False, 4, 6), [0, -131072, 851968, 131072, 0, 196608]),
          ((100.25, 50.5, 0.5, -37, True, 16, 12), [-26170, 19720, 6566015, 19720, 26170, 3004834]),
          ((960, 540, 1.5, 10, False, 512, 512), [96811, -17070, 42540931, 17070, 96811, 6292882]),
          ((20, 20, 4, 180, False, 8, 8), [-262144, 0, 2228224, 0, -262144, 2228224])]


@pytest.mark.parametrize("args,want", PINNED)
def test_crop_matrix_pinned(args, want):
    assert crops.crop_matrix(*args) == want == R.crop_matrix(*args)


def test_crop_matrix_maps_the_crop_centre_to_the_centre_and_refuses():
    rng = np.random.default_rng(5)
    for _ in range(200):
        cx, cy = rng.uniform(0, 4000, 2)
        s, ang, flip = rng.uniform(0.1, 4.0), rng.uniform(-180, 180), bool(rng.integers(2))
        h, w = (int(v) for v in rng.integers(1, 600, 2))
        a = crops.crop_matrix(cx, cy, s, ang, flip, h, w)
        assert a == R.crop_matrix(cx, cy, s, ang, flip, h, w)
        # the crop's centre (x + .5, y + .5) = (w / 2, h / 2) lands on (cx, cy): a2 holds the half-pixel terms
        u = a[0] * (w / 2 - 0.5) + a[1] * (h / 2 - 0.5) + a[2]
        v = a[3] * (w / 2 - 0.5) + a[4] * (h / 2 - 0.5) + a[5]
        assert abs(u / ONE - cx) < (w + h) / ONE + 1e-3 and abs(v / ONE - cy) < (w + h) / ONE + 1e-3
    for bad in (0.0, -1.0, 4.0001, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            crops.crop_matrix(5, 5, bad, 0, False, 4, 4)
    with pytest.raises(ValueError, match="fixed point"):
        crops.crop_matrix(40000.0, 5, 1.0, 0, False, 4, 4)              # 40000 * 65536 > 2^31
    with pytest.raises(ValueError, match="fixed point"):
        crops.crop_matrix(5, -33000.0, 1.0, 0, False, 4, 4)
    with pytest.raises(ValueError):
        crops.crop_matrix(float("inf"), 5, 1.0, 0, False, 4, 4)
    assert crops.crop_matrix(5, 5, 4.0, 0, False, 4, 4)[0] == 4 * ONE


# ------------------------------------------------------------------------------------------------ exports
def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "tiaozhanbei_unet_amd", "csrc", "Makefile")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    name = "unet_affine_crop_u8"
    assert re.search(rf"\b{name}\(", header) and "typedef struct unet_crop_desc" in header
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 14
    assert hasattr(handle, name) and handle.unet_abi_version() == 1
    assert ctypes.sizeof(_lib.CropDesc) == 32 == crops.CROP_DTYPE.itemsize
    assert re.search(r"^SRCS = .* crops\.hip\b", makefile, re.M)
    for n in ("crop_matrix", "affine_crops_u8", "CropSampler", "GearCropPreprocess"):
        assert hasattr(crops, n) and not hasattr(ops, n), n
    t = crops.crop_table([(2, [1, -2, 3, -4, 5, -6])])
    d = _lib.CropDesc.from_buffer_copy(t.tobytes())
    assert (d.image, list(d.a), d.reserved) == (2, [1, -2, 3, -4, 5, -6], 0)


def test_refusals_are_decided_on_the_host():
    """dummy device pointers: every call below is refused before anything could read them"""
    lib = _lib.lib()
    dummy = ctypes.c_void_p(64)

    def call(src=dummy, src_bytes=100, off=dummy, hw=dummy, n_images=2, c=3, desc=dummy, n_crops=3, out_h=4, out_w=5,
             mode=1, fill=0, dst=dummy):
        return lib.unet_affine_crop_u8(src, src_bytes, off, hw, n_images, c, desc, n_crops, out_h, out_w, mode, fill, dst,
                                       None)

    for name in ("src", "off", "hw", "desc", "dst"):
        assert call(**{name: None}) == -1 and b"null pointer" in lib.unet_last_error(), name
        assert b"unet_affine_crop_u8" in lib.unet_last_error()
    for c in (0, 2, 4, -1):
        assert call(c=c) == -2 and b"1 or 3 channels" in lib.unet_last_error(), c
    for mode in (-1, 2, 7):
        assert call(mode=mode) == -2 and b"0 nearest, 1 bilinear" in lib.unet_last_error(), mode
    for fill in (-1, 256, 1000):
        assert call(fill=fill) == -2 and b"fill" in lib.unet_last_error() and b"0..255" in lib.unet_last_error(), fill
    for kw in (dict(out_h=0), dict(out_w=0), dict(out_h=4097), dict(out_w=4097), dict(out_h=-3)):
        assert call(**kw) == -2 and b"1..4096" in lib.unet_last_error(), kw
    for n in (0, -1, 65536):
        assert call(n_crops=n) == -2 and b"crops (1..65535)" in lib.unet_last_error(), n
        assert call(n_images=n) == -2 and b"images (1..65535)" in lib.unet_last_error(), n
    for b in (0, -5):
        assert call(src_bytes=b) == -2 and b"src_bytes" in lib.unet_last_error(), b


def test_wrapper_checks_before_the_device():
    torch = pytest.importorskip("torch")
    img = torch.zeros((6, 7, 3), dtype=torch.uint8)
    ident = [ONE, 0, ONE // 2, 0, ONE, ONE // 2]
    ok = dict(images=[img], descs=[(0, ident)], out_hw=(4, 5), mode=1, fill=0)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            crops.affine_crops_u8(**dict(ok, **kw))

    bad("uint8", images=[img.float()])
    bad("uint8", images=[img[0]])
    bad("uint8", images=["image"])
    bad(r"\[N, H, W, C\]", images=img)
    bad("1 or 3", images=[torch.zeros((6, 7, 2), dtype=torch.uint8)])
    bad("channels", images=[img, torch.zeros((6, 7, 1), dtype=torch.uint8)])
    bad("16384", images=[torch.zeros((1, 16385, 1), dtype=torch.uint8)])
    bad("16384", images=[torch.zeros((0, 5, 1), dtype=torch.uint8)])
    bad("images", images=[])
    bad("names image 1", descs=[(0, ident), (1, ident)])
    bad("names image -1", descs=[(-1, ident)])
    bad("crops", descs=[])
    bad("int32", descs=[(0, ident[:5])])
    bad("int32", descs=[(0, [1 << 31] + ident[1:])])
    for hw in ((0, 5), (4, 4097), (-1, 4)):
        bad("4096", out_hw=hw)
    for mode in (2, -1, "cubic"):
        bad("mode", mode=mode)
    for fill in (-1, 256):
        bad("fill", fill=fill)
    for kw in ({}, dict(images=img[None]), dict(mode="nearest"), dict(device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crops.affine_crops_u8(**dict(ok, **kw))


# ------------------------------------------------------------------------------------------------ the sampler
def _footprint_inside(p, k, crop_hw, size):
    ex, ey = crops.footprint_half_extents(p["scale"][k], p["angle"][k], crop_hw)
    # the corners themselves: centre + scale R (+-W/2, +-H/2)
    t = math.radians(p["angle"][k])
    for sx in (-1, 1):
        for sy in (-1, 1):
            dx, dy = sx * crop_hw[1] / 2, sy * crop_hw[0] / 2
            x = p["cx"][k] + p["scale"][k] * (math.cos(t) * dx - math.sin(t) * dy)
            y = p["cy"][k] + p["scale"][k] * (math.sin(t) * dx + math.cos(t) * dy)
            if not (-1e-9 <= x <= size[1] + 1e-9 and -1e-9 <= y <= size[0] + 1e-9):
                return False
    return ex <= p["cx"][k] <= size[1] - ex and ey <= p["cy"][k] <= size[0] - ey


def test_sampler_is_deterministic_and_keeps_footprints_inside():
    pytest.importorskip("torch")
    crop_hw = (48, 64)
    sizes = [(400, 640), (300, 300), (1080, 1920)]                      # larger than any footprint: 1.5 * (64 + 48) / 2 * ...
    boxes = [[(5.0, 5.0, 30.0, 20.0), (600.0, 380.0, 640.0, 400.0)], [], [(900.0, 500.0, 1000.0, 600.0)]]
    a = crops.CropSampler(crop_hw, seed=11).draw(sizes, boxes, 1000)
    b = crops.CropSampler(crop_hw, seed=11).draw(sizes, boxes, 1000)
    c = crops.CropSampler(crop_hw, seed=12).draw(sizes, boxes, 1000)
    assert a == b and a != c
    assert set(a) == {"image", "cx", "cy", "scale", "angle", "flip", "defect"} and all(len(v) == 3000 for v in a.values())
    assert a["image"] == [0] * 1000 + [1] * 1000 + [2] * 1000
    assert all(_footprint_inside(a, k, crop_hw, sizes[a["image"][k]]) for k in range(3000))
    assert all(0.75 <= s <= 1.5 for s in a["scale"]) and all(-10.0 <= v <= 10.0 for v in a["angle"])
    assert 0.4 < np.mean(a["flip"]) < 0.6
    logs = np.log(a["scale"])                                           # log-uniform: the mean log is the middle
    assert abs(logs.mean() - (math.log(0.75) + math.log(1.5)) / 2) < 0.02
    assert not any(a["defect"][1000:2000])                              # the image without polygons
    assert 0.4 < np.mean(a["defect"][:1000]) < 0.6 and 0.4 < np.mean(a["defect"][2000:]) < 0.6
    # a box at the border is clamped away from: image 0's defect crops still lie inside (checked above)
    # an image smaller than the footprint: the centre is the middle of that axis
    small = crops.CropSampler(crop_hw, seed=3).draw([(20, 500)], [[]], 50)
    assert all(cy == 10.0 for cy in small["cy"]) and len(set(small["cx"])) > 40


def test_sampler_defect_fraction():
    pytest.importorskip("torch")
    crop_hw = (32, 32)
    sizes = [(1000, 1000), (800, 1200)]
    boxes = [[(400.0, 450.0, 520.0, 500.0), (300.0, 600.0, 310.0, 700.0)], [(500.0, 300.0, 700.0, 420.0)]]
    p = crops.CropSampler(crop_hw, defect_fraction=1.0, seed=0).draw(sizes, boxes, 500)
    assert all(p["defect"])
    for k in range(1000):
        assert any(x0 <= p["cx"][k] <= x1 and y0 <= p["cy"][k] <= y1 for x0, y0, x1, y1 in boxes[p["image"][k]]), k
    in_second = sum(300.0 <= p["cx"][k] <= 310.0 for k in range(500))
    assert 180 < in_second < 320                                        # a uniformly chosen polygon, not area-weighted
    p = crops.CropSampler(crop_hw, defect_fraction=0.0, seed=0).draw(sizes, boxes, 500)
    assert not any(p["defect"])
    p = crops.CropSampler(crop_hw, defect_fraction=1.0, seed=0).draw(sizes, [[], []], 100)
    assert not any(p["defect"])
    for kw in (dict(scale_range=(0.0, 1.0)), dict(scale_range=(2.0, 1.0)), dict(scale_range=(1.0, 4.5)),
               dict(defect_fraction=1.5), dict(flip_p=-0.1), dict(crop_hw=(0, 8)), dict(degrees=-1.0)):
        with pytest.raises(ValueError):
            crops.CropSampler(**dict(dict(crop_hw=crop_hw), **kw))


def test_polygon_boxes_and_descs():
    pytest.importorskip("torch")
    from tiaozhanbei_unet_amd.gear_dataset import flatten_polygons
    polys = flatten_polygons([[(0, [(3, 4), (10, 4), (7, 9)]), (7, [(0, 0), (1, 1), (2, 0)])], [],
                              [(2, [(5, 5), (6, 8), (2, 7)]), (1, [(0, 1), (4, 1), (4, 3)])]])
    assert crops.polygon_boxes(polys, 3) == [[(3.0, 4.0, 11.0, 10.0)], [], [(2.0, 5.0, 7.0, 9.0), (0.0, 1.0, 5.0, 4.0)]]
    sub = crops._subset_polygons(polys, [2])
    assert sub["images"].tolist() == [0, 0] and sub["offsets"].tolist() == [0, 3, 6] and sub["classes"].tolist() == [2, 1]
    assert sub["verts"].tolist() == [[5, 5], [6, 8], [2, 7], [0, 1], [4, 1], [4, 3]]
    s = crops.CropSampler((4, 6), seed=0)
    params = {"image": [1], "cx": [10], "cy": [8], "scale": [2], "angle": [90], "flip": [False], "defect": [False]}
    assert s.descs(params) == [(1, PINNED[2][1])]


# ------------------------------------------------------------------------------------------------ CLI
NEW_FLAGS = {"crop_size", "crops_per_image", "defect_fraction", "scale_range", "degrees", "min_overlap"}


def test_train_gear_crops_flags():
    args = vars(train_gear_crops.parse_args([]))
    base = {name[2:] for name, _ in train_gear.FLAGS}
    assert {"image_size", "sync_mask"} <= base
    assert set(args) == (base - {"image_size", "sync_mask"}) | NEW_FLAGS == {name[2:] for name, _ in train_gear_crops.FLAGS}
    ref = vars(train_gear.parse_args([]))
    assert all(args[k] == ref[k] for k in base - {"image_size", "sync_mask"})          # train_gear's defaults
    assert (args["crop_size"], args["crops_per_image"], args["defect_fraction"], args["scale_range"], args["degrees"],
            args["min_overlap"]) == ([512, 512], 4, 0.5, [0.75, 1.5], 10.0, 64)
    assert args["batch_size"] == 8
    own = vars(train_gear_crops.parse_args(["--crop_size", "64", "96", "--crops_per_image", "2", "--batch_size", "6",
                                            "--defect_fraction", "1", "--scale_range", "1", "4", "--degrees", "0",
                                            "--min_overlap", "63", "--precision", "bf16"]))
    assert (own["crop_size"], own["crops_per_image"], own["batch_size"], own["defect_fraction"], own["scale_range"],
            own["degrees"], own["min_overlap"], own["precision"]) == ([64, 96], 2, 6, 1.0, [1.0, 4.0], 0.0, 63, "bf16")
    assert vars(train_gear_crops.parse_args(["--scale_range", "0.5", "0.5", "--defect_fraction", "0"]))["scale_range"] == [0.5, 0.5]


@pytest.mark.parametrize("extra", [["--batch_size", "6"], ["--crops_per_image", "3"], ["--crops_per_image", "0"],
                                   ["--batch_size", "0"], ["--defect_fraction", "-0.1"], ["--defect_fraction", "1.5"],
                                   ["--scale_range", "0", "1"], ["--scale_range", "1.5", "0.75"], ["--scale_range", "1", "4.5"],
                                   ["--scale_range", "1"], ["--min_overlap", "512"], ["--min_overlap", "-1"],
                                   ["--crop_size", "64", "32", "--min_overlap", "32"], ["--crop_size", "0", "64"],
                                   ["--crop_size", "64"], ["--crop_size", "8192", "64"], ["--image_size", "512"],
                                   ["--sync_mask"], ["--degrees", "-5"]])
def test_train_gear_crops_refuses(extra):
    with pytest.raises(SystemExit):
        train_gear_crops.parse_args(extra)


def test_train_gear_crops_refuses_cpu():
    with pytest.raises(SystemExit) as e:
        train_gear_crops.main(["--device", "cpu", "--synthetic"])
    assert "no CPU path" in str(e.value)


def test_fit_segmentation_keeps_its_defaults():
    """the new keyword arguments are optional and default to the trainers' behaviour before them"""
    import inspect
    sig = inspect.signature(train_gear.fit_segmentation)
    assert sig.parameters["ignore_index"].default is None and sig.parameters["validate"].default is None
    assert sig.parameters["ignore_index"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(train_gear.train_seg_epoch).parameters["ignore_index"].default is None
