"""CPU checks of copy-paste augmentation: the export and host-side refusals of unet_paste_crop_u8, the wrapper's checks,
crops.paste_matrix against pinned ints, crops.paste_dst_box against the restatement of tests/_paste_ref.py, the paste
sampler's guarantees, the train_gear_paste CLI's flags and refusals, and that the fixture of tests/test_gpu_paste.py
exercises what it is meant to."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _crops_ref as R
import _paste_ref as P
from tiaozhanbei_unet_amd import _lib, crops, ops, train_gear_crops, train_gear_paste

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 65536
NAME = "unet_paste_crop_u8"


# ------------------------------------------------------------------------------------------------ exports
def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    csrc = os.path.join(ROOT, "tiaozhanbei_unet_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    assert re.search(rf"\b{NAME}\(", header) and "typedef struct unet_paste_desc" in header
    assert re.search(r"^#define UNET_PASTE_MAX 8$", header, re.M)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 20
    assert hasattr(handle, NAME) and handle.unet_abi_version() == 1
    assert ctypes.sizeof(_lib.PasteDesc) == 64 == crops.PASTE_DTYPE.itemsize
    assert crops.MAX_PASTES == 8 == P.PASTE_MAX
    assert re.search(r"^SRCS = .* paste\.hip\b", makefile, re.M)
    # one copy of the tap arithmetic, in the header both kernels include
    for f in ("crops.hip", "paste.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "croptaps.h"' in text and "Taps taps_of(" not in text, f
    assert "Taps taps_of(" in open(os.path.join(csrc, "croptaps.h")).read()
    for n in ("paste_matrix", "paste_dst_box", "paste_table", "paste_crops_u8", "PasteSampler", "PASTE_DTYPE"):
        assert hasattr(crops, n) and not hasattr(ops, n), n
    rec, start = crops.paste_table([(1, 2, [1, -2, 3, -4, 5, -6], (7, 8, 9, 10))], 2, 3, (4, 5))
    d = _lib.PasteDesc.from_buffer_copy(rec.tobytes())
    assert (d.image, list(d.b), list(d.box), d.reserved) == (2, [1, -2, 3, -4, 5, -6], [7, 8, 9, 10], 0)
    assert list(d.dst) == list(crops.paste_dst_box([1, -2, 3, -4, 5, -6], (7, 8, 9, 10), 4, 5)) and start.tolist() == [0, 0, 1]


def test_refusals_are_decided_on_the_host():
    """dummy device pointers: every call below is refused before anything could read them"""
    lib = _lib.lib()
    dummy = ctypes.c_void_p(64)

    def call(src=dummy, src_bytes=100, off=dummy, hw=dummy, n_images=2, masks=dummy, mask_bytes=40, moff=dummy, desc=dummy,
             n_crops=3, start=dummy, paste=dummy, n_pastes=2, out_h=4, out_w=5, fill=0, ignore=255, dst=dummy, dst_mask=dummy):
        return lib.unet_paste_crop_u8(src, src_bytes, off, hw, n_images, masks, mask_bytes, moff, desc, n_crops, start, paste,
                                      n_pastes, out_h, out_w, fill, ignore, dst, dst_mask, None)

    for name in ("src", "off", "hw", "masks", "moff", "desc", "start", "dst", "dst_mask", "paste"):
        assert call(**{name: None}) == -1 and b"null pointer" in lib.unet_last_error(), name
        assert NAME.encode() in lib.unet_last_error()
    for n in (-1, -100):
        assert call(n_pastes=n) == -2 and b"n_pastes" in lib.unet_last_error(), n
        assert call(n_pastes=n, paste=None) == -2 and b"n_pastes" in lib.unet_last_error(), n
    for v in (-1, 256, 1000):
        assert call(fill=v) == -2 and b"fill" in lib.unet_last_error() and b"0..255" in lib.unet_last_error(), v
        assert call(ignore=v) == -2 and b"ignore" in lib.unet_last_error() and b"0..255" in lib.unet_last_error(), v
    for kw in (dict(out_h=0), dict(out_w=0), dict(out_h=4097), dict(out_w=4097), dict(out_h=-3)):
        assert call(**kw) == -2 and b"1..4096" in lib.unet_last_error(), kw
    for n in (0, -1, 65536):
        assert call(n_crops=n) == -2 and b"crops (1..65535)" in lib.unet_last_error(), n
        assert call(n_images=n) == -2 and b"images (1..65535)" in lib.unet_last_error(), n
    for b in (0, -5):
        assert call(src_bytes=b) == -2 and b"src_bytes" in lib.unet_last_error(), b
        assert call(mask_bytes=b) == -2 and b"mask_bytes" in lib.unet_last_error(), b


def test_wrapper_checks_before_the_device():
    torch = pytest.importorskip("torch")
    img, msk = torch.zeros((6, 7, 3), dtype=torch.uint8), torch.zeros((6, 7), dtype=torch.uint8)
    ident = [ONE, 0, ONE // 2, 0, ONE, ONE // 2]
    ok = dict(images=[img], masks=[msk], descs=[(0, ident)], pastes=[(0, 0, ident, (1, 1, 3, 3))], out_hw=(4, 5))

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            crops.paste_crops_u8(**dict(ok, **kw))

    bad("uint8", images=[img.float()])
    bad(r"channels \(3\)", images=[torch.zeros((6, 7, 1), dtype=torch.uint8)])
    bad("images", images=[], masks=[])
    bad("2 masks for 1 images", masks=[msk, msk])
    bad("mask 0", masks=[msk.float()])
    bad("mask 0", masks=[torch.zeros((6, 8), dtype=torch.uint8)])
    bad("mask 0", masks=[torch.zeros((6, 7, 1), dtype=torch.uint8)])
    bad("mask 0", masks=["mask"])
    bad("names image 1", descs=[(1, ident)])
    bad("crops", descs=[])
    bad("4096", out_hw=(0, 5))
    for v in (-1, 256):
        bad("fill", fill=v)
        bad("ignore", ignore=v)
    bad("names crop 1 of 1", pastes=[(1, 0, ident, (1, 1, 3, 3))])
    bad("names crop -1", pastes=[(-1, 0, ident, (1, 1, 3, 3))])
    bad("names donor image 1 of 1", pastes=[(0, 1, ident, (1, 1, 3, 3))])
    bad("six int32", pastes=[(0, 0, ident[:5], (1, 1, 3, 3))])
    bad("six int32", pastes=[(0, 0, ident, (1, 1, 3))])
    bad("six int32", pastes=[(0, 0, [1 << 31] + ident[1:], (1, 1, 3, 3))])
    bad("paste 0 is not", pastes=[(0, 0, ident)])
    bad("9 pastes", pastes=[(0, 0, ident, (1, 1, 3, 3))] * 9)
    for kw in ({}, dict(pastes=[]), dict(pastes=[(0, 0, ident, (1, 1, 3, 3))] * 8), dict(device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crops.paste_crops_u8(**dict(ok, **kw))


def test_paste_table_sorts_stably_by_crop():
    ident = [ONE, 0, ONE // 2, 0, ONE, ONE // 2]
    pastes = [(2, 0, ident, (0, 0, 1, 1)), (0, 1, ident, (0, 0, 2, 2)), (2, 1, ident, (0, 0, 3, 3)), (0, 0, ident, (0, 0, 4, 4))]
    rec, start = crops.paste_table(pastes, 4, 2, (8, 8))
    assert start.dtype == np.int32 and start.tolist() == [0, 2, 2, 4, 4]
    assert rec["image"].tolist() == [1, 0, 0, 1] and rec["box"][:, 2].tolist() == [2, 4, 1, 3]
    assert rec["dst"].tolist() == [list(crops.paste_dst_box(ident, (0, 0, n, n), 8, 8)) for n in (2, 4, 1, 3)]
    rec, start = crops.paste_table([], 3, 2, (8, 8))
    assert len(rec) == 0 and start.tolist() == [0, 0, 0, 0]
    # the restatement's table maker agrees
    tab, st = P.tables(pastes, 4, lambda b, box: crops.paste_dst_box(b, box, 8, 8))
    assert st.tolist() == [0, 2, 2, 4, 4] and [t[0] for t in tab] == [1, 0, 0, 1]


def test_the_packing_helper_keeps_the_crop_layout():
    """affine_crops_u8's upload, now shared: the tables, then the host images, in one buffer"""
    torch = pytest.importorskip("torch")
    a, b = torch.arange(24, dtype=torch.uint8).reshape(2, 4, 3), torch.arange(100, 106, dtype=torch.uint8).reshape(1, 2, 3)
    m = torch.arange(200, 208, dtype=torch.uint8).reshape(2, 4)
    offsets, sizes, total = crops._layout([a, b])
    assert offsets.tolist() == [0, 24] and sizes.tolist() == [[2, 4], [1, 2]] and total == 30
    head = np.arange(5, dtype=np.uint8)
    tables, (src,) = crops._upload(head, [[a, b]], torch.device("cpu"))
    assert tables.tolist() == list(range(5)) + list(range(24)) + list(range(100, 106)) and src.tolist() == tables[5:].tolist()
    assert src.data_ptr() == tables.data_ptr() + 5                      # a view: one upload
    tables, (src, msk) = crops._upload(head, [[a, b], [m]], torch.device("cpu"))
    assert len(tables) == 5 + 30 + 8 and src.tolist() == tables[5:35].tolist() and msk.tolist() == list(range(200, 208))


# ------------------------------------------------------------------------------------------------ paste_matrix
PINNED = [((10, 8, 1, 0, False, 3, 2), [65536, 0, 491520, 0, 65536, 425984]),
          ((10, 8, 1, 0, True, 3, 2), [-65536, 0, 819200, 0, 65536, 425984]),
          ((10, 8, 2, 90, False, 0, 0), [0, -131072, 589824, 131072, 0, 589824]),
          ((100.25, 50.5, 0.5, 0, False, 7.25, 1.5), [32768, 0, 6348800, 0, 32768, 3276800])]


@pytest.mark.parametrize("args,want", PINNED)
def test_paste_matrix_pinned(args, want):
    assert crops.paste_matrix(*args) == want == P.paste_matrix(*args)


def test_paste_matrix_is_crop_matrix_about_another_point_and_refuses():
    rng = np.random.default_rng(7)
    for _ in range(200):
        cx, cy = rng.uniform(0, 4000, 2)
        s, ang, flip = rng.uniform(0.1, 4.0), rng.uniform(-180, 180), bool(rng.integers(2))
        h, w = (int(v) for v in rng.integers(1, 600, 2))
        assert crops.paste_matrix(cx, cy, s, ang, flip, w / 2, h / 2) == crops.crop_matrix(cx, cy, s, ang, flip, h, w)
        tx, ty = rng.uniform(0, w), rng.uniform(0, h)
        b = crops.paste_matrix(cx, cy, s, ang, flip, tx, ty)
        assert b == P.paste_matrix(cx, cy, s, ang, flip, tx, ty)
        # the target point (x + .5, y + .5) = (tx, ty) lands on the donor centre
        u, v = b[0] * (tx - 0.5) + b[1] * (ty - 0.5) + b[2], b[3] * (tx - 0.5) + b[4] * (ty - 0.5) + b[5]
        assert abs(u / ONE - cx) < (w + h) / ONE + 1e-3 and abs(v / ONE - cy) < (w + h) / ONE + 1e-3
    for bad in (0.0, -1.0, 4.0001, float("nan")):
        with pytest.raises(ValueError, match="paste_matrix: scale"):
            crops.paste_matrix(5, 5, bad, 0, False, 2, 2)
    with pytest.raises(ValueError, match="paste_matrix: the matrix is outside 16.16 fixed point"):
        crops.paste_matrix(40000.0, 5, 1.0, 0, False, 2, 2)
    with pytest.raises(ValueError):
        crops.paste_matrix(float("inf"), 5, 1.0, 0, False, 2, 2)


# ------------------------------------------------------------------------------------------------ paste_dst_box
def test_paste_dst_box_by_hand():
    ident = [ONE, 0, ONE // 2, 0, ONE, ONE // 2]
    # centre to centre: members at columns 2..4 reach, through a tap, nothing but themselves; the box may hold a ring more
    x0, y0, x1, y1 = crops.paste_dst_box(ident, (2, 1, 5, 3), 8, 8)
    assert x0 <= 2 and y0 <= 1 and x1 >= 5 and y1 >= 3 and (x0, y0) >= (1, 0) and (x1, y1) <= (6, 4)
    assert crops.paste_dst_box(ident, (2, 1, 2, 3), 8, 8) == (0, 0, 0, 0)                   # an empty donor box
    assert crops.paste_dst_box(ident, (20, 20, 25, 25), 8, 8) == (0, 0, 0, 0)               # lands outside the crop
    assert crops.paste_dst_box(ident, (-9, -9, 100, 100), 6, 7) == (0, 0, 7, 6)             # clamped to the crop
    assert crops.paste_dst_box([0, 0, ONE, 0, 0, ONE], (0, 0, 5, 5), 6, 7) == (0, 0, 7, 6)  # a singular matrix: everything


def test_paste_dst_box_holds_every_pixel_a_paste_can_change():
    """over random pastes the restatement gives the same bytes with the computed dst as with dst = the whole crop"""
    images, masks = P.fixture(seed=3)
    masks[3] = np.random.default_rng(1).integers(0, 4, (33, 40)).astype(np.uint8)          # members all over every image
    masks[0][:], masks[1][:], masks[2][:] = 1, 2, 3
    src, off, sizes = P.pack(images)
    msrc, moff, _ = P.pack(masks)
    rng = np.random.default_rng(11)
    n, acted, small = 320, 0, 0
    for oh, ow in ((9, 11), (16, 12)):
        descs = [(3, P.shift(2, 3))] * (n // 2)
        pastes = []
        for k in range(n // 2):
            donor = int(rng.choice([0, 1, 2, 3]))
            dh, dw = P.SIZES[donor]
            s = float(np.exp(rng.uniform(np.log(0.25), np.log(4.0))))
            x0, y0 = int(rng.integers(-3, dw)), int(rng.integers(-3, dh))           # touching and crossing the image's edges
            box = (x0, y0, x0 + int(rng.integers(1, dw + 4)), y0 + int(rng.integers(1, dh + 4)))
            b = crops.paste_matrix(rng.uniform(box[0] - 1, box[2] + 1), rng.uniform(box[1] - 1, box[3] + 1), s,
                                   rng.uniform(-180, 180), bool(rng.integers(2)), rng.uniform(0, ow), rng.uniform(0, oh))
            pastes.append((k, donor, b, box))
        tab, start = P.tables(pastes, len(descs), lambda b, box: crops.paste_dst_box(b, box, oh, ow))
        got = P.paste_crops(src, off, sizes, 4, msrc, moff, descs, start, tab, oh, ow, 0, 255)
        whole = P.paste_crops(src, off, sizes, 4, msrc, moff, descs, start, tab, oh, ow, 0, 255, whole_dst=True)
        assert int((got[0] != whole[0]).sum()) == 0 and int((got[1] != whole[1]).sum()) == 0
        for (_d, _b, _box, dst), seen in zip(tab, whole[2]):
            assert 0 <= dst[0] <= dst[2] <= ow and 0 <= dst[1] <= dst[3] <= oh
            acted += bool(seen[0]["alpha"].any())
            small += (dst[2] - dst[0]) * (dst[3] - dst[1]) < oh * ow
    assert acted >= 200 and small >= 100                   # 200 pastes that do something; boxes that spare some of the crop


# ------------------------------------------------------------------------------------------------ the sampler
def _polys():
    from tiaozhanbei_unet_amd.gear_dataset import flatten_polygons
    # class 0 once, class 2 nine times, class 1 never; image 1 has no polygon
    tri = lambda x, y: [(x, y), (x + 10, y), (x + 4, y + 6)]            # noqa: E731
    return flatten_polygons([[(0, tri(5, 5))] + [(2, tri(20 + 3 * j, 30)) for j in range(4)], [],
                             [(2, tri(7 * j, 11)) for j in range(5)]])


def test_sampler_is_deterministic_and_draws_classes_uniformly():
    pytest.importorskip("torch")
    polys, sizes = _polys(), [(100, 120), (50, 50), (80, 90)]
    crop_params = {"scale": [1.0 + 0.001 * k for k in range(3000)]}
    mk = lambda seed: crops.PasteSampler((48, 64), paste_p=0.5, max_pastes=3, scale_range=(0.5, 2.0), degrees=90.0, seed=seed)  # noqa: E731
    a, b, c = (mk(s).draw(crop_params, polys, sizes) for s in (11, 11, 12))
    assert a == b and a != c
    crop_of = [p[0] for p in a]
    assert crop_of == sorted(crop_of) and 0.45 < len(set(crop_of)) / 3000 < 0.55          # paste_p of the crops take pastes
    per_crop = np.bincount(np.bincount(crop_of, minlength=3000), minlength=4)
    assert per_crop[4:].sum() == 0 and all(abs(per_crop[n] - len(set(crop_of)) / 3) < 80 for n in (1, 2, 3))
    boxes = crops.polygon_boxes(polys, 3)
    for k, image, cls, cx, cy, s, ang, flip, tx, ty, box in a:
        assert cls in (0, 2) and image in (0, 2) and tuple(float(v) for v in box) in boxes[image]
        assert (cx, cy) == ((box[0] + box[2]) / 2, (box[1] + box[3]) / 2)
        assert 0.5 * crop_params["scale"][k] - 1e-9 <= s <= min(2.0 * crop_params["scale"][k], 4.0) + 1e-9
        assert -90.0 <= ang <= 90.0 and 0.0 <= tx <= 64.0 and 0.0 <= ty <= 48.0
    # one polygon of class 0 against nine of class 2: the CLASS is drawn uniformly, so each gets half of the pastes
    n0, n2 = sum(p[2] == 0 for p in a), sum(p[2] == 2 for p in a)
    assert (n0, n2) == (1522, 1435) and abs(n0 - n2) < 4 * math.sqrt(n0 + n2)
    assert mk(11).counts == {} and (lambda s: (s.draw(crop_params, polys, sizes), s.counts)[1])(mk(11)) == {0: n0, 2: n2}
    assert 0.45 < np.mean([p[7] for p in a]) < 0.55
    # within class 2 every polygon is as likely as another
    per_box = np.unique([p[10] for p in a if p[2] == 2], axis=0, return_counts=True)[1]
    assert len(per_box) == 9 and per_box.min() > n2 / 9 - 60 and per_box.max() < n2 / 9 + 60
    # the scale is clamped into (0, 4]
    big = mk(5).draw({"scale": [3.9] * 200}, polys, sizes)
    assert max(p[5] for p in big) == 4.0 and min(p[5] for p in big) >= 1.95
    m = crops.PasteSampler.table(a[:3])
    assert m[0] == (a[0][0], a[0][1], crops.paste_matrix(*a[0][3:10]), a[0][10])


def test_sampler_draws_nothing_without_polygons_or_probability():
    pytest.importorskip("torch")
    from tiaozhanbei_unet_amd.gear_dataset import flatten_polygons
    crop_params = {"scale": [1.0] * 50}
    s = crops.PasteSampler((48, 64), paste_p=1.0, max_pastes=8, seed=0)
    assert s.draw(crop_params, flatten_polygons([[], []]), [(50, 50)] * 2) == [] and s.counts == {}
    full = s.draw(crop_params, _polys(), [(100, 120), (50, 50), (80, 90)])
    assert {p[0] for p in full} == set(range(50)) and max(np.bincount([p[0] for p in full])) == 8
    assert "Pastes drawn: %d (pitting " % len(full) in s.report() and s.counts == {}
    assert crops.PasteSampler((48, 64), paste_p=0.0, seed=0).draw(crop_params, _polys(), [(100, 120), (50, 50), (80, 90)]) == []
    for kw in (dict(paste_p=1.5), dict(paste_p=-0.1), dict(max_pastes=0), dict(max_pastes=9), dict(scale_range=(0.0, 1.0)),
               dict(scale_range=(2.0, 1.0)), dict(scale_range=(1.0, 4.5)), dict(degrees=181.0), dict(crop_hw=(0, 8))):
        with pytest.raises(ValueError):
            crops.PasteSampler(**dict(dict(crop_hw=(48, 64)), **kw))


def test_pasting_leaves_the_crop_draws_alone():
    pytest.importorskip("torch")
    polys, sizes = _polys(), [(100, 120), (50, 50), (80, 90)]
    kw = dict(crop_hw=(24, 32), train=True, crops_per_image=3, scale_range=(0.5, 3.0), degrees=25.0, seed=9)
    plain = crops.GearCropPreprocess(**kw)
    pasted = crops.GearCropPreprocess(**kw, paste=crops.PasteSampler((24, 32), paste_p=1.0, max_pastes=2, seed=9))
    assert plain.paste is None
    for _ in range(3):                                  # batch after batch: the two generators never meet
        want, got = plain.draw(sizes, polys), pasted.draw(sizes, polys)
        assert "pastes" not in want and len(got.pop("pastes")) >= 9
        assert got == want
    with pytest.raises(ValueError, match="paste sampler"):
        crops.GearCropPreprocess(**kw, paste=crops.PasteSampler((24, 24)))


# ------------------------------------------------------------------------------------------------ CLI
NEW_FLAGS = {"copy_paste", "max_pastes", "paste_scale_range", "paste_degrees"}


def test_train_gear_paste_flags():
    args = vars(train_gear_paste.parse_args([]))
    base = vars(train_gear_crops.parse_args([]))
    assert set(base) == {name[2:] for name, _ in train_gear_crops.FLAGS} and NEW_FLAGS.isdisjoint(base)
    assert set(args) == set(base) | NEW_FLAGS == {name[2:] for name, _ in train_gear_paste.FLAGS}
    assert all(args[k] == base[k] for k in base)                        # train_gear_crops' defaults
    assert (args["copy_paste"], args["max_pastes"], args["paste_scale_range"], args["paste_degrees"]) == (0.5, 2, [0.75, 1.33], 180.0)
    own = vars(train_gear_paste.parse_args(["--copy_paste", "1", "--max_pastes", "8", "--paste_scale_range", "0.5", "4",
                                            "--paste_degrees", "0", "--crop_size", "64", "96", "--min_overlap", "16", "--precision", "bf16"]))
    assert (own["copy_paste"], own["max_pastes"], own["paste_scale_range"], own["paste_degrees"], own["crop_size"],
            own["precision"]) == (1.0, 8, [0.5, 4.0], 0.0, [64, 96], "bf16")
    assert callable(train_gear_crops.run) and callable(train_gear_crops.crop_preprocess)


@pytest.mark.parametrize("extra", [["--copy_paste", "-0.1"], ["--copy_paste", "1.5"], ["--max_pastes", "0"], ["--max_pastes", "9"],
                                   ["--paste_scale_range", "0", "1"], ["--paste_scale_range", "2", "1"],
                                   ["--paste_scale_range", "1", "4.5"], ["--paste_scale_range", "1"], ["--paste_degrees", "-1"],
                                   ["--paste_degrees", "181"], ["--batch_size", "6"], ["--crop_size", "0", "64"],
                                   ["--min_overlap", "512"], ["--image_size", "512"]])
def test_train_gear_paste_refuses(extra):
    with pytest.raises(SystemExit):
        train_gear_paste.parse_args(extra)


def test_train_gear_paste_refuses_cpu():
    with pytest.raises(SystemExit) as e:
        train_gear_paste.main(["--device", "cpu", "--synthetic"])
    assert "no CPU path" in str(e.value)


# ------------------------------------------------------------------------------------------------ the GPU test's fixture
def _run(oh, ow, pastes=None, ignore=255):
    images, masks = P.fixture()
    src, off, sizes = P.pack(images)
    msrc, moff, _ = P.pack(masks)
    descs, all_pastes = P.cases(oh, ow)
    tab, start = P.tables(all_pastes if pastes is None else pastes, len(descs), lambda b, box: crops.paste_dst_box(b, box, oh, ow))
    return P.paste_crops(src, off, sizes, 4, msrc, moff, descs, start, tab, oh, ow, 0, ignore), (images, masks, descs, all_pastes)


@pytest.mark.parametrize("oh,ow", [(4, 5), (16, 12), (8, 8)])
def test_the_fixture_is_not_vacuous(oh, ow):
    (img, lab, info), (images, masks, descs, pastes) = _run(oh, ow)
    counts = [sum(p[0] == k for p in pastes) for k in range(len(descs))]
    assert counts == [1, 1, 2, 3, 1, 4, 8, 0, 9] and [len(s) for s in info] == counts[:8] + [8]       # the ninth is not looked at
    for k in range(8):
        for j, seen in enumerate(info[k]):
            assert seen["label"].any() and seen["image"].any(), (k, j)
    soft = sum(int(((s["alpha"] > 0) & (s["alpha"] < 65536)).sum()) for seen in info for s in seen)
    assert soft > 50
    # centre to centre: alpha is all or nothing, and the flipped paste is the mirror image
    assert set(np.unique(info[0][0]["alpha"])) == {0, 65536} and np.array_equal(info[1][0]["alpha"], info[0][0]["alpha"][:, ::-1])
    # the member rule: 255 (the ignore value) is never carried over, 200 is
    assert 200 in lab[0] and 200 in masks[3] and 255 in masks[3]
    base = R.crop(masks[3][..., None], descs[0][1], oh, ow, 0, 255)[..., 0]
    assert not ((lab[0] == 255) & (base != 255)).any()
    (_i9, lab9, _), _ = _run(oh, ow, ignore=9)                           # with another ignore value 255 is a label like any
    assert ((lab9[0] == 255) & (base != 255)).any()
    # the crop that hangs off its image: the paste reaches its fill rows, and nothing lands there
    outside = ~R.inside_mask(P.SIZES[1], descs[4][1], oh, ow)
    whole = _run(oh, ow)[0]
    assert outside.any() and (lab[4][outside] == 255).all() and (lab[4][~outside] != 255).all() and (img[4][outside] == 0).all()
    ys = np.nonzero(info[4][0]["alpha"].any(1))[0]
    assert ys.min() == np.nonzero(~outside.all(1))[0].min()             # cut by the fill, not by its own extent
    assert np.array_equal(whole[0], img)
    # the order of the two overlapping pastes on crop 2 matters
    i2 = [j for j, p in enumerate(pastes) if p[0] == 2]
    swapped = list(pastes)
    swapped[i2[0]], swapped[i2[1]] = pastes[i2[1]], pastes[i2[0]]
    (img_s, lab_s, _), _ = _run(oh, ow, pastes=swapped)
    assert (img_s[2] != img[2]).any() and (lab_s[2] != lab[2]).any()
    assert np.array_equal(np.delete(img_s, 2, 0), np.delete(img, 2, 0))
    # the restatement's own bilinear value is the crop rule's wherever that one is inside
    a = descs[2][1]
    y, x = np.meshgrid(np.arange(oh, dtype=np.int64), np.arange(ow, dtype=np.int64), indexing="ij")
    inside = R.inside_mask(P.SIZES[3], a, oh, ow)
    val = P.bilinear(images[3], a[0] * x + a[1] * y + a[2], a[3] * x + a[4] * y + a[5])
    assert inside.all() and np.array_equal(val.astype(np.uint8), R.crop(images[3], a, oh, ow, 1, 0))
