"""GPU tests of the shape records (csrc/shapes.hip through ops.measure_class_regions) against the numpy restatement of
tests/_shapes_ref.py (pinned by test_cpu_shapes.py), and of the predict CLIs' shape flags end to end.  Everything is
integer arithmetic: every field of every record is compared for equality.  The frames are the smallest at which the
accumulation can go wrong: waves of more regions than are reduced with shuffles, one region over every wave and block
and along all four frame edges, regions across the 2048-pixel block boundary, and the masks whose quads are special."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _defects_ref as D
import _shapes_ref as S
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import defects, ops, predict, predict_tiled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(name):
    """(maps uint8 [n, h, w], C); built once, never modified"""
    rng = np.random.default_rng(5)
    if name == "random":                               # p ~ 0.3 of three classes; 4, 200 and 255 are background
        maps, C = rng.choice(np.array([0] * 14 + [1, 1, 2, 2, 3, 3] + [4, 200, 255], np.uint8), (2, 33, 67)), 4
    elif name == "filled":                             # every wave and block shares one record; all four frame edges
        maps, C = np.ones((1, 96, 96), np.uint8), 2
    elif name == "long":                               # blocks end at the linear indices 2048, 4096, 6144
        m = np.zeros((3, 2051), np.uint8)
        m[0, :] = 1                                    # row 0 runs through 2048
        m[1, 2040:] = 2                                # linear 4091 .. 4101, under row 0 and not its class
        m[2, 2030:] = 3                                # linear 6132 .. 6152
        m[2, :100:2] = 2                               # single pixels
        m[2, 500:1500] = 1                             # a second region of class 1
        maps, C = m[None], 4
    elif name == "patterns":
        m = np.zeros((3, 37, 53), np.uint8)
        yy, xx = np.mgrid[0:37, 0:53]
        r2 = (yy - 15) ** 2 + (xx - 16) ** 2
        m[0][(r2 <= 14 ** 2) & (r2 >= 8 ** 2)] = 1     # a ring
        m[0][r2 <= 3 ** 2] = 1                         # ... with an island in its hole
        m[0, 20:36, 36:52][(yy[20:36, 36:52] + xx[20:36, 36:52]) % 2 == 0] = 2      # a checkerboard: diagonals only
        k = np.arange(30)
        m[1, 3 + k, 2 + k] = 3                         # a one-pixel diagonal chain
        m[1, 5:20, 35:42] = 1                          # two classes that touch along an edge and by corners
        m[1, 5:20, 42:50] = 2
        m[1, 20:25, 30:35] = 2
        m[2][(yy + xx) % 2 == 0] = 1                   # a checkerboard over the whole frame
        maps, C = m, 4
    else:
        raise KeyError(name)
    maps.setflags(write=False)
    return maps, C


@functools.lru_cache(maxsize=None)
def _want(name, min_pixels=1, image_base=0, directions=32):
    maps, C = _case(name)
    rec = S.shape_records(maps, C, min_pixels, image_base, directions)
    rec.setflags(write=False)
    return rec


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cases are read-only


def _got(name, **kw):
    maps, C = _case(name)
    return ops.measure_class_regions(_dev(maps), C, **kw)


def _assert_equal(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    fields = ops.shape_fields((want.shape[1] - S.HEAD) // 2)
    assert bad.size == 0, f"{what}: first difference at record {bad[0][0]} field {fields[bad[0][1]]}: " \
                          f"{got[bad[0][0]].tolist()} != {want[bad[0][0]].tolist()}"


@pytest.mark.parametrize("name", ["random", "filled", "long", "patterns"])
def test_records_equal_the_reference(name):
    want = _want(name)
    assert want.shape[1] == len(ops.SHAPE_FIELDS)
    _assert_equal(_got(name), want, name)
    if name == "random":
        assert len(want) > 200 and set(want[:, 0].tolist()) == {0, 1}
    if name == "filled":
        t = 95 * 96 * 191 // 6 * 96                    # sum of x^2 over a row, 96 rows
        assert want[0, :11].tolist() == [0, 0, 96 * 96, t, t, (95 * 96 // 2) ** 2, 4, 4 * 95, 0, 0, 95 * 95]
    if name == "long":
        assert want[:3, 1].tolist() == [0, 2051 + 2040, 2 * 2051] and want[:3, 2].tolist() == [2051, 11, 1]
    if name == "patterns":
        by_root = {(r[0], r[1]): r for r in want.tolist()}
        chain = by_root[(1, 3 * 53 + 2)]
        assert chain[2] == 30 and chain[6:11] == [62, 0, 29, 0, 0]
        board = by_root[(2, 0)]
        assert board[7] == 0 and board[9] == 0 and board[10] == 0 and board[8] == 36 * 52      # diagonal quads only
        ring = by_root[(0, 1 * 53 + 16)]
        assert (ring[6] - ring[9] - 2 * ring[8]) // 4 == 0                                      # one hole


def test_two_runs_are_bitwise_equal():
    first = _got("random")
    for _ in range(2):
        assert _got("random").tobytes() == first.tobytes()


def test_options_min_pixels_image_base_and_directions():
    maps, C = _case("random")
    _assert_equal(_got("random", min_pixels=5), _want("random", 5), "min_pixels 5")
    assert 0 < len(_want("random", 5)) < len(_want("random"))
    described = ops.describe_class_regions(_dev(maps), C, None, 5, 7)
    kept = _got("random", min_pixels=5, image_base=7)
    _assert_equal(kept, _want("random", 5, 7), "min_pixels 5, image_base 7")
    assert np.array_equal(kept[:, :3], described[:, [0, 2, 3]])          # the rows align: image, root, size
    _assert_equal(_got("random", image_base=7), _want("random", 1, 7), "image_base 7")
    for d in (2, 16):
        _assert_equal(_got("patterns", directions=d), _want("patterns", 1, 0, d), f"{d} directions")
    nothing = ops.measure_class_regions(torch.zeros((2, 9, 9), dtype=torch.uint8, device=DEV), 4)
    assert nothing.shape == (0, len(ops.SHAPE_FIELDS)) and nothing.dtype == np.int64
    assert ops.measure_class_regions(torch.zeros((1, 4, 4), dtype=torch.int64, device=DEV), 4, directions=4).shape == (0, 19)


def test_describe_and_measure_label_once_and_agree_with_the_two_calls():
    maps, C = _case("patterns")
    conf = torch.rand(maps.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    rec, shapes = ops.describe_and_measure_class_regions(_dev(maps), C, conf, 2, 3, 16)
    assert rec.tobytes() == ops.describe_class_regions(_dev(maps), C, conf, 2, 3).tobytes()
    _assert_equal(shapes, _want("patterns", 2, 3, 16), "both on one labelling")
    empty = ops.describe_and_measure_class_regions(torch.zeros((1, 5, 5), dtype=torch.uint8, device=DEV), C)
    assert empty[0].shape == (0, 12) and empty[1].shape == (0, len(ops.SHAPE_FIELDS))


MARGIN = 256    # bytes of sentinel on each side of every buffer
SENTINEL = 0xA5


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + MARGIN


def test_direct_call_with_an_exactly_sized_workspace():
    maps, C = _case("random")
    n, h, w = maps.shape
    want = _want("random")
    F, cap = want.shape[1], len(want)
    region, sizes, _ = ops.label_class_regions(_dev(maps), C)
    lib, vp = L.lib(), ctypes.c_void_p
    need = lib.unet_measure_class_regions_workspace(n, h, w, 32)
    assert need == (n * h * w * 4 + 15) // 16 * 16
    table = defects.direction_table(32)
    bufs = {k: _guarded(b) for k, b in (("records", cap * F * 8), ("count", 8), ("ws", need))}
    bufs["count"][0][MARGIN:-MARGIN] = 0
    L.check(lib.unet_measure_class_regions(vp(region.data_ptr()), vp(sizes.data_ptr()), n, h, w, 1, 0,
                                           vp(table.ctypes.data), 32, vp(bufs["records"][1]), cap, vp(bufs["count"][1]),
                                           vp(bufs["ws"][1]), need, None), "unet_measure_class_regions")
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():                   # the guard behind (and before) every buffer is untouched
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all()), k
    assert bufs["count"][0][MARGIN:-MARGIN].view(torch.int64).tolist() == [cap]
    got = bufs["records"][0][MARGIN:-MARGIN].view(torch.int64).cpu().numpy().reshape(cap, F)
    got = np.ascontiguousarray(got[np.lexsort((got[:, 1], got[:, 0]))])
    assert got.tobytes() == _got("random").tobytes()
    _assert_equal(got, want, "direct call")


def test_refused_shapes_raise_before_any_launch():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    for d in (1, 3, 34, 0, -2):
        with pytest.raises(RuntimeError, match="2..32 directions"):
            ops.measure_class_regions(x, 4, directions=d)
    with pytest.raises(RuntimeError, match="sides up to 16384"):      # a view, no memory behind it
        ops.measure_class_regions(x[:1, :1, :1].expand(1, 2, 16385), 4)
    with pytest.raises(RuntimeError, match="2..255 classes"):
        ops.measure_class_regions(x, 1)
    with pytest.raises(ValueError, match="min_pixels"):
        ops.measure_class_regions(x, 4, min_pixels=0)
    with pytest.raises(ValueError, match="image_base"):
        ops.measure_class_regions(x, 4, image_base=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.measure_class_regions(x.cpu(), 4)


# ------------------------------------------------------------------------------------------------ CLI
@functools.lru_cache(maxsize=None)
def _tree(tmp):
    """(image directory, sorted paths, checkpoint) of a synthetic Gear tree and a randomly initialised model"""
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd import gear_dataset as G
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    root = G.write_synthetic_gear(os.path.join(tmp, "gear"))
    source = os.path.join(root, "images", "test")
    paths = sorted(os.path.join(source, f) for f in os.listdir(source))
    ckpt = os.path.join(tmp, "model.pth")
    torch.manual_seed(1)
    model = SegmentationUNet(3, 4, precision="fp32").to(DEV)
    save_checkpoint(model, get_optimizer(model), 0, 0.0, ckpt)
    return source, paths, ckpt


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _tree(str(tmp_path_factory.mktemp("shapes")))


NAMES = ["background", "pitting", "spalling", "scrape"]
DEFECT_KEYS = {"class", "class_name", "pixels", "bbox", "bbox_original", "centroid", "centroid_original",
               "mean_confidence", "peak_confidence", "counted"}


def _predict(tree, out, *extra):
    source, _paths, ckpt = tree
    predict.main(["--task", "gear", "--checkpoint", ckpt, "--input", source, "--image_size", "64", "64", "--batch_size", "3",
                  "--num_workers", "0", "--mask_size", "frame", "--output_dir", str(out), *extra])
    return json.load(open(os.path.join(out, "predictions.json")))


def test_predict_without_the_flags_writes_what_it_wrote_before(tree, tmp_path):
    _source, paths, _ckpt = tree
    res = _predict(tree, tmp_path / "plain")
    assert set(res) == {"args", "class_names", "frame_size", "images", "summary"}
    assert set(res["args"]) == {name[2:] for name, _ in predict.FLAGS}
    total = 0
    for k, e in enumerate(res["images"]):
        assert set(e) == {"image_path", "name", "original_size", "mean_confidence", "defect_pixels", "defects", "decision"}
        # the entry of the code path that was there before: the mask's records through defect_entries alone
        mask = np.array(Image.open(tmp_path / "plain" / "masks" / (e["name"] + ".png")))
        want = D.describe_records(mask[None], 4)
        assert [set(d) for d in e["defects"]] == [DEFECT_KEYS] * len(want)
        (entry,) = defects.defect_entries(want, NAMES, (64, 64), [tuple(e["original_size"])])
        for d, p in zip(e["defects"], entry["defects"]):
            assert {key: d[key] for key in ("class", "pixels", "bbox", "bbox_original", "centroid", "centroid_original")} \
                == {key: p[key] for key in ("class", "pixels", "bbox", "bbox_original", "centroid", "centroid_original")}
        assert e["decision"] == ("reject" if len(want) else "accept")
        total += len(want)
    assert total > 0                                   # a random head predicts something


def test_predict_measure_shapes_writes_a_shape_per_defect(tree, tmp_path, capsys):
    plain = _predict(tree, tmp_path / "plain")
    capsys.readouterr()
    res = _predict(tree, tmp_path / "shaped", "--measure_shapes", "--pixel_size", "0.05")
    assert " length " in capsys.readouterr().out
    assert set(res) == {"args", "class_names", "frame_size", "size_rules", "images", "summary"}
    assert res["size_rules"] == defects.size_rules(0.05, 0.0, 0.0)
    assert res["args"]["measure_shapes"] is True and res["args"]["pixel_size"] == 0.05
    for e, before in zip(res["images"], plain["images"]):
        mask = np.array(Image.open(tmp_path / "shaped" / "masks" / (e["name"] + ".png")))
        rec, shp = D.describe_records(mask[None], 4), S.shape_records(mask[None], 4)
        assert len(e["defects"]) == len(rec) == len(before["defects"])
        for d, b, r, s in zip(e["defects"], before["defects"], rec, shp):
            assert set(d) == DEFECT_KEYS | {"shape"} and {k: v for k, v in d.items() if k != "shape"} == b
            assert d["shape"]["area"] == d["pixels"]
            want = defects.shape_measures(s, 32, (64, 64), e["original_size"], 0.05, defect_record=r)
            assert d["shape"] == want                  # the device's integers through the same host geometry
            assert d["shape"]["feret_length_mm"] == d["shape"]["feret_length"] * 0.05
        assert e["decision"] == before["decision"]


def test_predict_tiled_with_a_huge_minimum_length_accepts_everything(tmp_path):
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    source = tmp_path / "photos"
    os.makedirs(source)
    rng = np.random.default_rng(11)
    for k, (h0, w0) in enumerate([(40, 56), (33, 70)]):
        Image.fromarray(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)).save(source / f"part_{k}.png")
    torch.manual_seed(1)
    model = SegmentationUNet(3, 4, precision="fp32").to(DEV)
    ckpt = tmp_path / "model.pth"
    save_checkpoint(model, get_optimizer(model), 0, 0.0, str(ckpt))
    argv = ["--task", "gear", "--checkpoint", str(ckpt), "--input", str(source), "--tile", "32", "32", "--min_overlap", "8",
            "--batch_size", "4", "--num_workers", "0"]
    predict_tiled.main(argv + ["--output_dir", str(tmp_path / "plain")])
    predict_tiled.main(argv + ["--output_dir", str(tmp_path / "ruled"), "--min_defect_length", "1e9"])
    plain = json.load(open(tmp_path / "plain" / "predictions.json"))
    ruled = json.load(open(tmp_path / "ruled" / "predictions.json"))
    assert "size_rules" not in plain and not any("shape" in d for e in plain["images"] for d in e["defects"])
    assert ruled["size_rules"] == defects.size_rules(None, 1e9, 0.0) and ruled["args"]["measure_shapes"] is True
    assert sum(len(e["defects"]) for e in plain["images"]) > 0 and any(e["decision"] == "reject" for e in plain["images"])
    for e, before in zip(ruled["images"], plain["images"]):
        assert e["decision"] == "accept"
        assert len(e["defects"]) == len(before["defects"])                 # listed all the same
        for d, b in zip(e["defects"], before["defects"]):
            assert d["counted"] is False and d["shape"]["area"] == d["pixels"] == b["pixels"] and d["bbox"] == b["bbox"]
            assert d["shape"]["perimeter_original"] is not None            # scale 1: the frame is the image
