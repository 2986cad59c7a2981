"""CPU checks of the tiled prediction: the tile plan of tests/_tiles_ref.py and tiling.plan_axis over every small axis,
the reference blend on hand cases, the exports and host-side refusals of unet_tile_gather / unet_tile_blend, and the
predict_tiled CLI's flags and refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _tiles_ref as T
from tiaozhanbei_unet_amd import _lib, ops, predict, predict_tiled, tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("unet_tile_gather", "unet_tile_blend")


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_covers_overlaps_and_is_minimal_on_every_small_axis():
    """every frame <= 80, tile <= 40, min_overlap < min(tile, frame): the origins cover [0, frame), neighbours overlap by
    at least min_overlap, no smaller count of tiles could, and tiling.plan_axis gives the same origins"""
    checked = refused = 0
    for frame in range(1, 81):
        for tile in range(1, 41):
            length = min(tile, frame)
            for mo in range(length):
                if length + 63 * (length - mo) < frame:                # 64 tiles do not reach: both refuse
                    for plan in (T.plan_axis, tiling.plan_axis):
                        with pytest.raises(ValueError):
                            plan(frame, tile, mo)
                    refused += 1
                    continue
                o = T.plan_axis(frame, tile, mo)
                assert tiling.plan_axis(frame, tile, mo) == o, (frame, tile, mo)
                n = len(o)
                assert o[0] == 0 and o[-1] == frame - length and n <= 64
                assert all(b > a for a, b in zip(o, o[1:]))
                assert all(a + length - b >= mo for a, b in zip(o, o[1:])), (frame, tile, mo, o)
                # n - 1 tiles overlapping by mo reach length + (n - 2) (length - mo) pixels at the most: not the frame
                assert n == 1 or length + (n - 2) * (length - mo) < frame, (frame, tile, mo, o)
                assert (n == 1) == (frame <= tile)
                checked += 1
    assert checked > 50000 and 0 < refused < 200


def test_plan_refusals_and_plan_tiles():
    for frame, tile, mo in ((10, 4, 4), (10, 4, -1), (3, 8, 3), (0, 4, 0), (10, 0, 0)):
        with pytest.raises(ValueError):
            tiling.plan_axis(frame, tile, mo)
    with pytest.raises(ValueError, match="at most 64"):
        tiling.plan_axis(1000, 8, 0)                    # 125 tiles
    assert len(tiling.plan_axis(512, 8, 0)) == 64
    assert tiling.plan_axis(1080, 512, 64) == [0, 284, 568] and tiling.plan_axis(1920, 512, 64) == [0, 352, 704, 1056, 1408]
    assert tiling.plan_tiles((1080, 1920), (512, 512), 64) == (512, 512, [0, 284, 568], [0, 352, 704, 1056, 1408])
    assert tiling.plan_tiles((36, 52), (512, 512), 16) == (36, 52, [0], [0])
    assert tiling.plan_tiles((7, 9), (4, 5), 1) == (4, 5, [0, 3], [0, 4])
    assert tiling.default_ramp([0, 284, 568], 512) == 228 and tiling.default_ramp([0], 512) == 1
    assert tiling.default_ramp([0, 100], 512) == 256 and tiling.default_ramp([0, 8], 8) == 1       # clipped both ways
    for o, length in (([0, 284, 568], 512), ([0], 9), ([0, 100], 512), ([0, 8], 8), ([0, 3, 7], 5)):
        assert tiling.default_ramp(o, length) == T.default_ramp(o, length)


# ------------------------------------------------------------------------------------------------ the reference blend
def _line(values):
    """1-D tiles [T, C, 1, L] of two classes: class 0 holds the values, class 1 their negation"""
    v = np.asarray(values, np.float32)[:, None, None, :]
    return np.concatenate([v, -v], axis=1)


def test_reference_blend_two_tiles_in_one_dimension():
    """frame 1 x 7, tiles of 5 at 0 and 2, overlap 3 (x = 2, 3, 4)"""
    a, b = [1.0, 2.0, 3.0, 4.0, 5.0], [10.0, 20.0, 30.0, 40.0, 50.0]
    tiles = _line([a, b])
    assert T.weights(5, 3).tolist() == [1, 2, 3, 2, 1] and T.weights(5, 1).tolist() == [1] * 5
    assert T.weights(5, 256).tolist() == [1, 2, 3, 2, 1] and T.weights(6, 2).tolist() == [1, 2, 2, 2, 2, 1]
    mixed, wsum, covers = T.blend(tiles, [0], [0, 2], (1, 7), 1, 3)
    assert covers[0].tolist() == [1, 1, 2, 2, 2, 1, 1]
    assert wsum[0].tolist() == [1, 2, 3 + 1, 2 + 2, 1 + 3, 2, 1]
    f = np.float32
    want = [f(1), f(2), (f(3) * f(3) + f(1) * f(10)) / f(4), (f(2) * f(4) + f(2) * f(20)) / f(4),
            (f(1) * f(5) + f(3) * f(30)) / f(4), f(40), f(50)]
    assert mixed[0, 0].tolist() == [float(v) for v in want] == [1.0, 2.0, 4.75, 12.0, 23.75, 40.0, 50.0]
    assert mixed[1, 0].tolist() == [-float(v) for v in want]
    # ramp 1: a plain mean where two tiles meet
    flat, wsum1, _ = T.blend(tiles, [0], [0, 2], (1, 7), 1, 1)
    assert wsum1[0].tolist() == [1, 1, 2, 2, 2, 1, 1] and flat[0, 0].tolist() == [1.0, 2.0, 6.5, 12.0, 17.5, 40.0, 50.0]
    # the same along y
    up, _, _ = T.blend(tiles.transpose(0, 1, 3, 2), [0, 2], [0], (7, 1), 3, 1)
    assert np.array_equal(up[:, :, 0], mixed[:, 0])


def test_reference_copies_single_cover_pixels_and_rounds_each_operation_once():
    rng = np.random.default_rng(3)
    tiles = rng.standard_normal((4, 3, 4, 5)).astype(np.float32)
    oy, ox = [0, 3], [0, 4]                            # frame 7 x 9: rows 3 and columns 4 are shared
    mixed, wsum, covers = T.blend(tiles, oy, ox, (7, 9), 1, 1)
    assert covers[3, 4] == 4 and covers[3, 0] == 2 and covers[0, 4] == 2 and covers[0, 0] == 1
    assert int((covers == 1).sum()) == 6 * 8 and int((covers == 2).sum()) == 6 + 8
    # every single-cover pixel carries its tile's bits: a weight that is not 1 must not touch it (ramp 3 weighs them 1..3)
    ramped, _, _ = T.blend(tiles, oy, ox, (7, 9), 3, 3)
    single = covers == 1
    assert np.array_equal(ramped[:, single].view(np.uint32), mixed[:, single].view(np.uint32))
    assert np.array_equal(mixed[:, :3, :4], tiles[0, :, :3, :4]) and np.array_equal(mixed[:, 4:, 5:], tiles[3, :, 1:, 1:])
    # the corner pixel under four tiles, ascending i then j, each step one fp32 rounding
    z = [tiles[0, :, 3, 4], tiles[1, :, 3, 0], tiles[2, :, 0, 4], tiles[3, :, 0, 0]]
    acc = np.zeros(3, np.float32)
    for v in z:
        acc = (acc + (np.float32(1.0) * v).astype(np.float32)).astype(np.float32)
    assert np.array_equal(mixed[:, 3, 4], (acc / np.float32(4.0)).astype(np.float32))
    labels, conf, again = T.predict(tiles, oy, ox, (7, 9), 1, 1)
    assert np.array_equal(again, mixed) and labels.dtype == np.uint8 and conf.dtype == np.float32
    assert np.array_equal(labels, np.argmax(mixed, axis=0)) and float(conf.min()) >= 1 / 3 - 1e-6
    # gather is slicing, and blending a gathered frame gives the frame back wherever one tile covers
    frame = rng.standard_normal((3, 7, 9)).astype(np.float32)
    g = T.gather(frame, 4, 5, oy, ox)
    assert g.shape == (4, 3, 4, 5) and np.array_equal(g[3], frame[:, 3:, 4:])
    back, _, _ = T.blend(g, oy, ox, (7, 9), 1, 1)
    assert np.array_equal(back[:, single], frame[:, single])


# ------------------------------------------------------------------------------------------------ exports
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "tiaozhanbei_unet_amd", "csrc", "Makefile")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert handle.unet_abi_version() == 1
    assert " tiles.hip" in makefile
    for obj in ("build/tiles.o", "build/stamps/tiles.o"):      # what make would run, for the default and the diagnostic build
        line = subprocess.run(["make", "-C", _lib.CSRC, "-n", "-B", obj], capture_output=True, text=True, check=True).stdout
        assert re.search(rf" -ffp-contract=off .*-c tiles\.hip -o {obj}\n", line), line
    for name in ("plan_axis", "plan_tiles", "gather_tiles", "blend_tiles", "TiledPredictor"):
        assert hasattr(tiling, name) and not hasattr(ops, name), name


def _ints(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_refusals_are_decided_on_the_host():
    """dummy device pointers: every call below is refused before anything could read them"""
    lib = _lib.lib()
    dummy = ctypes.c_void_p(16)
    zero = _ints([0])
    oy, ox = _ints([0, 3]), _ints([0, 4])              # the cover of 7 x 9 by 4 x 5

    def blend(c=3, th=4, tw=5, oy=oy, ny=2, ox=ox, nx=2, h=7, w=9, ry=1, rx=1, tiles=dummy, labels=dummy, conf=dummy):
        return lib.unet_tile_blend(tiles, c, th, tw, oy, ny, ox, nx, h, w, ry, rx, labels, conf, None, None)

    def gather(c=3, h=7, w=9, th=4, tw=5, oy=oy, ny=2, ox=ox, nx=2, frame=dummy, tiles=dummy):
        return lib.unet_tile_gather(frame, c, h, w, th, tw, oy, ny, ox, nx, tiles, None)

    for c in (1, 9, 0, -2):
        assert blend(c=c) == -2 and b"2..8 classes" in lib.unet_last_error()
    assert gather(c=0) == -2 and b"at least 1 channel" in lib.unet_last_error()
    for ry, rx in ((0, 1), (1, 0), (257, 1), (1, 257), (-1, 1)):
        assert blend(ry=ry, rx=rx) == -2 and b"1..256" in lib.unet_last_error()
    many = _ints(list(range(65)))
    for call in (blend, gather):
        for kw in (dict(ny=0), dict(nx=0), dict(ny=65, oy=many, h=68), dict(nx=65, ox=many, w=69), dict(ny=-1)):
            assert call(**kw) == -2 and b"1..64 per axis" in lib.unet_last_error(), kw
        for kw in (dict(th=0), dict(tw=0), dict(th=8), dict(tw=10), dict(h=0), dict(w=-9), dict(th=-1)):
            assert call(**kw) == -2 and b"1 <= tile <= frame" in lib.unet_last_error(), kw
        big = dict(h=1 << 16, w=1 << 15, oy=_ints([0, (1 << 16) - 4]), ox=_ints([0, (1 << 15) - 5]))
        assert call(**big) == -2 and b"2^31 - 1" in lib.unet_last_error()
        # null pointers
        assert call(tiles=None) == -1 and b"null pointer" in lib.unet_last_error()
        assert call(oy=None) == -1 and call(ox=None) == -1
        # tables that are no cover: a first origin past 0, a last one short of or past frame - tile, a repeat, a
        # descent, a gap wider than the tile
        for bad in ([1, 3], [0, 2], [0, 4], [0, 0], [3, 0]):
            assert call(oy=_ints(bad)) == -1 and b"not a cover" in lib.unet_last_error(), bad
        assert call(ox=_ints([0, 3])) == -1 and call(ox=_ints([0, 5])) == -1
        assert call(h=13, th=5, oy=_ints([0, 4, 3, 8]), ny=4) == -1          # only the descent is wrong with it
        assert call(h=13, th=5, oy=_ints([0, 4, 4, 8]), ny=4) == -1          # only the repeat
        assert call(h=13, oy=_ints([0, 9]), ny=2) == -1 and b"not a cover" in lib.unet_last_error()      # a gap of 9 > 4
        assert call(oy=zero, ny=1) == -1                # one tile of 4 does not cover 7 rows
    assert gather(frame=None) == -1
    assert blend(labels=None, conf=None) == -1 and b"null pointer" in lib.unet_last_error()
    # the 2^31 - 1 pixel frame itself is inside the limit: it gets as far as the tables
    assert blend(h=1, w=(1 << 31) - 1, th=1, oy=zero, ny=1, ox=_ints([0, 7])) == -1
    assert b"not a cover" in lib.unet_last_error()


def test_wrappers_check_shapes_and_dtypes_before_the_device():
    torch = pytest.importorskip("torch")
    z = torch.zeros((4, 3, 4, 5))
    for bad in (z[0], z.double(), "tiles"):
        with pytest.raises(ValueError, match="float32"):
            tiling.blend_tiles(bad, [0, 3], [0, 4], (7, 9))
    with pytest.raises(ValueError, match="4 tiles"):
        tiling.blend_tiles(z, [0, 3], [0], (7, 9))
    with pytest.raises(ValueError, match="origins"):
        tiling.blend_tiles(z, [], [0, 4], (7, 9))
    with pytest.raises(ValueError, match="frame of 3 x 9"):
        tiling.blend_tiles(z, [0, 3], [0, 4], (3, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tiling.blend_tiles(z, [0, 3], [0, 4], (7, 9))
    f = torch.zeros((3, 7, 9))
    for bad in (f[0], f.half(), None):
        with pytest.raises(ValueError, match="float32"):
            tiling.gather_tiles(bad, 4, 5, [0, 3], [0, 4])
    with pytest.raises(ValueError, match="origins"):
        tiling.gather_tiles(f, 4, 5, list(range(65)), [0, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tiling.gather_tiles(f, 4, 5, [0, 3], [0, 4])
    for kw in (dict(tile_hw=(0, 8)), dict(tile_hw=(8, 8), min_overlap=8), dict(tile_hw=(8, 8), batch_size=0)):
        with pytest.raises(ValueError):
            tiling.TiledPredictor(None, **kw)


# ------------------------------------------------------------------------------------------------ CLI flags
BASE = ["--task", "gear", "--checkpoint", "c.pth", "--input", "photos"]


def test_predict_tiled_flags():
    gear = vars(predict_tiled.parse_args(BASE))
    shared = {name[2:] for name, _ in predict.FLAGS} - {"image_size", "mask_size"}
    assert set(gear) == shared | {"tile", "min_overlap", "scale"} == {name[2:] for name, _ in predict_tiled.FLAGS}
    assert "image_size" not in gear and "mask_size" not in gear
    assert (gear["tile"], gear["min_overlap"], gear["scale"]) == ([512, 512], 64, 1.0)
    ref = vars(predict.parse_args(BASE))
    assert all(gear[k] == ref[k] for k in shared)      # predict's defaults
    assert (gear["output_dir"], gear["model"], gear["precision"], gear["batch_size"], gear["num_workers"],
            gear["device"]) == ("predictions", "seg_unet", "fp32", 8, 4, "auto")
    kol = vars(predict_tiled.parse_args(["--task", "kolektorsdd", "--checkpoint", "c.pth", "--input", "p.jpg"]))
    assert kol["tile"] == [1024, 512]
    own = vars(predict_tiled.parse_args(BASE + ["--tile", "64", "32", "--min_overlap", "31", "--scale", "0.25",
                                                "--save_overlays", "--batch_size", "3"]))
    assert (own["tile"], own["min_overlap"], own["scale"], own["save_overlays"], own["batch_size"]) == (
        [64, 32], 31, 0.25, True, 3)
    assert vars(predict_tiled.parse_args(BASE + ["--scale", "4"]))["scale"] == 4.0
    assert vars(predict_tiled.parse_args(BASE + ["--min_overlap", "0"]))["min_overlap"] == 0


@pytest.mark.parametrize("extra", [["--scale", "0"], ["--scale", "-1"], ["--scale", "4.5"], ["--min_overlap", "512"],
                                   ["--min_overlap", "600"], ["--tile", "64", "32", "--min_overlap", "32"],
                                   ["--min_overlap", "-1"], ["--tile", "0", "64"], ["--tile", "64"],
                                   ["--image_size", "64", "64"], ["--mask_size", "frame"], ["--batch_size", "0"],
                                   ["--min_region_pixels", "0"], ["--min_confidence", "2"]])
def test_predict_tiled_refuses(extra):
    with pytest.raises(SystemExit):
        predict_tiled.parse_args(BASE + extra)


@pytest.mark.parametrize("task", ["gear", "kolektorsdd"])
def test_predict_tiled_refuses_cpu(task):
    with pytest.raises(SystemExit) as e:
        predict_tiled.main(["--task", task, "--device", "cpu", "--checkpoint", "ckpt.pth", "--input", "photos"])
    assert "no CPU path" in str(e.value)


def test_working_frame():
    assert predict_tiled.working_frame((1080, 1920), 1.0) == (1080, 1920)
    assert predict_tiled.working_frame((1080, 1920), 0.5) == (540, 960)
    assert predict_tiled.working_frame((501, 1243), 0.3) == (150, 373)
    assert predict_tiled.working_frame((1, 3), 0.1) == (1, 1)
