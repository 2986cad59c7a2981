"""GPU tests of the tiled prediction (csrc/tiles.hip through tiling.gather_tiles / blend_tiles / TiledPredictor and the
predict_tiled CLI) against tests/_tiles_ref.py, which test_cpu_tiles.py pins: the gathered tiles and the blended logits
bit for bit, the labels byte for byte, the confidence within _segvis_ref.conf_bound of the float64 confidence of the
blended fp32 logits (the scheme of test_gpu_segvis.py).  The plans are the smallest that reach every path: one-pixel and
four-pixel lanes, the one-pixel fallback on an aligned frame, one tile along an axis, 64 origins along an axis.

Strictly increasing origins 0 .. 63 need frame - tile >= 63, so a 48-pixel axis cannot carry 64 of them: the 64-origin
plans put them on an axis of 72 (tile 9) and of 79 (tile 16) beside a 48-pixel axis."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import _ref64 as R64
import _segvis_ref as S
import _tiles_ref as T
from tiaozhanbei_unet_amd import defects, ops, predict_tiled, tiling
from tiaozhanbei_unet_amd.evaluation import describe_class_regions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24

# name -> (frame (h, w), tile (th, tw), oy, ox, takes the 16-byte path)
PLANS = {
    "7x9-scalar": ((7, 9), (4, 5), T.plan_axis(7, 4, 1), T.plan_axis(9, 5, 1), False),
    "40x32-vector": ((40, 32), (16, 16), T.plan_axis(40, 16, 12), T.plan_axis(32, 16, 12), True),
    "40x32-odd-ox": ((40, 32), (16, 16), T.plan_axis(40, 16, 12), [0, 3, 9, 13, 16], False),
    "33x64-one-row-of-tiles": ((33, 64), (33, 16), [0], T.plan_axis(64, 16, 4), True),
    "72x48-64-origins-y": ((72, 48), (9, 16), list(range(64)), [0, 16, 32], True),
    "48x79-64-origins-x": ((48, 79), (16, 16), T.plan_axis(48, 16, 0), list(range(64)), False),
}


def test_the_plans_are_what_their_names_say():
    assert PLANS["7x9-scalar"][2:4] == ([0, 3], [0, 4])
    assert PLANS["40x32-vector"][2:4] == ([0, 4, 8, 12, 16, 20, 24], [0, 4, 8, 12, 16])
    assert PLANS["33x64-one-row-of-tiles"][3] == [0, 12, 24, 36, 48]
    assert PLANS["48x79-64-origins-x"][2] == [0, 16, 32]
    for (h, w), (th, tw), oy, ox, vec in PLANS.values():
        assert oy[0] == 0 and oy[-1] == h - th and ox[0] == 0 and ox[-1] == w - tw
        assert vec == (w % 4 == 0 and tw % 4 == 0 and all(x % 4 == 0 for x in ox))


@functools.lru_cache(maxsize=None)
def _tied(name):
    (h, w) = PLANS[name][0]
    return np.random.default_rng(h * w).random((h, w)) < 0.5


@functools.lru_cache(maxsize=None)
def _tile_logits(name, c):
    """random fp32 tile logits N(0, 4^2); on half the pixels of the FRAME classes 0 and c - 1 tie, exactly, above the
    rest in every tile over the pixel (the blend treats both alike and keeps order: they tie on top in the blended
    logits too).  Built once, read-only."""
    (h, w), (th, tw), oy, ox, _ = PLANS[name]
    rng = np.random.default_rng(100 * c + h + w)
    z = (rng.standard_normal((len(oy) * len(ox), c, th, tw)) * 4.0).astype(np.float32)
    top = (z.max(axis=1) + np.float32(1.0)).astype(np.float32)
    where = T.gather(_tied(name)[None], th, tw, oy, ox)[:, 0]
    z[:, 0] = np.where(where, top, z[:, 0])
    z[:, c - 1] = np.where(where, top, z[:, c - 1])
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _want(name, c, ramp):
    (h, w), (th, tw), oy, ox, _ = PLANS[name]
    ry, rx = (T.default_ramp(oy, th), T.default_ramp(ox, tw)) if ramp is None else (ramp, ramp)
    labels, _, mixed = T.predict(_tile_logits(name, c), oy, ox, (h, w), ry, rx)
    for a in (labels, mixed):
        a.setflags(write=False)
    return labels, mixed


def _check_conf(out, z, what):
    """out against the float64 confidence of the fp32 logits z [N, C, ...]: allowed = max(4 x host error, 2^-22) [expf,
    measured on the host's fp32 evaluation of the same formula] + the derived terms of S.conf_bound"""
    c = z.shape[1]
    ref = torch.from_numpy(S.conf64(z))
    host = torch.from_numpy(S.conf32(z))
    derived = c * np.exp(-1.0) * U + (c - 1) * U + U
    worst = R64.assert_measured(out, (ref, ref), host, what, extra=derived)
    host_rel, kernel_rel, allowed = R64.MEASURED[what]
    total, _ = S.conf_bound(c, host_rel)
    assert abs(total - allowed) <= 1e-12 * allowed
    return worst, host_rel, kernel_rel, allowed


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("h, w, th, tw, mo", [(7, 9, 4, 5, 1), (40, 33, 16, 16, 4), (40, 32, 16, 16, 12), (12, 20, 12, 20, 0)],
                         ids=["7x9", "40x33", "40x32-vector", "single-tile"])
def test_gather_equals_slicing(h, w, th, tw, mo):
    rng = np.random.default_rng(h * w)
    frame = rng.standard_normal((3, h, w)).astype(np.float32)
    frame[0, 0, 0], frame[1, -1, -1], frame[2, 0, -1] = np.nan, -0.0, np.inf        # a copy keeps every bit
    oy, ox = T.plan_axis(h, th, mo), T.plan_axis(w, tw, mo)
    got = tiling.gather_tiles(torch.from_numpy(frame).to(DEV), th, tw, oy, ox)
    want = T.gather(frame, th, tw, oy, ox)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (len(oy) * len(ox), 3, th, tw)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    if len(oy) * len(ox) == 1:
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), frame.view(np.uint32))


# ------------------------------------------------------------------------------------------------ blend
@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("name", list(PLANS))
def test_blend_against_the_restatement(name, c):
    (h, w), (th, tw), oy, ox, _ = PLANS[name]
    zd = torch.from_numpy(np.array(_tile_logits(name, c))).to(DEV)
    for ramp in (1, None, 256):
        want_labels, want_mixed = _want(name, c, ramp)
        labels, conf, mixed = tiling.blend_tiles(zd, oy, ox, (h, w), ramp=ramp, blended=True)
        assert (labels.dtype, conf.dtype, mixed.dtype) == (torch.uint8, torch.float32, torch.float32)
        assert tuple(labels.shape) == (h, w) == tuple(conf.shape) and tuple(mixed.shape) == (c, h, w)
        got = mixed.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want_mixed.view(np.uint32)), (name, c, ramp)
        assert np.array_equal(labels.cpu().numpy(), want_labels), (name, c, ramp)
        what = f"tileconf {name} c{c} ramp {ramp}"
        worst, host_rel, kernel_rel, allowed = _check_conf(conf[None], got[None], what)
        print(f"REF64 {what}: host err {host_rel / U:.2f} u, kernel err {kernel_rel / U:.2f} u, allowed {allowed / U:.2f} u, "
              f"worst err / bound {worst:.3f}")
        # without the blended logits the other two outputs are the same bytes
        only = tiling.blend_tiles(zd, oy, ox, (h, w), ramp=ramp)
        assert len(only) == 2 and torch.equal(only[0], labels) and torch.equal(only[1], conf)
    # the planted ties are there, and the first maximum took them
    tied = _tied(name)
    assert 0.3 < tied.mean() < 0.7 and (want_mixed[0] == want_mixed[c - 1])[tied].all()
    assert (want_mixed[0] == want_mixed.max(axis=0))[tied].all() and (want_labels[tied] == 0).all()
    if name == "40x32-vector":                         # the ramps weigh its wide overlaps differently
        assert not np.array_equal(_want(name, c, 1)[1], _want(name, c, 256)[1])


def test_a_single_tile_over_the_frame_is_seg_confidence():
    for h, w in ((33, 65), (16, 20)):                  # one-pixel and four-pixel lanes
        z = torch.from_numpy((np.random.default_rng(h).standard_normal((1, 4, h, w)) * 4.0).astype(np.float32)).to(DEV)
        z[0, 1, 0, :5] = z[0, 3, 0, :5] = 9.0            # ties
        want_labels, want_conf = ops.seg_confidence(z)
        for ramp in (None, 7):
            labels, conf, mixed = tiling.blend_tiles(z, [0], [0], (h, w), ramp=ramp, blended=True)
            assert torch.equal(labels, want_labels[0]) and torch.equal(conf, want_conf[0]) and torch.equal(mixed, z[0])


def test_unaligned_buffers_take_the_one_pixel_path_to_the_same_bytes():
    name, c = "40x32-vector", 3
    (h, w), _, oy, ox, _ = PLANS[name]
    z = _tile_logits(name, c)
    shifted = torch.empty(z.size + 1, device=DEV)[1:].view(z.shape)       # 4 bytes past a 16-byte boundary
    shifted.copy_(torch.from_numpy(np.array(z)))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    labels, conf, mixed = tiling.blend_tiles(shifted, oy, ox, (h, w), blended=True)
    want_labels, want_mixed = _want(name, c, None)
    assert np.array_equal(mixed.cpu().numpy().view(np.uint32), want_mixed.view(np.uint32))
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    aligned = tiling.blend_tiles(shifted.clone(), oy, ox, (h, w))
    assert torch.equal(aligned[0], labels) and torch.equal(aligned[1], conf)
    frame = torch.empty(3 * h * w + 1, device=DEV).normal_()[1:].view(3, h, w)
    tiles = tiling.gather_tiles(frame, 16, 16, oy, ox)
    assert np.array_equal(tiles.cpu().numpy(), T.gather(frame.cpu().numpy(), 16, 16, oy, ox))


def test_non_default_stream():
    name, c = "40x32-vector", 3
    (h, w), (th, tw), oy, ox, _ = PLANS[name]
    frame = torch.from_numpy(np.random.default_rng(5).standard_normal((3, h, w)).astype(np.float32)).to(DEV)
    zd = torch.from_numpy(np.array(_tile_logits(name, c))).to(DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        tiles = tiling.gather_tiles(frame, th, tw, oy, ox)
        labels, conf, mixed = tiling.blend_tiles(zd, oy, ox, (h, w), blended=True)
    stream.synchronize()
    assert np.array_equal(tiles.cpu().numpy(), T.gather(frame.cpu().numpy(), th, tw, oy, ox))
    want_labels, want_mixed = _want(name, c, None)
    assert np.array_equal(mixed.cpu().numpy().view(np.uint32), want_mixed.view(np.uint32))
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    _check_conf(conf[None], want_mixed[None], "tileconf on a side stream")


def test_refusals_raise_before_any_launch():
    z = torch.zeros((4, 3, 4, 5), device=DEV)
    with pytest.raises(RuntimeError, match="not a cover"):
        tiling.blend_tiles(z, [0, 2], [0, 4], (7, 9))
    with pytest.raises(RuntimeError, match="1..256"):
        tiling.blend_tiles(z, [0, 3], [0, 4], (7, 9), ramp=0)
    with pytest.raises(RuntimeError, match="2..8 classes"):
        tiling.blend_tiles(torch.zeros((4, 9, 4, 5), device=DEV), [0, 3], [0, 4], (7, 9))
    with pytest.raises(RuntimeError, match="not a cover"):
        tiling.gather_tiles(torch.zeros((3, 7, 9), device=DEV), 4, 5, [0, 3], [1, 4])


# ------------------------------------------------------------------------------------------------ the predictor
@functools.lru_cache(maxsize=None)
def _model():
    from tiaozhanbei_unet_amd import SegmentationUNet
    torch.manual_seed(1)
    return SegmentationUNet(3, 4, precision="fp32").to(DEV).eval()


def _frame(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((3, h, w)).astype(np.float32)).to(DEV)


def test_predictor_with_a_tile_at_least_the_frame_is_the_model():
    model, x = _model(), _frame(36, 52, 2)
    labels, conf, plan = tiling.TiledPredictor(model, (64, 64), min_overlap=16, batch_size=2)(x)
    assert plan == {"tile": [36, 52], "origins_y": [0], "origins_x": [0], "ramp": [1, 1]}
    with torch.no_grad():
        want_labels, want_conf = ops.seg_confidence(model(x[None]))
    assert torch.equal(labels, want_labels[0]) and torch.equal(conf, want_conf[0])


def test_predictor_blends_the_models_own_tile_logits():
    model, x = _model(), _frame(48, 80, 3)
    predictor = tiling.TiledPredictor(model, (32, 32), min_overlap=8, batch_size=4)      # 6 tiles: chunks of 4 and 2
    labels, conf, plan = predictor(x)
    assert plan == {"tile": [32, 32], "origins_y": [0, 16], "origins_x": [0, 24, 48], "ramp": [16, 8]}
    tiles = tiling.gather_tiles(x, 32, 32, plan["origins_y"], plan["origins_x"])
    z = predictor.tile_logits(tiles)
    assert tuple(z.shape) == (6, 4, 32, 32) and z.dtype == torch.float32
    want_labels, _, mixed = T.predict(z.cpu().numpy(), plan["origins_y"], plan["origins_x"], (48, 80), 16, 8)
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    _check_conf(conf[None], mixed[None], "tileconf of the predictor")
    again = predictor(x)
    assert torch.equal(again[0], labels) and torch.equal(again[1], conf)


# ------------------------------------------------------------------------------------------------ CLI
SIZES = [(40, 56), (33, 70), (24, 50)]                   # (H0, W0); the last is lower than the tile


def test_predict_tiled_cli_round_trip(tmp_path):
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    source = tmp_path / "photos"
    os.makedirs(source / "sub")
    rng = np.random.default_rng(11)
    paths = []
    for k, (h0, w0) in enumerate(SIZES):
        p = source / ("sub" if k == 1 else "") / f"part_{k}.png"
        Image.fromarray(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)).save(p)
        paths.append(str(p))
    paths = sorted(paths)
    model = _model()
    ckpt = tmp_path / "model.pth"
    save_checkpoint(model, get_optimizer(model), 0, 0.0, str(ckpt))
    names = ["background", "pitting", "spalling", "scrape"]

    def expected(scale):
        predictor = tiling.TiledPredictor(model, (32, 32), 8, 4)
        out = []
        for p in paths:
            image = torch.from_numpy(np.array(Image.open(p).convert("RGB"), dtype=np.uint8))
            original = (int(image.shape[0]), int(image.shape[1]))
            frame_hw = predict_tiled.working_frame(original, scale)
            labels, conf, plan = predictor(predict_tiled.load_frame(image, frame_hw, torch.device(DEV)))
            rec = describe_class_regions(labels[None], 4, conf[None], 1)
            (entry,) = defects.defect_entries(rec, names, frame_hw, [original])
            out.append((labels.cpu().numpy(), float(conf.double().mean()), plan, frame_hw, original, entry))
        return out

    out = tmp_path / "out"
    argv = ["--task", "gear", "--checkpoint", str(ckpt), "--input", str(source), "--tile", "32", "32", "--min_overlap", "8",
            "--batch_size", "4", "--num_workers", "0", "--output_dir", str(out)]
    res = subprocess.run([sys.executable, "-m", "tiaozhanbei_unet_amd.predict_tiled", *argv, "--save_overlays"], cwd=ROOT,
                         capture_output=True, text=True, timeout=400)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "Predictions saved to" in res.stdout

    def check(folder, scale):
        got = json.load(open(folder / "predictions.json"))
        assert set(got) == {"args", "class_names", "images", "summary"} and got["class_names"] == names
        assert (got["args"]["tile"], got["args"]["min_overlap"], got["args"]["scale"]) == ([32, 32], 8, scale)
        assert [e["image_path"] for e in got["images"]] == paths
        total = {n: 0 for n in names[1:]}
        for e, (labels, mean, plan, frame_hw, original, entry) in zip(got["images"], expected(scale)):
            assert set(e) == {"image_path", "name", "original_size", "frame_size", "tiling", "mean_confidence",
                              "defect_pixels", "defects", "decision"}
            assert e["original_size"] == list(original) and e["frame_size"] == list(frame_hw)
            assert e["tiling"] == plan and e["mean_confidence"] == mean
            assert e["defects"] == entry["defects"] and e["decision"] == entry["decision"]
            assert e["defect_pixels"] == {n: int((labels == k).sum()) for k, n in enumerate(names) if k}
            for d in e["defects"]:
                total[d["class_name"]] += 1
                if scale == 1.0:                        # the frame is the image: boxes in its own pixels
                    assert d["bbox_original"] == d["bbox"] and d["centroid_original"] == d["centroid"]
            png = Image.open(folder / "masks" / (e["name"] + ".png"))
            assert png.mode == "P" and png.size == (original[1], original[0])        # the image's own size
            want = labels if frame_hw == original else np.array(
                Image.fromarray(labels).resize((original[1], original[0]), Image.NEAREST))
            assert np.array_equal(np.array(png), want), e["name"]
        assert got["summary"] == {"images": 3, "rejected": sum(e["decision"] == "reject" for e in got["images"]),
                                  "defects": total}
        return got

    first = check(out, 1.0)
    assert [e["name"] for e in first["images"]] == ["part_0", "part_2", "sub__part_1"]
    assert [len(e["tiling"]["origins_y"]) * len(e["tiling"]["origins_x"]) for e in first["images"]] == [4, 2, 6]
    assert first["images"][1]["tiling"]["tile"] == [24, 32]
    assert sum(first["summary"]["defects"].values()) > 0          # a random head predicts something
    for e, (h0, w0) in zip(first["images"], (SIZES[0], SIZES[2], SIZES[1])):
        sheet = Image.open(out / "overlays" / (e["name"] + ".png"))
        assert sheet.mode == "RGB" and sheet.size == (2 * w0 + 4, h0)

    # a second run, in this process, writes the same bytes
    kept = {f: open(out / f, "rb").read() for f in ["predictions.json"] + [f"masks/{e['name']}.png" for e in first["images"]]}
    predict_tiled.main(argv + ["--save_overlays"])
    for f, data in kept.items():
        assert open(out / f, "rb").read() == data, f

    half = tmp_path / "half"
    predict_tiled.main(argv[:-1] + [str(half), "--scale", "0.75"])
    second = check(half, 0.75)
    assert [e["frame_size"] for e in second["images"]] == [[30, 42], [18, 38], [25, 52]]
    assert not os.path.exists(half / "overlays")
