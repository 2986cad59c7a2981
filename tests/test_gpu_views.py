"""GPU tests of the view ensembling (csrc/views.hip through views.merge_views / ViewEnsemble and the predict_views and
eval_views CLIs) against tests/_views_ref.py, which test_cpu_views.py pins: the merged logits bit for bit, the labels and
the agreement byte for byte, the confidence within _segvis_ref.conf_bound of the float64 confidence of the merged fp32
logits (the scheme of test_gpu_tiles.py).  The cases are the smallest that reach every path: one-pixel and four-pixel
lanes, the reversed 16-byte load, the one-pixel fallback on an aligned frame, up- and downsampling by odd ratios, views
of one row and of one column, one view and sixteen."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _ref64 as R64
import _segvis_ref as S
import _views_ref as VR
from tiaozhanbei_unet_amd import eval_detection, eval_views, ops, predict_tiled, predict_views, tiling, views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# name -> (frame (h, w), [((hv, wv), flip_x, flip_y)], takes the 16-byte path)
CASES = {
    "7x9-scalar": ((7, 9), [((7, 9), 0, 0), ((7, 9), 1, 1), ((4, 5), 0, 0), ((14, 18), 0, 1), ((11, 13), 1, 0)], False),
    "40x32-vector": ((40, 32), [((40, 32), 0, 0), ((40, 32), 1, 0), ((20, 16), 0, 0), ((60, 48), 0, 1)], True),
    "5x64-a-row-and-a-column": ((5, 64), [((1, 64), 0, 0), ((5, 1), 0, 0)], True),
    "8x8-one-view": ((8, 8), [((8, 8), 0, 0)], True),
    "8x8-sixteen-views": ((8, 8), [((8, 8), k & 1, (k >> 1) & 1) for k in range(16)], True),
}


def _flips(name):
    return [(fx, fy) for _hw, fx, fy in CASES[name][1]]


@functools.lru_cache(maxsize=None)
def _tied(name):
    h, w = CASES[name][0]
    return np.random.default_rng(h * w).random((h, w)) < 0.5


@functools.lru_cache(maxsize=None)
def _view_logits(name, c):
    """random fp32 logits N(0, 4^2) per view; on half the pixels of the FRAME classes 0 and c - 1 tie, exactly, above the
    rest, in every view at every sample the pixel's taps read (the interpolation and the sum treat both classes alike and
    keep order: they tie on top in every view's value and in the merged logits).  Built once, read-only."""
    (h, w), specs, _ = CASES[name]
    rng = np.random.default_rng(100 * c + h + w)
    ys, xs = np.nonzero(_tied(name))
    out = []
    for (hv, wv), fx, fy in specs:
        z = (rng.standard_normal((c, hv, wv)) * 4.0).astype(np.float32)
        y0, y1, _ = VR.taps(h, hv, bool(fy))
        x0, x1, _ = VR.taps(w, wv, bool(fx))
        where = np.zeros((hv, wv), bool)
        for ya in (y0, y1):
            for xa in (x0, x1):
                where[ya[ys], xa[xs]] = True
        top = (z.max(axis=0) + np.float32(1.0)).astype(np.float32)
        z[0] = np.where(where, top, z[0])
        z[c - 1] = np.where(where, top, z[c - 1])
        z.setflags(write=False)
        out.append(z)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _want(name, c):
    merged, labels, agreement = VR.merge(_view_logits(name, c), _flips(name), CASES[name][0])
    for a in (merged, labels, agreement):
        a.setflags(write=False)
    return merged, labels, agreement


def _on_device(name, c):
    return [torch.from_numpy(np.array(z)).to(DEV) for z in _view_logits(name, c)]


def _check_conf(out, z, what):
    """out against the float64 confidence of the fp32 logits z [N, C, ...]: test_gpu_tiles.py's bound -- max(4 x host
    error, 2^-22) for expf, measured on the host's fp32 evaluation of the same formula, + the derived terms of
    S.conf_bound"""
    c = z.shape[1]
    ref = torch.from_numpy(S.conf64(z))
    host = torch.from_numpy(S.conf32(z))
    derived = c * np.exp(-1.0) * U + (c - 1) * U + U
    worst = R64.assert_measured(out, (ref, ref), host, what, extra=derived)
    host_rel, kernel_rel, allowed = R64.MEASURED[what]
    total, _ = S.conf_bound(c, host_rel)
    assert abs(total - allowed) <= 1e-12 * allowed
    return worst, host_rel, kernel_rel, allowed


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_cases_are_what_their_names_say():
    for name, ((h, w), specs, vec) in CASES.items():
        assert vec == (w % 4 == 0), name
        assert all(1 <= hv and 1 <= wv for (hv, wv), _, _ in specs)
    assert len(CASES["8x8-sixteen-views"][1]) == 16 and len(set(_flips("8x8-sixteen-views"))) == 4
    assert any(hw == (40, 32) and fx for hw, fx, _ in CASES["40x32-vector"][1])       # the reversed 16-byte load
    assert not any(hw == (5, 64) for hw, _, _ in CASES["5x64-a-row-and-a-column"][1])


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_merge_against_the_restatement(name, c):
    (h, w), specs, _ = CASES[name]
    zd, flips = _on_device(name, c), _flips(name)
    want_merged, want_labels, want_agreement = _want(name, c)
    labels, conf, agreement, merged = views.merge_views(zd, flips, (h, w), merged=True)
    assert (labels.dtype, conf.dtype, agreement.dtype, merged.dtype) == (torch.uint8, torch.float32, torch.uint8, torch.float32)
    assert tuple(labels.shape) == tuple(conf.shape) == tuple(agreement.shape) == (h, w) and tuple(merged.shape) == (c, h, w)
    assert np.array_equal(_bits(merged), _bits(want_merged)), (name, c)
    assert np.array_equal(labels.cpu().numpy(), want_labels), (name, c)
    assert np.array_equal(agreement.cpu().numpy(), want_agreement), (name, c)
    what = f"viewconf {name} c{c}"
    worst, host_rel, kernel_rel, allowed = _check_conf(conf[None], merged.cpu().numpy()[None], what)
    print(f"REF64 {what}: host err {host_rel / U:.2f} u, kernel err {kernel_rel / U:.2f} u, allowed {allowed / U:.2f} u, "
          f"worst err / bound {worst:.3f}")
    # each output may be left out in turn: the others are the same bytes
    full = {"labels": labels, "conf": conf, "agreement": agreement, "merged": merged}
    for left_out in full:
        got = views.merge_views(zd, flips, (h, w), **{k: k != left_out for k in full})
        got = dict(zip(("labels", "conf", "agreement", "merged"), tuple(got) + (None,) * (4 - len(got))))
        assert got[left_out] is None
        assert all(torch.equal(got[k], full[k]) for k in full if k != left_out), (name, c, left_out)
    only = views.merge_views(zd, flips, (h, w), labels=False, conf=False)      # agreement alone
    assert only[0] is None and only[1] is None and torch.equal(only[2], agreement)
    # the planted ties are there in the merged logits, the first maximum took them, and every view agrees there
    tied = _tied(name)
    assert 0.3 < tied.mean() < 0.7 and (want_merged[0] == want_merged[c - 1])[tied].all()
    assert (want_merged[0] == want_merged.max(axis=0))[tied].all() and (want_labels[tied] == 0).all()
    assert (want_agreement[tied] == len(specs)).all() and int(want_agreement.max()) <= len(specs)
    if sum(hw == (h, w) for hw, _, _ in specs) > 1 and c > 2:
        # two views of the frame's own size carry independent logits off the ties: elsewhere the views do disagree (the
        # row and the column of 5 x 64 are tied on nearly every sample, as every sample serves some tied pixel)
        assert int(want_agreement.min()) < len(specs)


def test_a_single_view_of_the_frames_size_is_seg_confidence():
    for h, w in ((33, 65), (16, 20)):                  # one-pixel and four-pixel lanes
        z = torch.from_numpy((np.random.default_rng(h).standard_normal((4, h, w)) * 4.0).astype(np.float32)).to(DEV)
        z[1, 0, :5] = z[3, 0, :5] = 9.0                  # ties
        want_labels, want_conf = ops.seg_confidence(z[None])
        labels, conf, agreement, merged = views.merge_views([z], [(0, 0)], (h, w), merged=True)
        assert torch.equal(labels, want_labels[0]) and torch.equal(conf, want_conf[0])
        assert np.array_equal(_bits(merged), _bits(z)) and bool((agreement == 1).all())
        # its own mirror, flagged, changes nothing: (a + a) / 2
        both = views.merge_views([z, torch.flip(z, [1, 2])], [(0, 0), (1, 1)], (h, w), merged=True)
        assert np.array_equal(_bits(both[3]), _bits(z)) and torch.equal(both[0], labels) and bool((both[2] == 2).all())


def test_an_unaligned_first_view_takes_the_one_pixel_path_to_the_same_bytes():
    name, c = "40x32-vector", 3
    (h, w), _, _ = CASES[name]
    zd = _on_device(name, c)
    shifted = torch.empty(zd[0].numel() + 1, device=DEV)[1:].view(zd[0].shape)       # 4 bytes past a 16-byte boundary
    shifted.copy_(zd[0])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    labels, conf, agreement, merged = views.merge_views([shifted] + zd[1:], _flips(name), (h, w), merged=True)
    want_merged, want_labels, want_agreement = _want(name, c)
    assert np.array_equal(_bits(merged), _bits(want_merged))
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(agreement.cpu().numpy(), want_agreement)
    aligned = views.merge_views(zd, _flips(name), (h, w))
    assert torch.equal(aligned[0], labels) and torch.equal(aligned[1], conf) and torch.equal(aligned[2], agreement)


def test_non_default_stream_and_refusals():
    name, c = "40x32-vector", 3
    (h, w), _, _ = CASES[name]
    zd = _on_device(name, c)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        labels, conf, agreement, merged = views.merge_views(zd, _flips(name), (h, w), merged=True)
    stream.synchronize()
    want_merged, want_labels, want_agreement = _want(name, c)
    assert np.array_equal(_bits(merged), _bits(want_merged)) and np.array_equal(labels.cpu().numpy(), want_labels)
    assert np.array_equal(agreement.cpu().numpy(), want_agreement)
    with pytest.raises(RuntimeError, match="2..8 classes"):
        views.merge_views([torch.zeros((9, 4, 4), device=DEV)], [(0, 0)], (4, 4))
    with pytest.raises(RuntimeError, match=r"status -2\): unet_view_merge: a frame of"):
        views.merge_views([torch.zeros((3, 4, 4), device=DEV)], [(0, 0)], (4, 16385))


# ------------------------------------------------------------------------------------------------ the ensemble
class PixelStub(torch.nn.Module):
    """A fixed per-pixel function of the frame: a seeded 3 -> 4 affine map from elementwise operators (the same
    arithmetic wherever the pixel lies in a tile), rounded to multiples of 1/8.  Logits of so few bits make the tile
    blend exact -- every weight times logit and every sum of them is representable, and the division returns the logit
    -- so the blended logits of a frame are this function of its pixels whatever the tiling, and of a mirrored frame the
    mirror of them: what is left to go wrong is the bookkeeping of the views."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.weight = torch.nn.Parameter(torch.randn((4, 3), generator=g) * 2.0)
        self.bias = torch.nn.Parameter(torch.randn((4,), generator=g))

    def forward(self, x):
        w, b = self.weight, self.bias
        z = torch.stack([x[:, 0] * w[k, 0] + x[:, 1] * w[k, 1] + x[:, 2] * w[k, 2] + b[k] for k in range(4)], dim=1)
        return torch.round(z * 8.0) / 8.0


def _stub_ensemble(plan):
    predictor = tiling.TiledPredictor(PixelStub().to(DEV), (32, 32), min_overlap=8, batch_size=4)
    return views.ViewEnsemble(predictor, plan)


def _image(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV)


def test_flips_are_undone_end_to_end():
    image = _image(48, 40, 1)
    ensemble = _stub_ensemble(views.plan_views([1], "all"))
    labels, conf, agreement, plan = ensemble(image, (48, 40))
    merged = ensemble.merged_logits(image, (48, 40))
    logits, again = ensemble.view_logits(image, (48, 40))
    assert again == plan and [(p["scale"], p["flip_x"], p["flip_y"]) for p in plan] == [
        (1.0, False, False), (1.0, True, False), (1.0, False, True), (1.0, True, True)]
    tiles = {"tile": [32, 32], "origins_y": [0, 16], "origins_x": [0, 8], "ramp": [16, 24]}
    assert all(p["frame_size"] == [48, 40] and p["tiling"] == tiles for p in plan)
    assert merged.dtype == torch.float32 and tuple(merged.shape) == (4, 48, 40)
    assert np.array_equal(_bits(merged), _bits(logits[0]))              # (a + a + a + a) / 4 is exact
    assert bool((agreement == 4).all())
    want_labels, want_conf = ops.seg_confidence(logits[0][None])
    assert torch.equal(labels, want_labels[0]) and torch.equal(conf, want_conf[0])
    assert len(torch.unique(labels)) > 1 and not torch.equal(logits[0], logits[1])   # the map is not flat or symmetric
    # the stub is the per-pixel function its docstring says: the identity view's logits are the model on the whole frame
    frame = predict_tiled.load_frame(image, (48, 40), torch.device(DEV))
    with torch.no_grad():
        assert torch.equal(logits[0], ensemble.predictor.model(frame[None])[0])


def test_scales_end_to_end():
    image = _image(48, 40, 2)
    plan_in = views.plan_views([1, 0.5], "h")
    ensemble = _stub_ensemble(plan_in)
    labels, conf, agreement, plan = ensemble(image, (48, 40))
    assert [p["frame_size"] for p in plan] == [[48, 40], [48, 40], [24, 20], [24, 20]]
    assert plan[2]["tiling"] == {"tile": [24, 20], "origins_y": [0], "origins_x": [0], "ramp": [1, 1]}
    logits, _ = ensemble.view_logits(image, (48, 40))
    assert [tuple(z.shape) for z in logits] == [(4, 48, 40)] * 2 + [(4, 24, 20)] * 2
    want_merged, want_labels, want_agreement = VR.merge([z.cpu().numpy() for z in logits],
                                                        [(fx, fy) for _s, fx, fy in plan_in], (48, 40))
    merged = ensemble.merged_logits(image, (48, 40))
    assert np.array_equal(_bits(merged), _bits(want_merged))
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(agreement.cpu().numpy(), want_agreement)
    _check_conf(conf[None], want_merged[None], "viewconf of the ensemble")
    assert int(want_agreement.min()) < 4 <= int(want_agreement.max())    # the half-size views do not always agree
    # an output frame other than the image's: every view is resized
    small = ensemble(image, (36, 30))
    assert tuple(small[0].shape) == (36, 30) and [p["frame_size"] for p in small[3]] == [[36, 30]] * 2 + [[18, 15]] * 2


# ------------------------------------------------------------------------------------------------ CLIs
@functools.lru_cache(maxsize=None)
def _model():
    from tiaozhanbei_unet_amd import SegmentationUNet
    torch.manual_seed(1)
    return SegmentationUNet(3, 4, precision="fp32").to(DEV).eval()


def _checkpoint(path):
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    model = _model()
    save_checkpoint(model, get_optimizer(model), 0, 0.0, str(path))
    return str(path)


def test_mean_view_agreement_of_known_regions():
    from tiaozhanbei_unet_amd.evaluation import describe_class_regions
    labels = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    agreement = torch.full((1, 8, 8), 1, dtype=torch.uint8, device=DEV)
    labels[0, 0:2, 0:4], labels[0, 5:8, 4:8] = 1, 2
    agreement[0, 0, 0:4], agreement[0, 1, 0:4], agreement[0, 5:8, 4:8] = 4, 2, 3
    records = describe_class_regions(labels, 4, None, 1)
    assert records[:, 1].tolist() == [1, 2] and records[:, 3].tolist() == [8, 12]
    assert predict_views.agreement_means(labels, agreement, 4, 4, 1, records) == [0.75, 0.75]
    assert predict_views.agreement_means(labels, agreement, 8, 4, 1, records) == [0.375, 0.375]
    with pytest.raises(RuntimeError, match="differ"):
        predict_views.agreement_means(labels, agreement, 4, 4, 9, records)       # the 8-pixel region is dropped


SIZES = [(40, 56), (36, 70)]                             # (H0, W0)
ADDED = {"views"}


def test_predict_views_cli_round_trip(tmp_path):
    source = tmp_path / "photos"
    os.makedirs(source)
    rng = np.random.default_rng(11)
    for k, (h0, w0) in enumerate(SIZES):
        Image.fromarray(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)).save(source / f"part_{k}.png")
    ckpt = _checkpoint(tmp_path / "model.pth")
    argv = ["--task", "gear", "--checkpoint", ckpt, "--input", str(source), "--tile", "32", "32", "--min_overlap", "8",
            "--batch_size", "4", "--num_workers", "0"]
    predict_tiled.main(argv + ["--output_dir", str(tmp_path / "tiled")])
    predict_views.main(argv + ["--output_dir", str(tmp_path / "one"), "--view_scales", "1", "--view_flips", "none"])
    want = json.load(open(tmp_path / "tiled" / "predictions.json"))
    got = json.load(open(tmp_path / "one" / "predictions.json"))
    assert got["class_names"] == want["class_names"] and got["summary"] == want["summary"]
    assert sum(want["summary"]["defects"].values()) > 0                  # a random head predicts something
    for e, t in zip(got["images"], want["images"]):
        assert set(e) == set(t) | ADDED
        assert all(e[k] == t[k] for k in t if k != "defects"), e["name"]          # mean_confidence and tiling among them
        assert e["views"] == [{"scale": 1.0, "flip_x": False, "flip_y": False, "frame_size": t["frame_size"],
                               "tiling": t["tiling"]}]
        assert len(e["defects"]) == len(t["defects"])
        for d, dt in zip(e["defects"], t["defects"]):
            assert set(d) == set(dt) | {"mean_view_agreement"} and all(d[k] == dt[k] for k in dt)
            assert d["mean_view_agreement"] == 1.0                       # one view agrees with itself
        a, b = (open(tmp_path / f / "masks" / (e["name"] + ".png"), "rb").read() for f in ("one", "tiled"))
        assert a == b, e["name"]

    predict_views.main(argv + ["--output_dir", str(tmp_path / "four"), "--view_scales", "1", "0.5", "--view_flips", "h",
                               "--save_overlays"])
    four = json.load(open(tmp_path / "four" / "predictions.json"))
    assert four["args"]["view_scales"] == [1.0, 0.5] and four["args"]["view_flips"] == "h"
    n_defects = 0
    for e, (h0, w0) in zip(four["images"], SIZES):
        assert [(v["scale"], v["flip_x"], v["flip_y"]) for v in e["views"]] == [(1.0, False, False), (1.0, True, False),
                                                                                (0.5, False, False), (0.5, True, False)]
        assert [v["frame_size"] for v in e["views"]] == [[h0, w0]] * 2 + [[h0 // 2, w0 // 2]] * 2
        assert all(set(v["tiling"]) == {"tile", "origins_y", "origins_x", "ramp"} for v in e["views"])
        for d in e["defects"]:
            assert 0.0 <= d["mean_view_agreement"] <= 1.0
            n_defects += 1
        png = Image.open(tmp_path / "four" / "masks" / (e["name"] + ".png"))
        assert png.mode == "P" and png.size == (w0, h0)
        sheet = Image.open(tmp_path / "four" / "overlays" / (e["name"] + ".png"))
        assert sheet.mode == "RGB" and sheet.size == (2 * w0 + 4, h0)
    assert n_defects > 0


def test_eval_views_cli_against_eval_detection(tmp_path, capsys):
    from tiaozhanbei_unet_amd import gear_dataset as G
    root = G.write_synthetic_gear(str(tmp_path / "gear"), sizes=((96, 80), (72, 64), (80, 80)))
    ckpt = _checkpoint(tmp_path / "model.pth")
    common = ["--dataset", "gear", "--checkpoint", ckpt, "--data_root", root, "--image_size", "64", "--batch_size", "4",
              "--num_workers", "0", "--tile", "32", "32", "--min_overlap", "8", "--min_region_pixels", "4",
              "--coverage_thresholds", "0.5", "0"]
    eval_detection.main(common + ["--save_dir", str(tmp_path / "det"), "--tiled"])
    capsys.readouterr()
    eval_views.main(common + ["--save_dir", str(tmp_path / "views"), "--view_scales", "0.5", "1", "--view_flips", "h"])
    out = capsys.readouterr().out
    assert "4 views" in out and "average_precision" in out and "Mean view agreement at coverage 0.5" in out
    want = json.load(open(tmp_path / "det" / "detection_results.json"))
    got = json.load(open(tmp_path / "views" / "views_results.json"))
    assert set(got) == {"evaluation_args", "class_names", "min_region_pixels", "views", "single", "ensemble", "comparison",
                        "view_agreement"}
    assert got["class_names"] == want["class_names"] and got["min_region_pixels"] == want["min_region_pixels"] == 4
    assert got["views"][0] == {"scale": 1.0, "flip_x": False, "flip_y": False} and len(got["views"]) == 4
    assert [v["scale"] for v in got["views"]] == [1.0, 0.5, 0.5, 1.0]
    keys = {"images", "thresholds", "region_confusion", "panoptic"}
    assert set(got["single"]) == set(got["ensemble"]) == keys
    assert got["single"] == {k: want[k] for k in keys}                   # eval_detection --tiled's own figures
    assert got["single"]["images"] == got["ensemble"]["images"] == 4
    assert got["single"]["thresholds"]["0.5"]["overall"][0]["truth_regions"] > 0
    assert list(got["comparison"]) == ["0.5", "0.0"]
    for key, sides in got["comparison"].items():
        for side in ("single", "ensemble"):
            at, f = got[side]["thresholds"][key], sides[side]
            assert f["average_precision"] == at["average_precision"]["overall"]
            assert f["recall_at_best_f1"] == at["recommended"]["best_f1"]["region_recall"]
            assert f["min_confidence_at_best_f1"] == at["recommended"]["best_f1"]["min_confidence"]
            within = at["recommended"]["within_false_alarm_budget"]
            assert f["recall_within_false_alarm_budget"] == (None if within is None else within["region_recall"])
            assert f["panoptic_quality"] == got[side]["panoptic"]["overall"]["pq"]
    agree = got["view_agreement"]
    first = got["ensemble"]["thresholds"]["0.5"]["overall"][0]
    assert agree["coverage_threshold"] == 0.5 and agree["matched_regions"] == first["matched"]
    assert agree["matched_regions"] + agree["false_alarms"] == first["pred_regions"]
    for k in ("matched_mean", "false_alarm_mean"):
        assert agree[k] is None or 0.0 <= agree[k] <= 1.0
    with pytest.raises(SystemExit):
        eval_views.main(["--dataset", "kolektorsdd", "--checkpoint", ckpt])
