"""GPU tests of the class-region kernels (csrc/segregions.hip through ops.label_class_regions and
ops.ClassRegionMatcher) against the scipy / numpy restatement of tests/_seg_regions_ref.py (pinned by
test_cpu_seg_regions.py), and of the eval_regions CLI end to end.  Everything is integer arithmetic: equality is exact.
The frames are the smallest at which a union-find on 32x32 tiles can go wrong: one pixel, one row and one column across
two tile borders, less than a tile, a whole number of tiles, one pixel more than a tile each way."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _seg_regions_ref as R
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import ops, seg_regions
from tiaozhanbei_unet_amd.metrics import per_image_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(1, 1), (1, 70), (70, 1), (33, 31), (64, 96), (65, 33)]
FRAME_IDS = [f"{h}x{w}" for h, w in FRAMES]
NAMES4 = ["background", "full", "antidiagonal", "serpentine", "random", "junk", "blobs"]


def _patterns(h, w, seed):
    """name -> uint8 [h, w]; all of them are maps of C = 4 classes but the checkerboard (C = 3)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    p = {"background": np.zeros((h, w), np.uint8), "full": np.full((h, w), 2, np.uint8)}
    p["checkerboard"] = np.where((yy + xx) % 2 == 0, 1, 2).astype(np.uint8)
    p["antidiagonal"] = np.where(xx == w - 1 - yy, 3, 0).astype(np.uint8)      # NE to SW: tiles meet at corners only
    end = np.where((yy // 2) % 2 == 0, w - 1, 0)
    p["serpentine"] = np.where((yy % 2 == 0) | (xx == end), 1, 2).astype(np.uint8)   # class 1 winds, class 2 fills
    p["random"] = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), (h, w))    # about half background: tiny regions
    p["junk"] = rng.choice(np.array([0, 1, 2, 3, 4, 7, 200, 255], np.uint8), (h, w))   # 255 and values >= C
    blobs = np.zeros((h, w), np.uint8)
    for c, (cy, cx) in zip((1, 2, 3, 1), rng.random((4, 2))):                    # discs that touch and overlap
        blobs[(yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (0.3 * max(h, w)) ** 2] = c
    p["blobs"] = blobs
    return p


def _perturbed(m, seed):
    """a prediction that mostly agrees: a tenth of the pixels redrawn"""
    rng = np.random.default_rng(seed)
    out = m.copy()
    redraw = rng.random(m.shape) < 0.1
    out[redraw] = rng.integers(0, 4, int(redraw.sum()), dtype=np.uint8)
    return out


def _cases(h, w):
    """(id, C, truth [n, h, w], pred [n, h, w]): every pattern alone (N = 1) and in batches of three different images"""
    p = _patterns(h, w, seed=h * 131 + w)
    cases = []
    for k, name in enumerate(NAMES4):
        cases.append((name, 4, p[name][None], _perturbed(p[name], k)[None]))
    cases.append(("checkerboard", 3, p["checkerboard"][None], _perturbed(p["checkerboard"], 9)[None]))
    for k in (0, 2, 4):
        names = [NAMES4[(k + i) % len(NAMES4)] for i in range(4)]
        truth = np.stack([p[n] for n in names[:3]])
        pred = np.stack([p[n] for n in names[1:]])                               # another pattern: few common pixels
        cases.append(("+".join(names[:3]), 4, truth, pred))
    board = p["checkerboard"]
    cases.append(("checkerboards", 3, np.stack([board, 3 - board, np.where(p["junk"] == 255, 255, board).astype(np.uint8)]),
                  np.stack([board, board, _perturbed(board, 10)])))
    return cases


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _match(truth, pred, C, min_pixels):
    m = ops.ClassRegionMatcher(C, min_pixels)
    m.update(_dev(pred), _dev(truth))
    return m.compute()


def _assert_result(got, truth, pred, C, min_pixels, what):
    trec, prec = R.match_records(truth, pred, C, min_pixels)
    assert got["truth"].dtype == np.int32 and got["truth"].shape == trec.shape, what
    assert np.array_equal(got["truth"], trec), what
    assert got["pred"].shape == prec.shape and np.array_equal(got["pred"], prec), what
    assert np.array_equal(got["truth_counts"], R.class_regions64(truth, C)[2]), what
    assert np.array_equal(got["pred_counts"], R.class_regions64(pred, C)[2]), what
    assert got["images"] == truth.shape[0]


@pytest.mark.parametrize("h, w", FRAMES, ids=FRAME_IDS)
def test_regions_and_records_equal_the_reference(h, w):
    for name, C, truth, pred in _cases(h, w):
        what = f"{name} {truth.shape}"
        for maps in (truth, pred):
            region, sizes, counts = ops.label_class_regions(_dev(maps), C)
            assert region.dtype == torch.int32 and sizes.dtype == torch.int32 and counts.dtype == torch.int64
            want = R.class_regions64(maps, C)
            for g, r, part in zip((region, sizes, counts), want, ("region", "sizes", "counts")):
                assert np.array_equal(g.cpu().numpy(), r), f"{what}: {part}"
        for min_pixels in (1, 3):                      # dropped predicted regions neither appear nor cover anything
            _assert_result(_match(truth, pred, C, min_pixels), truth, pred, C, min_pixels, f"{what} min {min_pixels}")


def test_hand_drawn_cases_on_the_device():
    yy, xx = np.mgrid[0:6, 0:6]
    board = np.where((yy + xx) % 2 == 0, 1, 2).astype(np.uint8)[None]
    region, sizes, counts = ops.label_class_regions(_dev(board), 3)
    assert counts.tolist() == [[0, 1, 1]]              # two regions, each connected through diagonals alone
    assert np.array_equal(region[0].cpu().numpy(), board[0]) and bool((sizes == 18).all())
    touching = np.array([[[1, 1, 2, 2, 0], [1, 1, 2, 2, 0], [0, 0, 0, 0, 3]]], np.uint8)
    region, sizes, counts = ops.label_class_regions(_dev(touching), 4)
    assert region[0].tolist() == [[1, 1, 3, 3, 0], [1, 1, 3, 3, 0], [0, 0, 0, 0, 15]] and counts.tolist() == [[0, 1, 1, 1]]
    pred = np.array([[[1, 1, 1, 2, 0], [0, 1, 0, 2, 0], [0, 0, 0, 0, 0]]], np.uint8)
    got = _match(touching, pred, 4, 3)
    assert got["truth"].tolist() == [[0, 1, 0, 4, 3], [0, 2, 2, 4, 0], [0, 3, 14, 1, 0]]
    assert got["pred"].tolist() == [[0, 1, 0, 4, 3]]


@pytest.mark.parametrize("h, w", [(64, 96), (65, 33)], ids=["64x96", "65x33"])
def test_two_runs_are_bitwise_equal(h, w):
    p = _patterns(h, w, seed=5)
    truth = np.stack([p["random"], p["serpentine"], p["junk"]])
    pred = np.stack([_perturbed(p["random"], 1), p["blobs"], p["random"]])
    first_labels = [t.cpu().numpy().tobytes() for t in ops.label_class_regions(_dev(truth), 4)]
    first = _match(truth, pred, 4, 2)
    for _ in range(2):
        assert [t.cpu().numpy().tobytes() for t in ops.label_class_regions(_dev(truth), 4)] == first_labels
        again = _match(truth, pred, 4, 2)
        for k in ("truth", "pred", "truth_counts", "pred_counts"):
            assert again[k].tobytes() == first[k].tobytes(), k


@pytest.mark.parametrize("h, w", [(33, 31), (65, 33)], ids=["33x31", "65x33"])
def test_matcher_accumulates_over_updates_of_different_sizes(h, w):
    p = _patterns(h, w, seed=11)
    truth = np.stack([p["blobs"], p["background"], p["random"]])
    pred = np.stack([_perturbed(p["blobs"], 3), p["antidiagonal"], _perturbed(p["random"], 4)])
    whole = ops.ClassRegionMatcher(4, 2)
    whole.update(_dev(pred), _dev(truth))
    parts = ops.ClassRegionMatcher(4, 2)
    parts.update(_dev(pred[:2]), _dev(truth[:2]))
    parts.update(_dev(pred[2:]), _dev(truth[2:]))
    a, b = whole.compute(), parts.compute()
    for k in ("truth", "pred", "truth_counts", "pred_counts"):
        assert np.array_equal(a[k], b[k]), k
    assert a["images"] == b["images"] == 3
    _assert_result(b, truth, pred, 4, 2, "2 + 1")
    assert set(b["truth"][:, 0].tolist()) == {0, 2} and 1 in set(b["pred"][:, 0].tolist())      # global image indices
    again = parts.compute()                            # compute leaves the state as it is
    assert all(np.array_equal(again[k], b[k]) for k in ("truth", "pred"))
    # the loaders' masks are int64; what does not fit a class byte is background
    wide = truth.astype(np.int64)
    wide[truth == 0] = np.resize(np.array([0, -1, 255, 256, 300, 1 << 40]), int((truth == 0).sum()))
    m = ops.ClassRegionMatcher(4, 2)
    m.update(_dev(pred), _dev(wide))
    got = m.compute()
    assert np.array_equal(got["truth"], a["truth"]) and np.array_equal(got["pred"], a["pred"])
    empty = ops.ClassRegionMatcher(4).compute()
    assert empty["truth"].shape == (0, 5) and empty["pred"].shape == (0, 5) and empty["images"] == 0


MARGIN = 256    # bytes of sentinel on each side of every buffer
SENTINEL = 0xA5


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + MARGIN


def test_outputs_workspace_and_short_record_buffers_stay_in_bounds():
    n, h, w, C, cap = 3, 65, 33, 4, 4
    p = _patterns(h, w, seed=2)
    truth, pred = np.stack([p["random"], p["serpentine"], p["junk"]]), np.stack([p["junk"], p["random"], p["blobs"]])
    both = _dev(np.concatenate([truth, pred]))
    lib, px, vp = L.lib(), n * h * w, ctypes.c_void_p
    need = lib.unet_label_class_regions_workspace(2 * n, h, w, C)
    need_m = lib.unet_match_class_regions_workspace(n, h, w, C)
    assert need == need_m == (px * 8 + 15) // 16 * 16
    bufs = {k: _guarded(b) for k, b in (("region", 2 * px * 4), ("sizes", 2 * px * 4), ("counts", 2 * n * C * 8),
                                        ("ws", need), ("ws_m", need_m), ("trec", cap * 20), ("prec", cap * 20),
                                        ("rec_counts", 16))}
    for k in ("counts", "rec_counts"):
        bufs[k][0][MARGIN:-MARGIN] = 0
    L.check(lib.unet_label_class_regions(vp(both.data_ptr()), 2 * n, h, w, C, vp(bufs["region"][1]), vp(bufs["sizes"][1]),
                                         vp(bufs["counts"][1]), vp(bufs["ws"][1]), need, None),
            "unet_label_class_regions")
    reg, siz = bufs["region"][1], bufs["sizes"][1]
    L.check(lib.unet_match_class_regions(vp(both.data_ptr()), vp(reg), vp(siz), vp(both.data_ptr() + px),
                                         vp(reg + 4 * px), vp(siz + 4 * px), n, h, w, C, 1, 0, vp(bufs["trec"][1]),
                                         vp(bufs["prec"][1]), cap, vp(bufs["rec_counts"][1]), vp(bufs["ws_m"][1]),
                                         need_m, None), "unet_match_class_regions")
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all()), k
    want = R.class_regions64(np.concatenate([truth, pred]), C)
    inner = {k: bufs[k][0][MARGIN:-MARGIN] for k in bufs}
    assert np.array_equal(inner["region"].view(torch.int32).cpu().numpy().reshape(2 * n, h, w), want[0])
    assert np.array_equal(inner["sizes"].view(torch.int32).cpu().numpy().reshape(2 * n, h, w), want[1])
    assert np.array_equal(inner["counts"].view(torch.int64).cpu().numpy().reshape(2 * n, C), want[2])
    trec, prec = R.match_records(truth, pred, C)
    assert len(trec) > cap and len(prec) > cap         # both buffers are too short: counted, not written
    assert inner["rec_counts"].view(torch.int64).tolist() == [len(trec), len(prec)]
    kept = inner["trec"].view(torch.int32).cpu().numpy().reshape(cap, 5)
    assert all(r.tolist() in trec.tolist() for r in kept)


def test_unsupported_shapes_raise():
    x = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    for c in (1, 256):
        with pytest.raises(RuntimeError, match="2..255 classes"):
            ops.label_class_regions(x, c)
    with pytest.raises(ValueError):
        ops.ClassRegionMatcher(4, 0)
    with pytest.raises(ValueError):
        ops.ClassRegionMatcher(4).update(x, x[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_class_regions(x.cpu(), 4)


# ------------------------------------------------------------------------------------------------ CLI
def _run(module, *argv):
    res = subprocess.run([sys.executable, "-m", f"tiaozhanbei_unet_amd.{module}", *argv], cwd=ROOT, capture_output=True,
                         text=True, timeout=400)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return res.stdout


def _fresh_checkpoint(path, n_classes, seed=0):
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd.train_utils import get_optimizer
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    torch.manual_seed(seed)
    model = SegmentationUNet(3, n_classes, precision="fp32").to(DEV)
    save_checkpoint(model, get_optimizer(model), 0, 0.0, str(path))
    return model


def _second_pass(model, batches):
    """the model's own argmax labels and the loader's masks, on the host"""
    model.eval()
    preds, masks = [], []
    with torch.no_grad():
        for x, m in batches:
            preds.append(per_image_stats(model(x), labels=True)["labels"].cpu().numpy())
            masks.append(m.cpu().numpy())
    return np.concatenate(preds), np.concatenate(masks)


def _check_cli_outputs(save, pred, masks, n_classes, class_names, paths, min_pixels, thresholds):
    truth = np.where((masks >= 0) & (masks < 255), masks, 255).astype(np.uint8)
    trec, prec = R.match_records(truth, pred, n_classes, min_pixels)
    want = seg_regions.region_metrics(trec, prec, len(paths), n_classes, thresholds, class_names)
    res = json.load(open(save / "region_results.json"))
    assert set(res) == {"evaluation_args", "class_names", "images", "min_region_pixels", "image_level", "thresholds",
                        "mean_coverage"}
    assert res["class_names"] == class_names and res["min_region_pixels"] == min_pixels
    assert res["images"] == len(paths) and res["evaluation_args"]["min_region_pixels"] == min_pixels
    assert list(res["thresholds"]) == [repr(float(t)) for t in thresholds]
    for k, v in json.loads(json.dumps(want)).items():
        assert res[k] == v, k
    per_region = json.load(open(save / "per_region_results.json"))
    alarms = prec[~seg_regions.covered(prec, thresholds[0])]
    assert len(per_region) == len(trec) + len(alarms)
    assert [e["kind"] for e in per_region] == ["truth"] * len(trec) + ["false_alarm"] * len(alarms)
    width = masks.shape[-1]
    for e, r in zip(per_region, np.concatenate([trec, alarms])):
        assert e == {"kind": e["kind"], "image_path": paths[r[0]], "class": class_names[r[1]], "y": int(r[2]) // width,
                     "x": int(r[2]) % width, "size": int(r[3]), "hit": int(r[4]), "coverage": int(r[4]) / int(r[3])}
    return len(trec), len(prec)


def test_eval_regions_cli_gear_and_eval_gear_unchanged(tmp_path):
    from tiaozhanbei_unet_amd import gear_dataset as G
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ckpt = tmp_path / "model.pth"
    model = _fresh_checkpoint(ckpt, 4, seed=1)
    ds = G.GearDataset(root, "test", (64, 64), raw=True)
    pre = G.GearPreprocess((64, 64), train=False)
    samples = [ds[i] for i in range(len(ds))]
    batches = []
    for i in range(0, len(samples), 3):
        images, polys, sizes, _ = G.collate_raw(samples[i:i + 3])
        batches.append(pre(images, polys, sizes, device=DEV))
    pred, masks = _second_pass(model, batches)
    names = ["background"] + ds.class_names

    save = tmp_path / "regions"
    out = _run("eval_regions", "--dataset", "gear", "--checkpoint", str(ckpt), "--data_root", root, "--image_size", "64",
               "--batch_size", "3", "--num_workers", "0", "--save_dir", str(save))
    assert "recall" in out and "false/img" in out
    n_truth, _ = _check_cli_outputs(save, pred, masks, 4, names, list(ds.image_paths), 1, [0.0, 0.25, 0.5])
    assert n_truth > 0                                 # the synthetic tree has defects to find

    save = tmp_path / "eval"                           # the pixel-level CLI still writes its two files, key for key
    _run("eval_gear", "--checkpoint", str(ckpt), "--data_root", root, "--image_size", "64", "--batch_size", "3",
         "--num_workers", "0", "--save_dir", str(save))
    res = json.load(open(save / "evaluation_results.json"))
    assert set(res) == {"evaluation_args", "overall_metrics", "per_class_metrics", "confusion_matrix"}
    assert set(res["evaluation_args"]) == {"data_root", "image_size", "split", "model", "checkpoint", "bilinear",
                                           "dropout", "batch_size", "num_workers", "device", "save_dir",
                                           "save_predictions", "save_confusion_matrix", "debug", "debug_samples",
                                           "precision"}
    assert set(res["per_class_metrics"]) == {"iou", "dice", "precision", "recall", "f1"}
    per_image = json.load(open(save / "per_image_results.json"))
    assert len(per_image) == len(ds)
    assert {"image_path", "accuracy", "confidence_mean", "confidence_std"} <= set(per_image[0])
    assert sorted(os.listdir(save)) == ["evaluation_results.json", "per_image_results.json"]


def test_eval_regions_cli_kolektorsdd(tmp_path):
    from tiaozhanbei_unet_amd import kolektorsdd_dataset as K
    root = K.write_synthetic_kolektorsdd(str(tmp_path / "kol"), n_folders=6, per_folder=5)
    ckpt = tmp_path / "model.pth"
    model = _fresh_checkpoint(ckpt, 3)
    ds = K.KolektorSDDDataset(root, "test", (64, 32), raw=True)
    pre = K.GpuPreprocess((64, 32), train=False)
    samples = [ds[i] for i in range(len(ds))]
    batches = [pre(*K.collate_raw(samples[i:i + 2])[:2], device=DEV) for i in range(0, len(samples), 2)]
    pred, masks = _second_pass(model, batches)
    save = tmp_path / "regions"
    _run("eval_regions", "--dataset", "kolektorsdd", "--checkpoint", str(ckpt), "--data_root", root, "--image_height",
         "64", "--image_width", "32", "--batch_size", "2", "--num_workers", "0", "--save_dir", str(save),
         "--min_region_pixels", "3", "--coverage_thresholds", "0.5", "0")
    _check_cli_outputs(save, pred, masks, 3, list(K.CLASS_NAMES), list(ds.image_paths), 3, [0.5, 0.0])
