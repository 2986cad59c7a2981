"""GPU tests of the region-pair kernels (csrc/regionpairs.hip through ops.pair_class_regions, the C entries and
ops.DetectionMatcher) against the numpy restatement of tests/_region_pairs_ref.py (pinned by test_cpu_detection.py), and
of the eval_detection CLI end to end.  Everything is integer arithmetic: equality is exact.  The frames are those of
test_gpu_seg_regions.py: one pixel, a row and a column that are no whole wave, less than a block of 2048 pixels with an
odd width (the one-pixel loads), whole 16-byte groups, one pixel more than a tile each way."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _region_pairs_ref as P
import _seg_regions_ref as R
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import eval_detection, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = [(1, 1), (1, 70), (70, 1), (33, 31), (64, 96), (65, 33)]
FRAME_IDS = [f"{h}x{w}" for h, w in FRAMES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _patterns(h, w, seed):
    """name -> uint8 [h, w] maps of C = 4 classes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    p = {"background": np.zeros((h, w), np.uint8), "full": np.full((h, w), 2, np.uint8)}
    p["random"] = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), (h, w))    # about half background: tiny regions
    end = np.where((yy // 2) % 2 == 0, w - 1, 0)
    p["serpentine"] = np.where((yy % 2 == 0) | (xx == end), 1, 2).astype(np.uint8)
    blobs = np.zeros((h, w), np.uint8)
    for c, (cy, cx) in zip((1, 2, 3, 1), rng.random((4, 2))):                    # discs that touch and overlap
        blobs[(yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (0.3 * max(h, w)) ** 2] = c
    p["blobs"] = blobs
    p["columns"] = np.where(xx % 2 == 0, 1, 0).astype(np.uint8)                  # 1-pixel vertical stripes on even x
    p["rows"] = np.where(yy % 2 == 0, 1, 0).astype(np.uint8)                     # 1-pixel horizontal stripes on even y
    return p


def _perturbed(m, seed):
    """a prediction that mostly agrees: a tenth of the pixels redrawn"""
    rng = np.random.default_rng(seed)
    out = m.copy()
    redraw = rng.random(m.shape) < 0.1
    out[redraw] = rng.integers(0, 4, int(redraw.sum()), dtype=np.uint8)
    return out


def _cases(h, w):
    """(id, truth [n, h, w], pred [n, h, w]) label maps of 4 classes"""
    p = _patterns(h, w, seed=h * 131 + w)
    cases = [(f"{name} against its perturbed copy", p[name][None], _perturbed(p[name], k)[None])
             for k, name in enumerate(("random", "blobs", "serpentine"))]
    cases += [("random against blobs", p["random"][None], p["blobs"][None]),
              ("serpentine against random", p["serpentine"][None], p["random"][None]),
              ("full against background", p["full"][None], p["background"][None]),
              ("full against full", p["full"][None], p["full"][None]),
              ("crossed stripes", p["columns"][None], p["rows"][None])]
    again = _perturbed(p["blobs"], 7)
    cases.append(("three images, two of them identical", np.stack([p["blobs"], p["random"], p["blobs"]]),
                  np.stack([again, p["serpentine"], again])))
    return cases


def _regions(maps):
    return ops.label_class_regions(_dev(maps), 4)[0]


def _bound(treg, preg):
    n, h, w = treg.shape
    bound = torch.zeros(n, dtype=torch.int64, device=DEV)
    vp = ctypes.c_void_p
    L.check(L.lib().unet_region_pair_bound(vp(treg.data_ptr()), vp(preg.data_ptr()), n, h, w, vp(bound.data_ptr()), None),
            "unet_region_pair_bound")
    return bound.cpu().numpy()


@pytest.mark.parametrize("h, w", FRAMES, ids=FRAME_IDS)
def test_pairs_equal_the_reference(h, w):
    for name, truth, pred in _cases(h, w):
        what = f"{name} {truth.shape}"
        treg, preg = _regions(truth), _regions(pred)
        want_t, want_p = R.class_regions64(truth, 4)[0], R.class_regions64(pred, 4)[0]
        want = P.pairs(want_t, want_p)
        got = ops.pair_class_regions(treg, preg)
        assert got.dtype == np.int64 and got.shape == want.shape, what
        assert np.array_equal(got, want), what
        assert np.array_equal(_bound(treg, preg), P.pair_starts(want_t, want_p)), what
        if name == "full against background":
            assert got.shape == (0, 4)
        if name == "full against full":
            assert got.tolist() == [[0, 0, 0, h * w]]
        if name == "crossed stripes":
            assert len(got) == -(-w // 2) * -(-h // 2) and bool((got[:, 3] == 1).all())
        if name.startswith("three"):                   # once per image, never merged across images
            first, last = got[got[:, 0] == 0], got[got[:, 0] == 2]
            assert (len(first) > 0 or h * w < 64) and np.array_equal(first[:, 1:], last[:, 1:])
            assert np.array_equal(ops.pair_class_regions(treg, preg, image_base=5), want + [5, 0, 0, 0])
    # region maps at an address that is no multiple of 16 bytes take the one-pixel loads to the same records
    name, truth, pred = _cases(h, w)[0]
    px = h * w
    shifted = torch.zeros(2 * px + 1, dtype=torch.int32, device=DEV)
    shifted[1:px + 1] = _regions(truth).reshape(-1)
    shifted[px + 1:] = _regions(pred).reshape(-1)
    got = ops.pair_class_regions(shifted[1:px + 1].view(1, h, w), shifted[px + 1:].view(1, h, w))
    assert np.array_equal(got, P.pairs_of_labels(truth, pred, 4)), name


def test_one_pair_over_a_whole_frame_counts_above_16_bits():
    full = torch.full((1, 512, 512), 2, dtype=torch.uint8, device=DEV)
    region = ops.label_class_regions(full, 4)[0]
    assert ops.pair_class_regions(region, region).tolist() == [[0, 0, 0, 262144]]
    assert _bound(region, region).tolist() == [512]    # one start per row


MARGIN = 256    # bytes of sentinel on each side of every buffer
SENTINEL = 0xA5


def _guarded(nbytes, zero=False):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    if zero:
        buf[MARGIN:-MARGIN] = 0
    return buf, buf.data_ptr() + MARGIN


def _pairs_through_c(treg, preg, capacity, record_cap, image_base=0):
    """(status, records written [min(count, record_cap), 4], count, overflow) with sentinels around every buffer"""
    n, h, w = treg.shape
    lib, vp = L.lib(), ctypes.c_void_p
    need = lib.unet_region_pairs_workspace(n, capacity)
    assert need == (n * capacity * 12 + 15) // 16 * 16
    bufs = {"records": _guarded(record_cap * 16), "count": _guarded(8, zero=True), "overflow": _guarded(8, zero=True),
            "ws": _guarded(need), "bound": _guarded(8 * n, zero=True)}
    rc = lib.unet_region_pair_bound(vp(treg.data_ptr()), vp(preg.data_ptr()), n, h, w, vp(bufs["bound"][1]), None)
    assert rc == 0
    rc = lib.unet_region_pairs(vp(treg.data_ptr()), vp(preg.data_ptr()), n, h, w, capacity, image_base,
                               vp(bufs["records"][1]), record_cap, vp(bufs["count"][1]), vp(bufs["overflow"][1]),
                               vp(bufs["ws"][1]), need, None)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all()), k
    inner = {k: bufs[k][0][MARGIN:-MARGIN] for k in bufs}
    count, overflow = int(inner["count"].view(torch.int64)), int(inner["overflow"].view(torch.int64))
    records = inner["records"].view(torch.int32).cpu().numpy().reshape(record_cap, 4)
    untouched = records[min(count, record_cap):]
    assert bool((untouched.view(np.uint8) == SENTINEL).all())                    # nothing past the count is written
    return rc, records[:min(count, record_cap)].astype(np.int64), count, overflow, inner["bound"].view(torch.int64).tolist()


def _sorted(rec):
    return rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]


@pytest.mark.parametrize("h, w", [(64, 64), (64, 96), (65, 33)], ids=["64x64", "64x96", "65x33"])
def test_probing_at_a_full_table_and_past_it(h, w):
    """crossed stripes: ceil(w / 2) ceil(h / 2) keys of one pixel each.  64 x 64 makes 1024 of them, a load factor of 1."""
    p = _patterns(h, w, seed=1)
    truth, pred = np.stack([p["columns"], p["columns"]]), np.stack([p["rows"], p["blobs"]])
    treg, preg = _regions(truth), _regions(pred)
    want = P.pairs_of_labels(truth, pred, 4, image_base=3)
    per_image = [int((want[:, 0] == 3 + i).sum()) for i in range(2)]
    most = max(per_image)
    assert most == -(-w // 2) * -(-h // 2)
    capacity = 1 << (most - 1).bit_length()            # the next power of two >= the pairs: a load factor of up to 1
    rc, rec, count, overflow, bound = _pairs_through_c(treg, preg, capacity, len(want), image_base=3)
    assert rc == 0 and overflow == 0 and count == len(want)
    assert np.array_equal(_sorted(rec), want)
    assert all(b >= k for b, k in zip(bound, per_image))
    # half the slots: every slot of the first image's table ends up used, the pixels of the other keys are dropped
    rc, rec, count, overflow, _ = _pairs_through_c(treg, preg, capacity // 2, len(want), image_base=3)
    assert rc == 0 and overflow > 0 and count == len(rec) < len(want)
    assert overflow >= most - capacity // 2            # one pixel a key in the first image
    assert int((rec[:, 0] == 3).sum()) == capacity // 2
    wanted = {tuple(r) for r in want.tolist()}
    assert len({tuple(r) for r in rec.tolist()}) == len(rec) and all(tuple(r) in wanted for r in rec.tolist())
    # a record buffer shorter than the pairs: counted, not written
    rc, rec, count, overflow, _ = _pairs_through_c(treg, preg, capacity, 4, image_base=3)
    assert rc == 0 and overflow == 0 and count == len(want) and len(rec) == 4
    assert all(tuple(r) in wanted for r in rec.tolist())
    rc, rec, count, overflow, _ = _pairs_through_c(treg, preg, capacity, 0, image_base=3)
    assert rc == 0 and count == len(want) and len(rec) == 0


def test_unsupported_arguments_are_refused():
    region = _regions(_patterns(8, 8, 0)["blobs"][None])
    lib, vp = L.lib(), ctypes.c_void_p
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)

    def call(n, h, w, capacity):
        return lib.unet_region_pairs(vp(region.data_ptr()), vp(region.data_ptr()), n, h, w, capacity, 0, vp(out.data_ptr()),
                                     4, vp(out[60:].data_ptr()), vp(out[61:].data_ptr()), vp(ws.data_ptr()), ws.numel(),
                                     None)

    for capacity in (0, 3, 24, -16):
        with pytest.raises(RuntimeError, match=r"status -1\): unet_region_pairs: capacity=-?\d+ is not a power of two"):
            L.check(call(1, 8, 8, capacity), "unet_region_pairs")
    for n, h, w in ((65536, 1, 1), (1, 1 << 16, 1 << 15), (2, 32768, 32768)):
        with pytest.raises(RuntimeError, match=r"status -2\): unet_region_pairs: n="):
            L.check(call(n, h, w, 16), "unet_region_pairs")
        with pytest.raises(RuntimeError, match=r"status -2\): unet_region_pair_bound: n="):
            L.check(lib.unet_region_pair_bound(vp(region.data_ptr()), vp(region.data_ptr()), n, h, w, vp(out.data_ptr()),
                                               None), "unet_region_pair_bound")
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(ws.any())  # nothing was launched
    with pytest.raises(ValueError, match="int32"):
        ops.pair_class_regions(region.long(), region.long())
    with pytest.raises(ValueError, match="differ"):
        ops.pair_class_regions(region, region[:, :4])
    with pytest.raises(ValueError, match="image_base"):
        ops.pair_class_regions(region, region, image_base=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pair_class_regions(region.cpu(), region.cpu())
    with pytest.raises(ValueError):
        ops.DetectionMatcher(4, 0)
    with pytest.raises(ValueError):
        ops.DetectionMatcher(4).update(region.to(torch.uint8), region, region.to(torch.uint8))      # conf is no float tensor


@pytest.mark.parametrize("h, w", [(64, 96), (65, 33)], ids=["64x96", "65x33"])
def test_two_runs_are_bitwise_equal(h, w):
    p = _patterns(h, w, seed=5)
    truth = np.stack([p["random"], p["serpentine"], p["columns"]])
    pred = np.stack([_perturbed(p["random"], 1), p["blobs"], p["rows"]])
    treg, preg = _regions(truth), _regions(pred)
    first = ops.pair_class_regions(treg, preg)
    assert len(first) > 0
    for _ in range(2):
        assert ops.pair_class_regions(treg, preg).tobytes() == first.tobytes()


def _resummed(records, pairs, mine, other, other_records):
    """hit per record: its overlaps with the partners of its own class"""
    cls = {(r[0], r[2]): r[1] for r in other_records.tolist()}
    hit = {(r[0], r[2]): 0 for r in records.tolist()}
    own = {(r[0], r[2]): r[1] for r in records.tolist()}
    for q in pairs.tolist():
        a, b = (q[0], q[mine]), (q[0], q[other])
        if own[a] == cls[b]:
            hit[a] += q[3]
    return [hit[(r[0], r[2])] for r in records.tolist()]


@pytest.mark.parametrize("min_pixels", [1, 5])
def test_detection_matcher_against_class_region_matcher(min_pixels):
    rng = np.random.default_rng(3)
    updates = []
    for (h, w), names in (((33, 31), ("blobs", "random")), ((65, 33), ("random",)), ((1, 70), ("background", "full"))):
        p = _patterns(h, w, seed=11)
        truth = np.stack([p[n] for n in names])
        pred = np.stack([_perturbed(p[n], 3 + k) for k, n in enumerate(names)])
        updates.append((truth, pred, 0.25 + 0.75 * rng.random(truth.shape, dtype=np.float32)))
    detection, matcher = ops.DetectionMatcher(4, min_pixels), ops.ClassRegionMatcher(4, min_pixels)
    want_t, want_p, want_pairs, base = [], [], [], 0
    for truth, pred, conf in updates:
        detection.update(_dev(pred), _dev(conf), _dev(truth))
        matcher.update(_dev(pred), _dev(truth))
        want_t.append(ops.describe_class_regions(_dev(truth), 4, None, 1, image_base=base))
        want_p.append(ops.describe_class_regions(_dev(pred), 4, _dev(conf), min_pixels, image_base=base))
        pairs = P.pairs_of_labels(truth, pred, 4, image_base=base)
        kept = {(r[0], r[2]) for r in want_p[-1].tolist()}
        want_pairs.append(pairs[[(q[0], q[2]) in kept for q in pairs.tolist()]].reshape(-1, 4))
        base += len(truth)
    got, old = detection.compute(), matcher.compute()
    assert got["images"] == old["images"] == 5
    assert got["image_sizes"] == [(33, 31)] * 2 + [(65, 33)] + [(1, 70)] * 2
    for key, want in (("truth", want_t), ("pred", want_p), ("pairs", want_pairs)):
        assert got[key].dtype == np.int64 and np.array_equal(got[key], np.concatenate(want)), key
    assert bool((got["truth"][:, 10:] == 0).all()) and bool((got["pred"][:, 10] > 0).all())
    assert np.array_equal(got["truth"][:, :4], old["truth"][:, :4]) and np.array_equal(got["pred"][:, :4], old["pred"][:, :4])
    assert _resummed(got["truth"], got["pairs"], 1, 2, got["pred"]) == old["truth"][:, 4].tolist()
    assert _resummed(got["pred"], got["pairs"], 2, 1, got["truth"]) == old["pred"][:, 4].tolist()
    if min_pixels > 1:                                 # the rule bites: some predicted regions and their pairs are gone
        assert len(got["pred"]) < sum(len(ops.describe_class_regions(_dev(p), 4)) for _, p, _ in updates)
    again = detection.compute()                        # compute leaves the state as it is
    assert all(np.array_equal(again[k], got[k]) for k in ("truth", "pred", "pairs"))
    empty = ops.DetectionMatcher(4).compute()
    assert empty["truth"].shape == empty["pred"].shape == (0, 12) and empty["pairs"].shape == (0, 4)
    assert empty["images"] == 0 and empty["image_sizes"] == []


# ------------------------------------------------------------------------------------------------ CLI
RESULT_KEYS = {"evaluation_args", "class_names", "images", "mode", "min_region_pixels", "thresholds", "region_confusion",
               "panoptic"}
POINT_KEYS = {"min_confidence", "truth_regions", "detected", "region_recall", "pred_regions", "matched", "region_precision",
              "region_f1", "false_alarms_per_image", "tp", "fp", "fn", "tn"}
TRUTH_KEYS = {"kind", "image_path", "class", "y", "x", "bbox", "size", "detection_score", "best_overlap_class", "best_iou"}
PRED_KEYS = {"kind", "image_path", "class", "y", "x", "bbox", "size", "score", "matched"}


def _checkpoint_of_one_epoch(module, save, *argv):
    exp = module.main(["--epochs", "1", "--val_freq", "1", "--save_freq", "1", "--batch_size", "4", "--num_workers", "0",
                       "--save_dir", str(save), *argv])
    ckpt = os.path.join(exp, "checkpoints", "checkpoint_epoch_0.pth")
    assert os.path.exists(ckpt)
    return ckpt


def _check_outputs(save, mode, paths, class_names, thresholds, min_pixels, n_truth, sizes):
    res = json.load(open(save / "detection_results.json"))
    assert set(res) == RESULT_KEYS
    assert res["mode"] == mode and res["images"] == len(paths) and res["class_names"] == class_names
    assert res["min_region_pixels"] == min_pixels == res["evaluation_args"]["min_region_pixels"]
    assert list(res["thresholds"]) == [repr(float(t)) for t in thresholds]
    for at in res["thresholds"].values():
        assert set(at) == {"overall", "per_class", "average_precision", "recommended"}
        assert set(at["per_class"]) == set(class_names[1:]) == set(at["average_precision"]["per_class"])
        assert set(at["recommended"]) == {"best_f1", "within_false_alarm_budget"}
        for series in [at["overall"]] + list(at["per_class"].values()):
            assert all(set(p) == POINT_KEYS for p in series)
            taus = [p["min_confidence"] for p in series]
            assert taus[0] == 0.0 and taus == sorted(set(taus))
            for a, b in zip(series, series[1:]):       # monotone in the threshold
                assert b["detected"] <= a["detected"] and b["region_recall"] <= a["region_recall"]
                assert b["false_alarms_per_image"] <= a["false_alarms_per_image"] and b["pred_regions"] <= a["pred_regions"]
            assert all(p["tp"] + p["fp"] + p["fn"] + p["tn"] == len(paths) for p in series)
        assert at["overall"][0]["truth_regions"] == n_truth
        assert 0.0 <= at["average_precision"]["overall"] <= 1.0
        assert at["recommended"]["best_f1"] in at["overall"]
    assert set(res["region_confusion"]) == {"rows", "columns", "matrix"}
    assert res["region_confusion"]["columns"] == ["missed"] + class_names[1:]
    assert int(np.sum(res["region_confusion"]["matrix"])) == n_truth
    assert set(res["panoptic"]) == {"overall", "per_class"} and set(res["panoptic"]["overall"]) == {"tp", "fp", "fn", "sq", "rq", "pq"}
    assert res["panoptic"]["overall"]["tp"] + res["panoptic"]["overall"]["fn"] == n_truth
    regions = json.load(open(save / "detection_regions.json"))
    kinds = [e["kind"] for e in regions]
    first = res["thresholds"][repr(float(thresholds[0]))]["overall"][0]
    assert kinds == ["truth"] * n_truth + ["pred"] * first["pred_regions"]
    size_of = dict(zip(paths, sizes))
    for e in regions:
        assert set(e) == (TRUTH_KEYS if e["kind"] == "truth" else PRED_KEYS)
        h, w = size_of[e["image_path"]]
        assert 0 <= e["y"] < h and 0 <= e["x"] < w     # the root in its own image's frame
        x0, y0, x1, y1 = e["bbox"]
        assert 0 <= x0 <= e["x"] <= x1 < w and 0 <= y0 == e["y"] <= y1 < h
        assert e["class"] in class_names[1:] and 1 <= e["size"] <= (x1 - x0 + 1) * (y1 - y0 + 1)
    assert sum(e["kind"] == "pred" and e["matched"] for e in regions) == first["matched"]
    assert sum(e["kind"] == "truth" and e["detection_score"] is not None for e in regions) == first["detected"]
    assert all(e["size"] >= min_pixels for e in regions if e["kind"] == "pred")
    return res


def test_eval_detection_cli_gear_frame_and_tiled(tmp_path, capsys):
    from tiaozhanbei_unet_amd import crops, train_gear
    from tiaozhanbei_unet_amd import gear_dataset as G
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ckpt = _checkpoint_of_one_epoch(train_gear, tmp_path / "runs", "--data_root", root, "--image_size", "64")
    ds = G.GearDataset(root, "test", (64, 64), raw=True)
    images, polys, sizes, paths = G.collate_raw([ds[i] for i in range(len(ds))])
    names = ["background"] + list(ds.class_names)
    assert list(paths) == list(ds.image_paths)
    common = ["--dataset", "gear", "--checkpoint", ckpt, "--data_root", root, "--image_size", "64", "--batch_size", "3",
              "--num_workers", "0"]

    _x, masks = G.GearPreprocess((64, 64), train=False)(images, polys, sizes, device=DEV)
    truth = np.where((masks.cpu().numpy() >= 0) & (masks.cpu().numpy() < 255), masks.cpu().numpy(), 255).astype(np.uint8)
    n_truth = int(R.class_regions64(truth, 4)[2].sum())
    assert n_truth > 0                                 # the synthetic tree has defects to find
    capsys.readouterr()
    eval_detection.main(common + ["--save_dir", str(tmp_path / "frame")])
    out = capsys.readouterr().out
    assert "Recommended --min_confidence" in out and "false/img" in out and "panoptic" in out
    res = _check_outputs(tmp_path / "frame", "frame", list(paths), names, [0.0, 0.25, 0.5], 1, n_truth,
                         [(64, 64)] * len(paths))
    assert res["evaluation_args"]["tile"] == [64, 64] and not res["evaluation_args"]["tiled"]

    full = [m.cpu().numpy() for m in crops.full_resolution_masks(polys, sizes, device=DEV)]
    own = [tuple(m.shape) for m in full]
    assert own == [(int(h), int(w)) for h, w in sizes] and len(set(own)) > 1
    n_full = sum(int(R.class_regions64(m[None], 4)[2].sum()) for m in full)
    eval_detection.main(common + ["--save_dir", str(tmp_path / "tiled"), "--tiled", "--tile", "64", "64", "--min_overlap", "8",
                                  "--min_region_pixels", "4", "--coverage_thresholds", "0.5", "0"])
    res = _check_outputs(tmp_path / "tiled", "tiled", list(paths), names, [0.5, 0.0], 4, n_full, own)
    assert res["evaluation_args"]["tile"] == [64, 64] and res["evaluation_args"]["min_overlap"] == 8


def test_eval_detection_cli_kolektorsdd(tmp_path):
    from tiaozhanbei_unet_amd import kolektorsdd_dataset as K
    from tiaozhanbei_unet_amd import train_kolektorsdd
    root = K.write_synthetic_kolektorsdd(str(tmp_path / "kol"), n_folders=6, per_folder=5)
    ckpt = _checkpoint_of_one_epoch(train_kolektorsdd, tmp_path / "runs", "--data_root", root, "--image_height", "64",
                                    "--image_width", "32")
    ds = K.KolektorSDDDataset(root, "test", (64, 32), raw=True)
    samples = [ds[i] for i in range(len(ds))]
    pre = K.GpuPreprocess((64, 32), train=False)
    masks = np.concatenate([pre(*K.collate_raw(samples[i:i + 2])[:2], device=DEV)[1].cpu().numpy()
                            for i in range(0, len(samples), 2)])
    truth = np.where((masks >= 0) & (masks < 255), masks, 255).astype(np.uint8)
    n_truth = int(R.class_regions64(truth, 3)[2].sum())
    eval_detection.main(["--dataset", "kolektorsdd", "--checkpoint", ckpt, "--data_root", root, "--image_height", "64",
                         "--image_width", "32", "--batch_size", "2", "--num_workers", "0", "--save_dir", str(tmp_path / "det"),
                         "--min_region_pixels", "3", "--max_false_alarms", "0"])
    res = _check_outputs(tmp_path / "det", "frame", list(ds.image_paths), list(K.CLASS_NAMES), [0.0, 0.25, 0.5], 3, n_truth,
                         [(64, 32)] * len(ds))
    assert res["evaluation_args"]["max_false_alarms"] == 0.0
    with pytest.raises(SystemExit):
        eval_detection.main(["--dataset", "kolektorsdd", "--checkpoint", ckpt, "--tiled"])
