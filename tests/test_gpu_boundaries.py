"""GPU tests of the boundary distance transform and the outline statistics (csrc/distance.hip through
ops.boundary_distance_sq, ops.BoundaryMatcher and the C entries) against the numpy restatement of tests/_boundary_ref.py
(pinned to scipy and a brute-force minimum by test_cpu_boundaries.py), and of the eval_boundaries CLI end to end.
Everything is integer arithmetic: equality is exact.  The frames are those of test_gpu_detection.py (one pixel, a row and a
column that are no whole wave, odd sizes, more than one block each way) plus 3 x 1100, a row longer than a workgroup so
that every lane takes several outputs, and the limits 2 x 4096 and 4096 x 2."""
import ctypes
import json

import numpy as np
import pytest
import torch

import _boundary_ref as B
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import eval_boundaries, ops, seg_boundaries

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAMES = [(1, 1), (1, 70), (70, 1), (33, 31), (64, 96), (65, 33), (3, 1100)]
FRAME_IDS = [f"{h}x{w}" for h, w in FRAMES]
C = 4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _patterns(h, w, seed):
    """name -> uint8 [h, w] maps of C = 4 classes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    p = {"background": np.zeros((h, w), np.uint8), "full": np.full((h, w), 2, np.uint8)}
    p["random"] = rng.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), (h, w))
    blobs = np.zeros((h, w), np.uint8)
    for c, (cy, cx) in zip((1, 2, 3, 1), rng.random((4, 2))):                    # discs that touch and overlap
        blobs[(yy - cy * h) ** 2 + (xx - cx * w) ** 2 <= (0.3 * max(h, w)) ** 2] = c
    p["blobs"] = blobs
    p["columns"] = np.where(xx % 2 == 0, 1, 0).astype(np.uint8)                  # 1-pixel vertical stripes on even x
    p["rows"] = np.where(yy % 2 == 0, 3, 0).astype(np.uint8)                     # 1-pixel horizontal stripes on even y
    one = np.zeros((h, w), np.uint8)
    one[rng.integers(0, h), rng.integers(0, w)] = 2
    p["one pixel"] = one
    disc = np.zeros((h, w), np.uint8)                                            # class 1 alone: no boundary of 2 and 3
    disc[(yy - 0.5 * h) ** 2 + (xx - 0.5 * w) ** 2 <= (0.25 * max(h, w)) ** 2] = 1
    p["disc"] = disc
    return p


NAMES = ("background", "full", "random", "blobs", "columns", "rows", "one pixel", "disc")


def _perturbed(m, seed):
    """a prediction that mostly agrees: a tenth of the pixels redrawn"""
    rng = np.random.default_rng(seed)
    out = m.copy()
    redraw = rng.random(m.shape) < 0.1
    out[redraw] = rng.integers(0, 4, int(redraw.sum()), dtype=np.uint8)
    return out


_REF = {}


def _ref_d2(maps):
    key = (maps.shape, maps.tobytes())
    if key not in _REF:
        _REF[key] = B.boundary_distance_sq(maps, C)
    return _REF[key]


def _truth_and_pred(h, w):
    p = _patterns(h, w, seed=h * 131 + w)
    truth = np.stack([p[n] for n in NAMES])
    pred = np.stack([_perturbed(p[n], k) for k, n in enumerate(NAMES)])
    pred[1] = 0                                        # full against background: the truth's class 2 has no outline either
    pred[7] = np.roll(p["disc"], 1, axis=1) * 3        # the disc, one pixel to the right, as ANOTHER class: both one-sided
    return truth, pred


MARGIN = 256    # bytes of sentinel on each side of every buffer
SENTINEL = 0xA5


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + MARGIN


def _distance_through_c(maps):
    """d2 [n, C - 1, h, w] of the C entry, with sentinels around the output and the workspace"""
    n, h, w = maps.shape
    lib, vp = L.lib(), ctypes.c_void_p
    need = lib.unet_boundary_distance_sq_workspace(n, h, w, C)
    assert need == (n * (C - 1) * 4 + 15) // 16 * 16
    t = _dev(maps)
    out, ws = _guarded(n * (C - 1) * h * w * 4), _guarded(need)
    rc = lib.unet_boundary_distance_sq(vp(t.data_ptr()), n, h, w, C, vp(out[1]), vp(ws[1]), need, None)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, _ in (out, ws):
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all())
    return out[0][MARGIN:-MARGIN].view(torch.int32).cpu().numpy().reshape(n, C - 1, h, w).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the distance
@pytest.mark.parametrize("h, w", FRAMES, ids=FRAME_IDS)
def test_distance_equals_the_reference(h, w):
    truth, _ = _truth_and_pred(h, w)                   # a batch of eight images, some without a boundary of some class
    want = _ref_d2(truth)
    got = ops.boundary_distance_sq(_dev(truth), C)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(NAMES), C - 1, h, w) and got.is_cuda
    got = got.cpu().numpy().astype(np.int64)
    for i, name in enumerate(NAMES):
        assert np.array_equal(got[i], want[i]), name
    # BOUNDARY_NONE per (image, class), not per batch
    assert bool((got[0] == B.NONE).all()) and bool((got[1] == B.NONE).all())     # background; a full frame has no outline
    assert bool((got[7, 1:] == B.NONE).all())
    if h * w > 1:
        assert int(got[6, 1].max()) < B.NONE and bool((got[6, [0, 2]] == B.NONE).all())      # one pixel of class 2
    if min(h, w) > 2:
        assert all(int(got[2, c].max()) < B.NONE for c in range(C - 1))
    assert np.array_equal(_distance_through_c(truth[2:5]), want[2:5])
    # int64 labels: 255 and a value >= num_classes are background
    odd = truth[2].astype(np.int64)
    odd[truth[2] == 0] = np.where(np.arange(int((truth[2] == 0).sum())) % 2 == 0, 255, 7)
    again = ops.boundary_distance_sq(_dev(odd[None]), C).cpu().numpy()
    assert np.array_equal(again[0], want[2])


@pytest.mark.parametrize("h, w", [(2, 4096), (4096, 2)], ids=["2x4096", "4096x2"])
def test_distance_at_the_largest_sides(h, w):
    corner = np.zeros((h, w), np.uint8)
    corner[h - 1, w - 1] = 1                           # every lane of the far end scans the whole row
    ends = np.zeros((h, w), np.uint8)
    ends[0, 0] = ends[h - 1, w - 1] = 3
    maps = np.stack([corner, ends])
    got = ops.boundary_distance_sq(_dev(maps), C).cpu().numpy().astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    far = (yy - (h - 1)) ** 2 + (xx - (w - 1)) ** 2
    assert np.array_equal(got[0, 0], far) and np.array_equal(got[1, 2], np.minimum(far, yy ** 2 + xx ** 2))
    assert int(got[0, 0].max()) == 4095 ** 2 + 1
    assert bool((got[0, 1:] == B.NONE).all()) and bool((got[1, :2] == B.NONE).all())
    assert np.array_equal(got, _ref_d2(maps))


# ------------------------------------------------------------------------------------------------ the records
def _compute(matcher):
    got = matcher.compute()
    assert got["records"].dtype == np.int64 and got["hist"].dtype == np.int64
    return got


@pytest.mark.parametrize("h, w", FRAMES, ids=FRAME_IDS)
def test_records_equal_the_reference(h, w):
    truth, pred = _truth_and_pred(h, w)
    want, want_hist = B.stats(truth, pred, C, (0, 1, 4), band=3)
    matcher = ops.BoundaryMatcher(C, (0, 1, 4), band_width=3)
    matcher.update(_dev(pred), _dev(truth))
    got = _compute(matcher)
    for i, name in enumerate(NAMES):
        rows = slice(i * (C - 1), (i + 1) * (C - 1))
        assert got["records"][rows].tolist() == want[rows].tolist(), name
    assert np.array_equal(got["hist"], want_hist)
    assert got["images"] == len(NAMES) and got["band_widths"] == [3] * len(NAMES) and got["tolerances"] == (0, 1, 4)
    assert got["image_sizes"] == [(h, w)] * len(NAMES)
    r = got["records"]
    assert bool((r[:, B.F["p_near3"]] == 0).all()) and bool((r[:, B.F["t_near3"]] == 0).all())      # three tolerances
    for side in "pt":
        near = [r[:, B.F[f"{side}_near{k}"]] for k in range(3)]
        assert bool((near[0] <= near[1]).all() and (near[1] <= near[2]).all() and (near[2] <= r[:, B.F[f"{side}_boundary"]]).all())
    assert bool((r[:, B.F["band_inter"]] <= r[:, B.F["band_union"]]).all())
    # the full frame against background and the disc against a disc of another class: outlines on one side only
    one_sided = r[[1 * 3 + 1, 7 * 3 + 0, 7 * 3 + 2]]
    assert bool((one_sided[:, B.F["p_near0"]:B.F["band_inter"]] == 0).all()) and bool((one_sided[:, B.F["p_dist_sum_q8"]:] == 0).all())
    # one tolerance and the 2 % rule; a second compute gives the same bytes
    want, want_hist = B.stats(truth, pred, C, (2,), band=B.band_width(h, w))
    matcher = ops.BoundaryMatcher(C, (2,))
    matcher.update(_dev(pred), _dev(truth))
    got = _compute(matcher)
    assert got["records"].tolist() == want.tolist() and np.array_equal(got["hist"], want_hist)
    assert got["band_widths"] == [B.band_width(h, w)] * len(NAMES)
    again = ops.BoundaryMatcher(C, (2,))
    again.update(_dev(pred), _dev(truth))
    assert _compute(again)["records"].tobytes() == got["records"].tobytes() == matcher.compute()["records"].tobytes()


def test_identical_maps_have_every_distance_zero():
    truth, _ = _truth_and_pred(65, 33)
    matcher = ops.BoundaryMatcher(C, (0, 1, 4), band_width=2)
    matcher.update(_dev(truth), _dev(truth))
    got = _compute(matcher)
    r, f = got["records"], B.F
    want, want_hist = B.stats(truth, truth, C, (0, 1, 4), band=2)
    assert r.tolist() == want.tolist() and np.array_equal(got["hist"], want_hist)
    assert int(r[:, f["t_boundary"]].sum()) > 0
    for k in range(3):
        assert np.array_equal(r[:, f[f"p_near{k}"]], r[:, f["p_boundary"]])
        assert np.array_equal(r[:, f[f"t_near{k}"]], r[:, f["t_boundary"]])
    assert np.array_equal(r[:, f["band_inter"]], r[:, f["band_union"]]) and int(r[:, f["band_union"]].sum()) > 0
    assert not r[:, f["p_dist_sum_q8"]:].any()
    assert int(got["hist"][:, :, 1:].sum()) == 0
    assert np.array_equal(got["hist"][:, 0, 0], got["hist"][:, 1, 0])
    assert int(got["hist"].sum()) == 2 * int(r[:, f["t_boundary"]].sum())
    # int64 labels whose background is 255 and 7 (>= num_classes) give the same records
    odd = truth.astype(np.int64)
    odd[truth == 0] = np.where(np.arange(int((truth == 0).sum())) % 2 == 0, 255, 7)
    _, pred = _truth_and_pred(65, 33)
    odd_pred = pred.astype(np.int64)
    odd_pred[pred == 0] = 7
    plain, other = ops.BoundaryMatcher(C, (0, 1, 4), band_width=2), ops.BoundaryMatcher(C, (0, 1, 4), band_width=2)
    plain.update(_dev(pred), _dev(truth))
    other.update(_dev(odd_pred), _dev(odd))
    assert _compute(other)["records"].tolist() == _compute(plain)["records"].tolist() == B.stats(odd, odd_pred, C, (0, 1, 4), 2)[0].tolist()
    assert np.array_equal(other.compute()["hist"], plain.compute()["hist"])


def test_updates_of_different_frames_run_on():
    matcher = ops.BoundaryMatcher(C)                   # tolerances 1 2 4, the 2 % rule per update
    want, hist, base, widths, sizes = [], None, 0, [], []
    for (h, w), pick in (((33, 31), [2, 3]), ((65, 33), [3]), ((1, 70), [0, 1, 2])):
        truth, pred = _truth_and_pred(h, w)
        truth, pred = truth[pick], pred[pick]
        matcher.update(_dev(pred.astype(np.int64)), _dev(truth.astype(np.int32)))
        rec, hist = B.stats(truth, pred, C, (1, 2, 4), band=B.band_width(h, w), image_base=base, hist=hist)
        want.append(rec)
        base += len(pick)
        widths += [B.band_width(h, w)] * len(pick)
        sizes += [(h, w)] * len(pick)
    got = _compute(matcher)
    assert got["records"].tolist() == np.concatenate(want).tolist()
    assert got["records"][:, 0].tolist() == [i for i in range(6) for _ in range(C - 1)]
    assert np.array_equal(got["hist"], hist) and int(hist.sum()) > 0
    assert (got["images"], got["band_widths"], got["image_sizes"]) == (6, widths, sizes) and widths[:3] == [1, 1, 1]


def test_stats_through_c_add_to_what_is_there():
    truth, pred = _truth_and_pred(33, 31)
    truth, pred = truth[2:5], pred[2:5]
    n, h, w = truth.shape
    want, want_hist = B.stats(truth, pred, C, (1, 3), band=2, image_base=9)
    t, p = _dev(truth), _dev(pred)
    d2 = ops.boundary_distance_sq(torch.cat([t, p]), C)
    rec, hist = _guarded(n * (C - 1) * 20 * 8), _guarded((C - 1) * 2 * 1025 * 8)
    rec[0][MARGIN:-MARGIN] = 0
    hist[0][MARGIN:-MARGIN].view(torch.int64).fill_(5)
    vp, tol = ctypes.c_void_p, (ctypes.c_int32 * 2)(1, 9)
    rc = L.lib().unet_boundary_stats(vp(t.data_ptr()), vp(p.data_ptr()), vp(d2[:n].data_ptr()), vp(d2[n:].data_ptr()), n, h,
                                     w, C, tol, 2, 4, 9, vp(rec[1]), vp(hist[1]), None)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, _ in (rec, hist):
        assert bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all())
    assert rec[0][MARGIN:-MARGIN].view(torch.int64).cpu().numpy().reshape(-1, 20).tolist() == want.tolist()
    assert np.array_equal(hist[0][MARGIN:-MARGIN].view(torch.int64).cpu().numpy().reshape(C - 1, 2, 1025), want_hist + 5)


def test_unsupported_arguments_are_refused():
    maps = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="boundary_distance_sq: 1 x 8 x 8 maps of 33 classes"):
        ops.boundary_distance_sq(maps, 33)
    with pytest.raises(RuntimeError, match="not supported"):
        ops.boundary_distance_sq(maps, 1)
    with pytest.raises(RuntimeError, match="not supported"):
        ops.boundary_distance_sq(torch.zeros((1, 1, 4097), dtype=torch.uint8, device=DEV), 4)
    with pytest.raises(ValueError, match="integer label maps"):
        ops.boundary_distance_sq(maps.float(), 4)
    with pytest.raises(ValueError, match="shapes differ"):
        ops.BoundaryMatcher(4).update(maps, maps[:, :4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.BoundaryMatcher(4).update(maps.cpu(), maps.cpu())
    lib, vp = L.lib(), ctypes.c_void_p
    out = torch.zeros(4096, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"status -2\): unet_boundary_distance_sq: n=1 h=4097 w=8 num_classes=4"):
        L.check(lib.unet_boundary_distance_sq(vp(maps.data_ptr()), 1, 4097, 8, 4, vp(out.data_ptr()), vp(out.data_ptr()),
                                              1 << 12, None), "unet_boundary_distance_sq")
    torch.cuda.synchronize()
    assert not bool(out.any())                         # nothing was launched


# ------------------------------------------------------------------------------------------------ CLI
RESULT_KEYS = {"evaluation_args", "class_names", "images", "mode", "tolerances", "band_width", "overall", "per_class",
               "unmatched"}


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
            preds.append(ops.seg_confidence(model(x))[0].cpu().numpy())
            masks.append(m.cpu().numpy())
    masks = np.concatenate(masks)
    return np.concatenate(preds), np.where((masks >= 0) & (masks < 255), masks, 255).astype(np.uint8)


def _check_outputs(save, mode, paths, class_names, tolerances, sizes, width):
    res = json.load(open(save / "boundary_results.json"))
    assert set(res) == RESULT_KEYS
    assert res["mode"] == mode and res["images"] == len(paths) and res["class_names"] == class_names
    assert res["tolerances"] == tolerances == res["evaluation_args"]["boundary_tolerances"]
    assert res["band_width"] == seg_boundaries.BAND_WIDTH_RULE and res["evaluation_args"]["boundary_width"] == width
    assert set(res["per_class"]) == set(class_names[1:]) == set(res["unmatched"]["per_class"])
    for f in [res["overall"]] + list(res["per_class"].values()):
        assert list(f["tolerances"]) == [str(t) for t in tolerances]
        for at in f["tolerances"].values():
            assert at["pred_near"] <= f["pred_boundary"] and at["truth_near"] <= f["truth_boundary"]
            assert 0.0 <= at["boundary_f1"] <= 1.0
        assert f["band_inter"] <= f["band_union"] and 0.0 <= f["boundary_iou"] <= 1.0
        assert f["truth_boundary"] <= f["truth_pixels"] and f["pred_boundary"] <= f["pred_pixels"]
        assert f["hausdorff_mean"] <= f["hausdorff_max"]
    assert res["overall"]["records"] == len(paths) * (len(class_names) - 1)
    per_image = json.load(open(save / "per_image_boundaries.json"))
    assert [e["image_path"] for e in per_image] == paths
    for e, (h, w) in zip(per_image, sizes):
        assert e["band_width"] == (width or B.band_width(h, w)) and set(e["classes"]) <= set(class_names[1:])
    for key, own in (("truth_pixels", "truth_pixels"), ("pred_boundary", "pred_boundary"), ("band_union", "band_union")):
        assert sum(c[own] for e in per_image for c in e["classes"].values()) == res["overall"][key]
    return res


def test_eval_boundaries_cli_gear_frame_and_tiled(tmp_path, capsys):
    from tiaozhanbei_unet_amd import crops
    from tiaozhanbei_unet_amd import gear_dataset as G
    root = G.write_synthetic_gear(str(tmp_path / "gear"))
    ckpt = tmp_path / "model.pth"
    model = _fresh_checkpoint(ckpt, 4, seed=1)
    ds = G.GearDataset(root, "test", (64, 64), raw=True)
    samples = [ds[i] for i in range(len(ds))]
    names, paths = ["background"] + list(ds.class_names), list(ds.image_paths)
    pre = G.GearPreprocess((64, 64), train=False)
    batches = []
    for i in range(0, len(samples), 3):
        images, polys, sizes, _ = G.collate_raw(samples[i:i + 3])
        batches.append(pre(images, polys, sizes, device=DEV))
    pred, truth = _second_pass(model, batches)
    assert int(((truth > 0) & (truth < 4)).sum()) > 0  # the synthetic tree has defects to outline
    common = ["--dataset", "gear", "--checkpoint", str(ckpt), "--data_root", root, "--image_size", "64", "--batch_size", "3",
              "--num_workers", "0"]
    capsys.readouterr()
    eval_boundaries.main(common + ["--save_dir", str(tmp_path / "frame")])
    out = capsys.readouterr().out
    assert "b-IoU" in out and "F1@4" in out and "Boundary results saved" in out
    res = _check_outputs(tmp_path / "frame", "frame", paths, names, [1, 2, 4], [(64, 64)] * len(paths), 0)
    rec, hist = B.stats(truth, pred, 4, (1, 2, 4), band=B.band_width(64, 64))
    want = seg_boundaries.boundary_results(rec, hist, len(paths), 4, (1, 2, 4), names)
    for key in ("overall", "per_class", "unmatched"):
        assert res[key] == json.loads(json.dumps(want[key])), key

    images, polys, sizes, _ = G.collate_raw(samples)
    own = [tuple(m.shape) for m in crops.full_resolution_masks(polys, sizes, device=DEV)]
    assert len(set(own)) > 1                           # images of several sizes: one update and one band width each
    eval_boundaries.main(common + ["--save_dir", str(tmp_path / "tiled"), "--tiled", "--tile", "64", "64", "--min_overlap", "8",
                                   "--boundary_tolerances", "0", "3", "--boundary_width", "2"])
    res = _check_outputs(tmp_path / "tiled", "tiled", paths, names, [0, 3], own, 2)
    assert res["evaluation_args"]["tile"] == [64, 64] and res["evaluation_args"]["min_overlap"] == 8
    full = [m.cpu().numpy() for m in crops.full_resolution_masks(polys, sizes, device=DEV)]
    assert res["overall"]["truth_pixels"] == sum(int(((m > 0) & (m < 4)).sum()) for m in full)


def test_eval_boundaries_cli_kolektorsdd(tmp_path):
    from tiaozhanbei_unet_amd import kolektorsdd_dataset as K
    root = K.write_synthetic_kolektorsdd(str(tmp_path / "kol"), n_folders=6, per_folder=5)
    ckpt = tmp_path / "model.pth"
    model = _fresh_checkpoint(ckpt, 3)
    ds = K.KolektorSDDDataset(root, "test", (64, 32), raw=True)
    pre = K.GpuPreprocess((64, 32), train=False)
    samples = [ds[i] for i in range(len(ds))]
    batches = [pre(*K.collate_raw(samples[i:i + 2])[:2], device=DEV) for i in range(0, len(samples), 2)]
    pred, truth = _second_pass(model, batches)
    eval_boundaries.main(["--dataset", "kolektorsdd", "--checkpoint", str(ckpt), "--data_root", root, "--image_height", "64",
                          "--image_width", "32", "--batch_size", "2", "--num_workers", "0", "--save_dir", str(tmp_path / "b"),
                          "--boundary_tolerances", "2", "--boundary_width", "3"])
    res = _check_outputs(tmp_path / "b", "frame", list(ds.image_paths), list(K.CLASS_NAMES), [2], [(64, 32)] * len(ds), 3)
    rec, hist = B.stats(truth, pred, 3, (2,), band=3)
    want = seg_boundaries.boundary_results(rec, hist, len(ds), 3, (2,), list(K.CLASS_NAMES))
    for key in ("overall", "per_class", "unmatched"):
        assert res[key] == json.loads(json.dumps(want[key])), key
    with pytest.raises(SystemExit):
        eval_boundaries.main(["--dataset", "kolektorsdd", "--checkpoint", str(ckpt), "--tiled"])
