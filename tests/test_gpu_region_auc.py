"""Region labelling and AUPRO on the device (ops.label_regions, ops.RegionOverlapAUC -> csrc/regions.hip,
csrc/rankauc.hip) against the exact restatement of tests/_region_auc_ref.py (pinned by test_cpu_region_auc.py): labels,
sizes and counts must EQUAL scipy's 8-connected components on random and adversarial masks; AUPRO must agree to the
bound the fp64 AUPRC sum is held to, across the sort's boundaries, ties, special scores and limits; bitwise invariance
to how the images are batched; no host synchronisation in update; the evaluation CLI's region block."""
import json
import os

import numpy as np
import pytest
import torch

from _rank_auc_ref import rank_auc64
from _region_auc_ref import aupro64, regions64

pytestmark = pytest.mark.gpu

TOL = 1e-12        # the bound tests/test_gpu_rank_auc.py holds the ordered fp64 AUPRC sum to
FMAX = float(np.finfo(np.float32).max)


def _ops():
    from tiaozhanbei_unet_amd import ops
    return ops


# ---- labelling ---------------------------------------------------------------------------------------------------------
def _check_labels(masks, select=None):
    """masks: bool [n, h, w]"""
    masks = np.ascontiguousarray(masks, bool)
    truth = torch.as_tensor(masks.astype(np.float32)).cuda()
    labels, sizes, counts = _ops().label_regions(truth, select=select)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.shape == truth.shape
    labels, sizes, counts = labels.cpu().numpy(), sizes.cpu().numpy(), counts.cpu().tolist()
    on = np.ones(len(masks), bool) if select is None else np.asarray(torch.as_tensor(select).cpu().numpy(), bool)
    want = [0, 0, 0]
    for i, m in enumerate(masks):
        if not on[i]:
            assert not labels[i].any() and not sizes[i].any(), i
            continue
        wl, ws, n = regions64(m)
        assert np.array_equal(labels[i], wl), (i, np.argwhere(labels[i] != wl)[:5])
        assert np.array_equal(sizes[i], ws), (i, np.argwhere(sizes[i] != ws)[:5])
        want = [want[0] + n, want[1] + int(m.sum()), want[2] + int((~m).sum())]
    assert counts == want
    return counts


@pytest.mark.parametrize("density", [0.01, 0.3, 0.59, 0.9])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 257), (1, 257, 1), (2, 37, 53), (2, 64, 64), (1, 255, 257),
                                   (1, 1024, 1024), (3, 1408, 512)])
def test_random_masks(shape, density):
    rng = np.random.default_rng(shape[1] * 7 + shape[2] + int(density * 100))
    _check_labels(rng.random(shape) < density)


def _spiral(n):
    """a one-pixel-wide spiral with one-pixel gaps: one region, the longest chain an n x n image holds"""
    m = np.zeros((n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    inside = lambda a, b: 0 <= a < n and 0 <= b < n
    moved = True
    while moved:
        moved = False
        for _ in range(2):                                          # straight on, else one turn to the right
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(ay, ax) and m[ay, ax]):
                y, x, moved = ny, nx, True
                m[y, x] = True
                break
            dy, dx = dx, -dy
    return m


def test_spiral_is_one_region():
    m = _spiral(256)
    assert regions64(m)[2] == 1 and 0.4 < m.mean() < 0.6
    assert _check_labels(m[None])[0] == 1
    assert _check_labels(np.stack([m[::-1, ::-1], m.T]))[0] == 2       # the root is found from the far end too


def test_serpentine_checkerboard_stripes_and_full_images():
    h, w = 130, 197
    serp = np.zeros((h, w), bool)
    serp[::2] = True
    serp[1::4, -1] = True
    serp[3::4, 0] = True
    assert regions64(serp)[2] == 1
    board = (np.indices((h, w)).sum(0) % 2).astype(bool)
    diag = (np.indices((h, w)).sum(0) % 3 == 0)                    # anti-diagonals: 8-connected lines
    anti = ((np.indices((h, w))[0] - np.indices((h, w))[1]) % 4 == 0)
    rows = np.zeros((h, w), bool)
    rows[::2] = True                                                # every other row: h / 2 regions across all tiles
    cols = rows.T[:h, :h]
    _check_labels(np.stack([serp, board, diag, anti, np.ones((h, w), bool), np.zeros((h, w), bool), rows]))
    _check_labels(cols[None])
    _check_labels(np.ones((1, 512, 512), bool))


def test_frame_enclosing_single_pixels_and_regions_across_every_tile_border():
    m = np.zeros((200, 200), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    m[2:-2:3, 2:-2:3] = True                                        # isolated pixels inside the frame
    counts = _check_labels(m[None])
    assert counts[0] == 1 + 66 * 66
    cross = np.zeros((160, 160), bool)
    for k in range(1, 5):                                           # 2 x 2 blocks on every tile corner, bars across the edges
        for j in range(1, 5):
            cross[32 * k - 1:32 * k + 1, 32 * j - 1:32 * j + 1] = True
        cross[32 * k - 1:32 * k + 1, 10:14] = True
        cross[100:104, 32 * k - 1:32 * k + 1] = True
    cross[31, 40], cross[32, 41] = True, True                       # corner contacts only
    cross[64, 50], cross[63, 49] = True, True
    _check_labels(cross[None])


def test_identical_images_do_not_leak_and_select_masks_images_out():
    rng = np.random.default_rng(5)
    m = rng.random((70, 90)) < 0.4
    counts = _check_labels(np.stack([m, m, m]))
    assert counts[0] == 3 * regions64(m)[2]
    batch = rng.random((6, 40, 70)) < 0.35
    sel = np.array([1, 0, 1, 1, 0, 0], bool)
    _check_labels(batch, select=sel)
    _check_labels(batch, select=torch.as_tensor(sel).cuda())
    assert _check_labels(batch, select=np.zeros(6, bool)) == [0, 0, 0]


# ---- AUPRO -------------------------------------------------------------------------------------------------------------
def _aupro(pred, truth, limit=0.3, select=None):
    m = _ops().RegionOverlapAUC(limit)
    m.update(pred, truth, select=select)
    return m.compute()


def _expect(got, pred, truth, limit=0.3, select=None):
    p, t = pred.cpu().numpy(), truth.cpu().numpy()
    if select is not None:
        sel = np.asarray(torch.as_tensor(select).cpu().numpy(), bool)
        p, t = p[sel], t[sel]
    want = aupro64(p, t > 0.5, limit)
    print(f"aupro {got['aupro']!r} want {want['aupro']!r} diff {abs(got['aupro'] - want['aupro']):.3e}  "
          f"pro@L diff {abs(got['pro_at_limit'] - want['pro_at_limit']):.3e}")
    for k in ("regions", "defective", "ok", "nonfinite", "fpr_limit"):
        assert got[k] == want[k], (k, got, want)
    assert abs(got["aupro"] - want["aupro"]) <= TOL, (got, want)
    assert abs(got["pro_at_limit"] - want["pro_at_limit"]) <= TOL, (got, want)
    return want


def _make(shape, frac, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    truth = (torch.rand(shape, generator=g, device="cuda") < frac).float()
    if kind == "continuous":
        pred = torch.randn(shape, generator=g, device="cuda") * 2.0 + 0.7 * truth
    else:
        q = 256.0 if kind == "q256" else 4096.0
        pred = torch.round((torch.rand(shape, generator=g, device="cuda") * 0.8 + 0.2 * truth) * q) / q
    return pred.contiguous(), truth.contiguous()


# the totals of tests/test_gpu_rank_auc.py (wave, block, tile and digit-table boundaries), as 2-D images
SMALL = [(1, 1, 1), (1, 1, 2), (1, 1, 63), (1, 8, 8), (1, 5, 13), (1, 15, 17), (4, 8, 8), (1, 1, 257), (1, 63, 65),
         (1, 17, 241), (1, 65537, 1)]
FRACS = [0.005, 0.05, 0.5]
KINDS = ["continuous", "q256", "q4096"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("shape", SMALL)
def test_small_totals(shape, frac, kind):
    pred, truth = _make(shape, frac, kind, seed=sum(shape) + int(frac * 1000))
    _expect(_aupro(pred, truth), pred, truth)


@pytest.mark.parametrize("shape, frac, kind", [
    ((1, 1, 1000003), 0.005, "continuous"), ((1, 1000003, 1), 0.05, "q256"), ((1, 1001, 999), 0.5, "q4096"),
    ((100, 1, 256, 256), 0.05, "continuous"), ((100, 1, 256, 256), 0.005, "q4096"), ((100, 1, 256, 256), 0.5, "q256"),
    ((1, 4097, 8191), 0.05, "q4096"),
])
def test_large_totals(shape, frac, kind):
    pred, truth = _make(shape, frac, kind, seed=shape[-1] % 1000)
    _expect(_aupro(pred, truth), pred, truth)


@pytest.mark.parametrize("limit", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("kind", KINDS)
def test_limits(kind, limit):
    pred, truth = _make((7, 1, 96, 80), 0.08, kind, seed=int(limit * 100))
    _expect(_aupro(pred, truth, limit), pred, truth, limit)


@pytest.mark.parametrize("kind", KINDS)
def test_single_pixel_regions_at_limit_one_equal_binary_auroc(kind):
    """every region has one pixel and the whole curve is integrated: AUPRO is the AUROC of another kernel path"""
    pred, truth = _make((5, 1, 128, 96), 0.3, kind, seed=21)
    keep = torch.zeros_like(truth)
    keep[..., ::2, ::2] = 1
    truth = truth * keep                                            # defects at even rows and columns only
    got = _expect(_aupro(pred, truth, 1.0), pred, truth, 1.0)
    assert got["regions"] == got["defective"] > 0
    auc = _ops().BinaryAUC()
    auc.update(pred, truth)
    roc = auc.compute()["auroc"]
    assert abs(_aupro(pred, truth, 1.0)["aupro"] - roc) <= TOL
    assert abs(roc - rank_auc64(pred.cpu().numpy(), truth.cpu().numpy() > 0.5)["auroc"]) <= TOL


def test_limit_on_a_curve_point_and_inside_a_tie_run():
    truth = np.zeros((1, 4, 10), np.float32)
    truth[0, 0, :2] = 1
    pred = np.zeros((1, 4, 10), np.float32)
    pred[0, 0, 0] = 0.9                                             # the other defective pixel ties with 19 ok pixels at 0
    pred.reshape(-1)[2:21] = 0.5                                    # 19 ok pixels: the curve (0, .5), (.5, .5), (1, 1)
    p, t = torch.as_tensor(pred).cuda(), torch.as_tensor(truth).cuda()
    for limit, aupro, pro in ((0.5, 0.5, 0.5), (0.25, 0.5, 0.5), (0.75, 0.40625 / 0.75, 0.75), (1.0, 0.625, 1.0)):
        got = _aupro(p, t, limit)
        _expect(got, p, t, limit)
        assert abs(got["aupro"] - aupro) <= TOL and abs(got["pro_at_limit"] - pro) <= TOL
    rng = np.random.default_rng(3)                                  # a limit of k / N on larger, tie-heavy data
    y = (rng.random((2, 50, 64)) < 0.1).astype(np.float32)
    s = (np.round(rng.random((2, 50, 64)) * 16) / 16 + 0.25 * y).astype(np.float32)
    n_ok = int((y < 0.5).sum())
    p, t = torch.as_tensor(s).cuda(), torch.as_tensor(y).cuda()
    for k in (1, n_ok // 16, max(1, int(np.sum(s[y < 0.5] >= 0.75))), n_ok - 1, n_ok):
        _expect(_aupro(p, t, k / n_ok), p, t, k / n_ok)


@pytest.mark.parametrize("n_def", [10, 2048, 1])
def test_all_scores_equal(n_def):
    truth = np.zeros((1, 271, 259), np.float32)
    truth.reshape(-1)[:n_def] = 1
    p, t = torch.full((1, 271, 259), 0.375).cuda(), torch.as_tensor(truth).cuda()
    for limit in (0.3, 0.05, 1.0):
        got = _aupro(p, t, limit)
        _expect(got, p, t, limit)
        assert abs(got["aupro"] - limit / 2) <= TOL and abs(got["pro_at_limit"] - limit) <= TOL


def test_perfect_and_inverted_separation():
    rng = np.random.default_rng(4)
    y = rng.random((5, 60, 50)) < 0.1
    s = np.where(y, 2.0 + rng.random(y.shape), rng.random(y.shape)).astype(np.float32)
    p, t = torch.as_tensor(s).cuda(), torch.as_tensor(y.astype(np.float32)).cuda()
    got = _aupro(p, t)
    _expect(got, p, t)
    assert abs(got["aupro"] - 1.0) <= TOL and abs(got["pro_at_limit"] - 1.0) <= TOL
    inv = _aupro(-p, t)
    _expect(inv, -p, t)
    assert inv["aupro"] == 0.0 and inv["pro_at_limit"] == 0.0
    assert abs(_aupro(-p, t, 1.0)["aupro"]) <= TOL


def test_signed_zeros_subnormals_and_extreme_scores():
    rng = np.random.default_rng(2)
    pool = np.array([-FMAX, -1e3, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 2e-45, 1e-40, np.finfo(np.float32).tiny, 0.5, 1e3,
                     FMAX, np.nextafter(np.float32(FMAX), np.float32(0))], np.float32)
    s = pool[rng.integers(0, pool.size, (3, 61, 67))]
    y = (rng.random((3, 61, 67)) < 0.3).astype(np.float32)
    p, t = torch.as_tensor(s).cuda(), torch.as_tensor(y).cuda()
    for limit in (0.3, 1.0):
        got = _aupro(p, t, limit)
        _expect(got, p, t, limit)
        plus = _aupro(torch.where(p == 0, torch.zeros_like(p), p), t, limit)
        assert (got["aupro"], got["pro_at_limit"]) == (plus["aupro"], plus["pro_at_limit"])   # -0.0 and +0.0 are one value


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("on_defect", [False, True])
def test_non_finite_scores_give_zero(bad, on_defect):
    pred, truth = _make((4, 1, 40, 25), 0.2, "continuous", seed=5)
    idx = (truth[2, 0] > 0.5).nonzero()[0] if on_defect else (truth[2, 0] < 0.5).nonzero()[0]
    pred[2, 0, idx[0], idx[1]] = bad
    got = _aupro(pred, truth)
    assert (got["aupro"], got["pro_at_limit"], got["nonfinite"]) == (0.0, 0.0, 1)
    _expect(got, pred, truth)


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_no_regions_or_no_ok_pixels_give_zero(label):
    pred, _ = _make((2, 1, 20, 25), 0.5, "continuous", seed=6)
    got = _aupro(pred, torch.full_like(pred, label))
    assert (got["aupro"], got["pro_at_limit"]) == (0.0, 0.0)
    assert (got["regions"], got["defective"], got["ok"]) == ((2, 1000, 0) if label else (0, 0, 1000))
    assert _ops().RegionOverlapAUC().compute()["aupro"] == 0.0


def test_label_threshold_is_strictly_above_half():
    rng = np.random.default_rng(8)
    levels = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1 / 255, 0.0, 1.0], np.float32)
    y = levels[rng.integers(0, levels.size, (2, 50, 100))]
    s = (rng.random((2, 50, 100)) + 0.3 * (y > 0.5)).astype(np.float32)
    p, t = torch.as_tensor(s).cuda(), torch.as_tensor(y).cuda()
    want = _expect(_aupro(p, t), p, t)
    assert want["defective"] == int(np.sum(y > 0.5)) and int(np.sum(y == 0.5)) > 0


@pytest.mark.parametrize("where", ["host", "device"])
def test_select_masks_images_out(where):
    pred, truth = _make((9, 1, 32, 33), 0.1, "q256", seed=9)
    sel = np.array([1, 0, 0, 1, 1, 0, 1, 0, 1], bool)
    select = torch.as_tensor(sel).cuda() if where == "device" else sel
    got = _aupro(pred, truth, select=select)
    _expect(got, pred, truth, select=sel)
    assert got["defective"] + got["ok"] == 5 * 32 * 33
    none = _aupro(pred, truth, select=np.zeros(9, bool))
    assert (none["aupro"], none["regions"], none["ok"]) == (0.0, 0, 0)


def test_batch_split_and_order_are_bitwise_invariant():
    pred, truth = _make((21, 1, 64, 64), 0.05, "continuous", seed=10)
    truth[:, :, 20:30, 20:40] = 1                                   # large regions beside the small ones
    truth[3:9, :, 40:44] = 1
    pred[:, :, :24] = torch.round(pred[:, :, :24] * 16) / 16        # ties across regions of different sizes
    sel = np.random.default_rng(10).random(21) < 0.8
    results = []
    for parts in (1, 3, 7):
        order = np.random.default_rng(parts).permutation(21)
        cuts = np.sort(np.random.default_rng(parts + 100).choice(np.arange(1, 21), parts - 1, replace=False))
        m = _ops().RegionOverlapAUC()
        for chunk in np.split(order, cuts):
            idx = torch.as_tensor(chunk).cuda()
            m.update(pred[idx], truth[idx], select=sel[chunk] if parts != 3 else torch.as_tensor(sel[chunk]).cuda())
        first, second = m.compute(), m.compute()
        assert first == second
        results.append(first)
    assert results[0] == results[1] == results[2]
    _expect(results[0], pred, truth, select=sel)
    flipped = _ops().RegionOverlapAUC()                             # the same multiset of (score, region size) pixels
    flipped.update(pred.flip(-1), truth.flip(-1), select=sel)
    assert flipped.compute() == results[0]


def test_update_does_not_synchronise():
    pred, truth = _make((6, 1, 48, 48), 0.1, "continuous", seed=11)
    m = _ops().RegionOverlapAUC()
    sel_dev = torch.ones(6, dtype=torch.bool, device="cuda")
    _ops().label_regions(truth)                                     # (library and allocator warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(pred, truth)
        m.update(pred, truth, select=np.array([1, 0, 1, 1, 0, 1], bool))
        m.update(pred, truth, select=sel_dev)
        _ops().label_regions(truth, select=sel_dev)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    got = m.compute()
    assert got["defective"] + got["ok"] == (6 + 4 + 6) * 48 * 48


# ---- the evaluation CLI ------------------------------------------------------------------------------------------------
def _cli(tmp_path, model_name, extra):
    from tiaozhanbei_unet_amd import AnomalyUNet, UNet
    from tiaozhanbei_unet_amd import test as test_cli
    from tiaozhanbei_unet_amd.dataset import write_synthetic_mvtec
    from tiaozhanbei_unet_amd.utils import save_checkpoint
    root = write_synthetic_mvtec(str(tmp_path / "data"), "bottle", n_train=2, n_good=3, n_bad=4, size=64)
    torch.manual_seed(0)
    model = (AnomalyUNet(3, False) if model_name == "anomaly_unet" else UNet(3, 1, False)).cuda()
    ck = str(tmp_path / "model.pth")
    save_checkpoint(model, torch.optim.Adam(model.parameters()), 0, 0.0, ck)
    out = test_cli.main(["--data_root", root, "--category", "bottle", "--model", model_name, "--checkpoint", ck,
                         "--batch_size", "3", "--image_size", "64", "--num_workers", "0", "--output_dir",
                         str(tmp_path / "test_out"), *extra])
    return root, model, ck, json.load(open(os.path.join(out, "test_metrics.json")))


@pytest.mark.parametrize("model_name, limit", [("anomaly_unet", 0.3), ("unet", 0.1)])
def test_cli_binary_masks_write_region_metrics(tmp_path, model_name, limit):
    from tiaozhanbei_unet_amd import test as test_cli
    from tiaozhanbei_unet_amd.dataset import get_dataloaders
    from tiaozhanbei_unet_amd.utils import load_checkpoint
    root, model, ck, tm = _cli(tmp_path, model_name, ["--binary_masks", "--pro_fpr_limit", str(limit)])
    assert tm["args"]["binary_masks"] is True and tm["args"]["pro_fpr_limit"] == limit
    assert len(tm["pixel_metrics"]) == 3                            # no monkey-patched masks needed
    assert list(tm["region_metrics"]) == ["aupro", "pro_at_limit", "fpr_limit", "regions"]
    _, loader = get_dataloaders(root, "bottle", 3, 64, 0, device_preprocess=True)
    load_checkpoint(model, None, ck, torch.device("cuda"))
    res = test_cli.test_model(model, loader, torch.device("cuda"), pixel_thresholds=[0.3, 0.5, 0.7], pro_fpr_limit=limit,
                              binary_masks=True)
    assert set(np.unique(res["masks_true"])) == {0.0, 1.0}
    want = aupro64(res["anomaly_maps"], res["masks_true"] > 0.5, limit)     # every test image: good ones are ok pixels
    assert want["regions"] > 0 and want["ok"] > 0
    for got in (res["pixel_pro"], tm["region_metrics"]):
        assert abs(got["aupro"] - want["aupro"]) <= TOL and abs(got["pro_at_limit"] - want["pro_at_limit"]) <= TOL
        assert got["regions"] == want["regions"] and got["fpr_limit"] == limit
    bad = res["labels"] == 1
    roc = rank_auc64(res["anomaly_maps"][bad], res["masks_true"][bad] > 0.5)
    for entry in tm["pixel_metrics"].values():
        assert abs(entry["auroc"] - roc["auroc"]) <= TOL and abs(entry["auprc"] - roc["auprc"]) <= TOL


def test_cli_default_masks_write_no_region_metrics(tmp_path):
    _, _, _, tm = _cli(tmp_path, "anomaly_unet", [])
    assert "region_metrics" not in tm and tm["pixel_metrics"] == {}
    assert tm["args"]["binary_masks"] is False and tm["args"]["pro_fpr_limit"] == 0.3
    assert list(tm) == ["image_metrics", "pixel_metrics", "type_metrics", "threshold", "args"]
