"""CPU checks of the AUPRO feature (ops.label_regions, ops.RegionOverlapAUC, csrc/regions.hip, csrc/rankauc.hip): the
exact restatement the GPU tests compare against is pinned here to the walk of the definition in exact fractions, to a
cumsum / argsort formulation in float64 and to hand-computed cases; the C-ABI is exported and refuses bad arguments
before anything reaches a device; the evaluation CLI adds its region block and its two flags."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from _region_auc_ref import EIGHT, aupro64, regions64
from tiaozhanbei_unet_amd import _lib

NAMES = ("unet_label_regions_workspace", "unet_label_regions", "unet_region_auc_append", "unet_region_auc_workspace",
         "unet_region_auc")


def _labelled(masks):
    from scipy.ndimage import label
    return [label(g, EIGHT) for g in masks]


def _cumsum(maps, masks, limit):
    """the evaluation code's construction: per-pixel fp / pro changes, argsort, cumulative sums, the last point of
    each tie run, trapezoids up to the limit (float64)"""
    fp = np.zeros(maps.shape)
    pc = np.zeros(maps.shape)
    n_ok = regions = 0
    for i, (lab, n) in enumerate(_labelled(masks)):
        regions += n
        fp[i][lab == 0] = 1
        n_ok += int((lab == 0).sum())
        for k in range(1, n + 1):
            pc[i][lab == k] = 1.0 / (lab == k).sum()
    s = maps.ravel().astype(np.float64) + 0.0
    order = np.argsort(-s, kind="stable")
    keep = np.append(np.diff(s[order]) != 0, True)
    x = np.r_[0.0, (np.cumsum(fp.ravel()[order]) / n_ok)[keep]]
    y = np.r_[0.0, (np.cumsum(pc.ravel()[order]) / regions)[keep]]
    area = 0.0
    for k in range(1, len(x)):
        if x[k] <= limit:
            area += (x[k] - x[k - 1]) * (y[k - 1] + y[k]) / 2
        else:
            if x[k - 1] < limit:
                yi = y[k - 1] + (y[k] - y[k - 1]) * (limit - x[k - 1]) / (x[k] - x[k - 1])
                area += (limit - x[k - 1]) * (y[k - 1] + yi) / 2
            break
    return area / limit


def _walk(maps, masks, limit):
    """the definition, point by point, in exact fractions: (aupro, pro at the limit), each rounded once"""
    L = Fraction(float(limit))
    pos, neg, regions = {}, {}, 0
    for m, (lab, n) in zip(maps, _labelled(masks)):
        regions += n
        sizes = np.bincount(lab.ravel())
        for v, k in zip(m.ravel().tolist(), lab.ravel().tolist()):
            v = v + 0.0
            if k:
                pos[v] = pos.get(v, Fraction(0)) + Fraction(1, int(sizes[k]))
            else:
                neg[v] = neg.get(v, 0) + 1
    n_ok = sum(neg.values())
    x = y = area = Fraction(0)
    at_limit = None
    for v in sorted(set(pos) | set(neg), reverse=True):
        x1, y1 = x + Fraction(neg.get(v, 0), n_ok), y + pos.get(v, Fraction(0)) / regions
        if x1 > L:
            at_limit = y + (y1 - y) * (L - x) / (x1 - x) if x < L else y
            area += (L - x) * (y + at_limit) / 2
            break
        area += (x1 - x) * (y + y1) / 2
        x, y = x1, y1
    return float(area / L), float(y if at_limit is None else at_limit)


def _case(seed, frac, kind, shape=(3, 24, 29)):
    rng = np.random.default_rng(seed)
    g = rng.random(shape) < frac
    if kind == "continuous":
        maps = rng.standard_normal(shape) + 1.0 * g
    else:
        q = {"q64": 64, "q8": 8}[kind]
        maps = np.round((rng.random(shape) * 0.8 + 0.2 * g) * q) / q
    return maps.astype(np.float32), g


@pytest.mark.parametrize("limit", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("kind", ["continuous", "q64", "q8"])
@pytest.mark.parametrize("frac", [0.02, 0.1, 0.3, 0.45])
def test_restatement_matches_the_walk_and_the_cumsum_formulation(frac, kind, limit):
    maps, g = _case(int(frac * 100), frac, kind)
    got = aupro64(maps, g, limit)
    assert (got["aupro"], got["pro_at_limit"]) == _walk(maps, g, limit)      # both exact, rounded once
    assert abs(got["aupro"] - _cumsum(maps, g, limit)) <= 1e-12
    assert got["regions"] == sum(n for _, n in _labelled(g)) and got["defective"] == int(g.sum())
    assert got["ok"] == int((~g).sum()) and got["nonfinite"] == 0 and got["fpr_limit"] == limit


def test_limit_on_a_curve_point_and_inside_a_tie_run():
    g = np.zeros((1, 4, 10), bool)
    g[0, 0, :2] = True                                        # one region of 2 pixels, 38 ok pixels
    maps = np.zeros((1, 4, 10), np.float32)
    maps[0, 0, 0] = 0.9                                       # the other defective pixel ties with 19 ok pixels at 0
    ok = np.argwhere(~g[0])
    for (y, x) in ok[:19]:
        maps[0, y, x] = 0.5                                   # the curve: (0, 0.5), (0.5, 0.5), (1, 1)
    for limit in (0.5, 0.25, 0.75):
        got = aupro64(maps, g, limit)
        assert (got["aupro"], got["pro_at_limit"]) == _walk(maps, g, limit)
    assert aupro64(maps, g, 0.5)["aupro"] == 0.5 and aupro64(maps, g, 0.5)["pro_at_limit"] == 0.5
    assert aupro64(maps, g, 0.25)["pro_at_limit"] == 0.5      # inside the tie run of the 19 ok pixels at 0.5
    assert aupro64(maps, g, 0.75)["pro_at_limit"] == 0.75     # inside the tie run that holds a defective pixel
    assert aupro64(maps, g, 0.75)["aupro"] == 0.40625 / 0.75 and aupro64(maps, g, 1.0)["aupro"] == 0.625


def test_hand_computed_cases():
    g = np.zeros((1, 16, 16), bool)
    g[0, 3:6, 4:9] = True
    perfect = np.where(g, 0.9, 0.1).astype(np.float32)
    assert aupro64(perfect, g, 0.3)["aupro"] == 1.0 and aupro64(perfect, g, 0.3)["pro_at_limit"] == 1.0
    assert aupro64(-perfect, g, 0.3)["aupro"] == 0.0
    for limit in (0.3, 0.05, 1.0):                            # all equal: the straight line (0, 0) - (1, 1)
        assert abs(aupro64(np.full(g.shape, 0.25, np.float32), g, limit)["aupro"] - limit / 2) <= 1e-15
    # regions of 1 and 100 pixels, only the large one detected: half of the REGIONS are found, not 100/101 of the pixels
    g = np.zeros((1, 32, 32), bool)
    g[0, 0, 0] = True
    g[0, 10:20, 10:20] = True
    maps = np.zeros(g.shape, np.float32)
    maps[0, 10:20, 10:20] = 1.0
    got = aupro64(maps, g, 0.3)
    assert got["regions"] == 2 and abs(got["pro_at_limit"] - 0.65) <= 1e-15
    # pro = 1/2 at fpr 0, then the line to (1, 1): area over [0, L] = L/2 + L^2/4
    assert abs(got["aupro"] - (0.5 + 0.3 / 4)) <= 1e-15


def test_connectivity_is_eight():
    board = (np.indices((8, 8)).sum(0) % 2).astype(bool)
    labels, sizes, n = regions64(board)
    assert n == 1 and set(np.unique(labels)) == {0, 2} and sizes.max() == 32     # root: pixel (0, 1)
    two = np.zeros((5, 5), bool)
    two[1, 1] = two[2, 2] = True
    labels, sizes, n = regions64(two)
    assert n == 1 and labels[1, 1] == labels[2, 2] == 1 + 1 * 5 + 1 and sizes[2, 2] == 2
    apart = np.zeros((5, 5), bool)
    apart[1, 1] = apart[1, 3] = True
    assert regions64(apart)[2] == 2
    assert regions64(np.ones((3, 4), bool))[0].tolist() == [[1] * 4] * 3
    assert regions64(np.zeros((3, 4), bool))[2] == 0


def test_degenerate_cases_give_zero():
    maps, g = _case(1, 0.1, "continuous")
    for bad in (np.nan, np.inf, -np.inf):
        m = maps.copy()
        m[1, 2, 3] = bad
        r = aupro64(m, g, 0.3)
        assert (r["aupro"], r["pro_at_limit"], r["nonfinite"]) == (0.0, 0.0, 1)
    none = aupro64(maps, np.zeros_like(g), 0.3)
    assert (none["aupro"], none["regions"], none["ok"]) == (0.0, 0, g.size)
    full = aupro64(maps, np.ones_like(g), 0.3)
    assert (full["aupro"], full["regions"], full["ok"]) == (0.0, 3, 0)
    flipped = np.where(maps == 0, np.float32(-0.0), maps)
    assert aupro64(flipped, g, 0.3) == aupro64(maps, g, 0.3)


def test_region_symbols_declared_and_exported():
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in NAMES:
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_queries():
    lib = _lib.lib()
    assert lib.unet_label_regions_workspace(1, 1, 1) >= 4
    assert lib.unet_label_regions_workspace(3, 1408, 512) >= 4 * 3 * 1408 * 512
    assert lib.unet_label_regions_workspace(8, 2048, 2048) >= 4 * 8 * 2048 * 2048
    assert lib.unet_label_regions_workspace(1, 1, (1 << 31) - 1) > 0
    assert lib.unet_label_regions_workspace(1, 1 << 16, 1 << 15) == 0               # 2^31 pixels: refused
    assert lib.unet_label_regions_workspace(65536, 4, 4) == 0
    assert lib.unet_label_regions_workspace(0, 4, 4) == 0 and lib.unet_label_regions_workspace(1, -4, 4) == 0
    small = lib.unet_region_auc_workspace(10, 20)
    assert small >= 8 * 10 + 4 * 20 and small % 16 == 0
    assert lib.unet_region_auc_workspace(1 << 20, 5 << 20) >= (8 << 20) + 4 * (5 << 20)
    assert lib.unet_region_auc_workspace(1 << 20, (1 << 31) - (1 << 20) - 1) > 0
    assert lib.unet_region_auc_workspace(1 << 30, 1 << 30) == 0
    assert lib.unet_region_auc_workspace(-1, 5) == 0


def test_abi_refuses_bad_arguments_on_the_host():
    """decided before any launch: no device needed"""
    lib = _lib.lib()
    d = ctypes.c_void_p(256)                           # only checked for NULL / alignment: refused first
    assert lib.unet_label_regions(None, None, 1, 8, 8, d, d, d, d, 1 << 20, None) == -1
    assert lib.unet_label_regions(d, None, 1, 8, 8, d, None, d, d, 1 << 20, None) == -1
    assert lib.unet_label_regions(d, None, 1, 8, 8, d, d, None, d, 1 << 20, None) == -1
    assert lib.unet_label_regions(d, None, 1, 0, 8, d, d, d, d, 1 << 20, None) == -1
    assert lib.unet_label_regions(d, None, 1, 1 << 16, 1 << 15, d, d, d, d, 1 << 40, None) == -2
    assert b"2^31" in lib.unet_last_error()
    assert lib.unet_label_regions(d, None, 65536, 2, 2, d, d, d, d, 1 << 40, None) == -2
    assert lib.unet_label_regions(d, None, 1, 8, 8, d, d, d, d, 16, None) == -3      # workspace too small
    assert lib.unet_region_auc_append(None, d, None, 1, 64, d, 64, d, None) == -1
    assert lib.unet_region_auc_append(d, None, None, 1, 64, d, 64, d, None) == -1
    assert lib.unet_region_auc_append(d, d, None, 1, 64, d, 64, None, None) == -1
    assert lib.unet_region_auc_append(d, d, None, 1, 0, d, 64, d, None) == -1
    assert lib.unet_region_auc(d, 4, d, 4, 1, 4, 0.3, None, d, 1 << 20, None) == -1
    assert lib.unet_region_auc(None, 4, d, 4, 1, 4, 0.3, d, d, 1 << 20, None) == -1
    for limit in (0.0, -0.1, 1.5, float("nan")):
        assert lib.unet_region_auc(d, 4, d, 4, 1, 4, limit, d, d, 1 << 20, None) == -1
    assert lib.unet_region_auc(d, 4, d, 4, 5, 4, 0.3, d, d, 1 << 20, None) == -1     # more regions than pixels
    assert lib.unet_region_auc(d, 1 << 30, d, 1 << 30, 1, 4, 0.3, d, d, 1 << 40, None) == -2
    assert b"2^31" in lib.unet_last_error()
    assert lib.unet_region_auc(d, 4, d, 4, 1, 4, 0.3, d, d, 16, None) == -3


def _results(with_pro, regions=3):
    rng = np.random.default_rng(3)
    labels = np.array([0, 1, 1, 0, 1, 0])
    masks = (rng.random((6, 1, 16, 16)) < 0.2).astype(np.float32) * labels[:, None, None, None]
    amaps = np.clip(rng.random((6, 1, 16, 16)) * 0.7 + 0.3 * masks, 0, 1).astype(np.float32)
    res = {"labels": labels, "predictions": labels.copy(), "image_scores": rng.random(6), "anomaly_maps": amaps,
           "masks_true": masks, "anomaly_types": ["good", "x", "x", "good", "y", "good"]}
    if with_pro:
        res["pixel_pro"] = {"aupro": 0.625, "pro_at_limit": 0.75, "fpr_limit": 0.3, "regions": regions, "defective": 40,
                            "ok": 1496 if regions else 1536, "nonfinite": 0}
    return res


def test_evaluate_results_adds_region_metrics_only_with_regions():
    pytest.importorskip("sklearn.metrics")
    from tiaozhanbei_unet_amd.test import evaluate_results
    plain = evaluate_results(_results(False), [0.3, 0.5, 0.7])
    assert list(plain) == ["image_metrics", "pixel_metrics", "type_metrics"]
    with_pro = evaluate_results(_results(True), [0.3, 0.5, 0.7])
    assert with_pro["region_metrics"] == {"aupro": 0.625, "pro_at_limit": 0.75, "fpr_limit": 0.3, "regions": 3}
    assert {k: v for k, v in with_pro.items() if k != "region_metrics"} == plain
    for entry in with_pro["pixel_metrics"].values():
        assert list(entry) == ["accuracy", "precision", "recall", "specificity", "f1_score", "auroc", "auprc"]
    assert evaluate_results(_results(True, regions=0), [0.3, 0.5, 0.7]) == plain
    no_ok = _results(True)
    no_ok["pixel_pro"]["ok"] = 0
    assert evaluate_results(no_ok, [0.3, 0.5, 0.7]) == plain


def test_cli_flags():
    from tiaozhanbei_unet_amd import test as test_cli
    a = test_cli.parse_args(["--checkpoint", "x.pth"])
    assert a.pro_fpr_limit == 0.3 and a.binary_masks is False
    b = test_cli.parse_args(["--checkpoint", "x.pth", "--pro_fpr_limit", "1.0", "--binary_masks"])
    assert b.pro_fpr_limit == 1.0 and b.binary_masks is True
    names = [n for n, _ in test_cli.FLAGS]
    assert names.index("--pro_fpr_limit") > names.index("--precision") < names.index("--binary_masks")
    for bad in ("0", "-0.3", "1.5", "nan"):
        with pytest.raises(SystemExit, match="pro_fpr_limit"):
            test_cli.parse_args(["--checkpoint", "x.pth", "--pro_fpr_limit", bad])
