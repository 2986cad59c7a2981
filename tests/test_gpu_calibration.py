"""GPU tests of confidence calibration (csrc/calibration.hip through ops.seg_confidence(temperature=), ops.CalibrationMeter
and the C entries) against tests/_calibration_ref.py -- labels byte for byte, the scaled confidence and the swept NLL within
float64 bounds whose terms are written out, the histogram exactly -- of TiledPredictor.blended_logits, and of the
eval_calibration CLI end to end.  The float cases print their figures as `REF64 segconf_t` / `REF64 tsweep` lines (-s).
Shapes and inputs are those of tests/test_gpu_segvis.py: scalar and 16-byte paths, more than one block, exact ties, +-80."""
import argparse
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import _calibration_ref as CR
import _ref64 as R64
import _segvis_ref as S
import test_gpu_segvis as TS
from tiaozhanbei_unet_amd import _lib as L
from tiaozhanbei_unet_amd import eval_calibration, eval_detection, ops, seg_calibration as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
N = TS.N_CONF                                            # 3
SHAPES = TS.CONF_SHAPES                                  # (7, 13), (33, 65), (1, 1), (16, 20)
IGNORE = 255
VP = ctypes.c_void_p


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ scaled confidence
def _scaled_through_c(zd, inv_t):
    n, c, h, w = zd.shape
    labels = torch.empty((n, h, w), dtype=torch.uint8, device=DEV)
    conf = torch.empty((n, h, w), dtype=torch.float32, device=DEV)
    L.check(L.lib().unet_seg_confidence_scaled(VP(zd.data_ptr()), n, c, h * w, float(inv_t), VP(labels.data_ptr()),
                                               VP(conf.data_ptr()), None), "unet_seg_confidence_scaled")
    return labels, conf


@pytest.mark.parametrize("kind, c, h, w", TS.CONF_CASES, ids=[f"{k}-c{c}-{h}x{w}" for k, c, h, w in TS.CONF_CASES])
def test_scaled_confidence_against_float64(kind, c, h, w):
    z = TS._logits(kind, c, h, w)
    zd = _dev(z)
    want_labels = S.labels64(z)                          # float64 argmax of the RAW logits, the first maximum
    plain_l, plain_c = ops.seg_confidence(zd)
    for t in (0.25, 1.0, 3.0):
        labels, conf = ops.seg_confidence(zd, temperature=t)
        assert labels.dtype == torch.uint8 and conf.dtype == torch.float32
        assert tuple(labels.shape) == (N, h, w) == tuple(conf.shape)
        assert np.array_equal(labels.cpu().numpy(), want_labels), t
        inv_t = CR.inv_t32(t)
        cl, cc = _scaled_through_c(zd, inv_t)
        assert torch.equal(cl, labels) and torch.equal(cc, conf)
        if t == 1.0:                                     # the existing call, and the scaled kernel at inv_t == 1: its bytes
            assert torch.equal(labels, plain_l) and torch.equal(conf, plain_c)
            continue
        ref = torch.from_numpy(CR.conf_scaled64(z, inv_t))
        host = torch.from_numpy(CR.conf_scaled32(z, inv_t))
        what = f"segconf_t {kind} c{c} {h}x{w} T={t}"
        worst = R64.assert_measured(conf, (ref, ref), host, what, extra=CR.conf_scaled_derived(c))
        host_rel, kernel_rel, allowed = R64.MEASURED[what]
        print(f"REF64 {what}: host err {host_rel / U:.2f} u, kernel err {kernel_rel / U:.2f} u, allowed {allowed / U:.2f} u "
              f"(derived {CR.conf_scaled_derived(c) / U:.2f} u), worst err / bound {worst:.3f}")
        only_l, none_c = ops.seg_confidence(zd, conf=False, temperature=t)
        none_l, only_c = ops.seg_confidence(zd, labels=False, temperature=t)
        assert none_c is None and none_l is None and torch.equal(only_l, labels) and torch.equal(only_c, conf)
    if kind == "pm80":                                   # one class 160 above the others: conf = 1 at every temperature
        assert float(ops.seg_confidence(zd, temperature=0.25)[1][0, 0, 0]) == 1.0
        inv_t = CR.inv_t32(0.25)
        ref, host = torch.from_numpy(CR.conf_scaled64(z, inv_t)), torch.from_numpy(CR.conf_scaled32(z, inv_t))
        with pytest.raises(AssertionError):
            R64.assert_measured(torch.from_numpy(CR.conf_scaled32(z, inv_t, subtract_max=False)), (ref, ref), host,
                                "planted: no max subtraction", extra=CR.conf_scaled_derived(c))


def test_scaled_confidence_refusals():
    z = torch.zeros((2, 3, 8, 8), device=DEV)
    for c in (1, 9):
        with pytest.raises(RuntimeError, match="2..8 classes"):
            ops.seg_confidence(torch.zeros((2, c, 8, 8), device=DEV), temperature=2.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.seg_confidence(z, temperature=bad)


# ------------------------------------------------------------------------------------------------ histogram
def _planted_conf(rng, shape, bins):
    """random confidences with, at the front, 0, 1, every k / bins with its fp32 neighbours, -0.5, 1.5 and NaN"""
    conf = rng.random(shape).astype(np.float32)
    edges = np.arange(bins + 1, dtype=np.float64) / bins
    e32 = edges.astype(np.float32)
    special = np.concatenate([[0.0, 1.0, -0.5, 1.5, np.nan], e32, np.nextafter(e32, np.float32(-1)),
                              np.nextafter(e32, np.float32(2))]).astype(np.float32)
    flat = conf.reshape(-1)
    k = min(len(special), flat.size)
    flat[:k] = special[:k]
    return conf


def _planted_maps(rng, shape, c):
    """targets with IGNORE, -1 and c planted, labels with values >= c planted, at the far end from the special confidences"""
    target = rng.integers(0, c, shape).astype(np.int64)
    labels = rng.integers(0, c, shape).astype(np.uint8)
    target[rng.random(shape) < 0.5] = 0                  # background-heavy, so that select = 1 leaves pixels out
    labels[rng.random(shape) < 0.5] = 0
    tf, lf = target.reshape(-1), labels.reshape(-1)
    if tf.size >= 8:
        tf[-3:] = (IGNORE, -1, c)
        lf[-6:-3] = (c, 255, c)
    return target, labels


def _hist_through_c(labels, conf, target, c, bins, select, hist=None):
    n, h, w = labels.shape
    if hist is None:
        hist = torch.zeros(c * bins * 3 + 1, dtype=torch.int64, device=DEV)
    L.check(L.lib().unet_reliability_histogram(VP(labels.data_ptr()), VP(conf.data_ptr()), VP(target.data_ptr()), n, h * w, c,
                                               bins, IGNORE, select, VP(hist.data_ptr()), VP(hist[c * bins * 3:].data_ptr()),
                                               None), "unet_reliability_histogram")
    return hist


@pytest.mark.parametrize("bins", [1, 10, 15, 64])
@pytest.mark.parametrize("c", [2, 4, 8])
def test_histogram_equals_the_restatement_exactly(c, bins):
    for h, w in SHAPES:
        rng = np.random.default_rng(c * 1000 + bins * 10 + h)
        conf = _planted_conf(rng, (N, h, w), bins)
        target, labels = _planted_maps(rng, (N, h, w), c)
        ld, cd, td = _dev(labels), _dev(conf), _dev(target)
        for select in (0, 1):
            what = f"c{c} bins{bins} {h}x{w} select{select}"
            want, want_skipped = CR.histogram(labels, conf, target, c, bins, IGNORE, select)
            got = _hist_through_c(ld, cd, td, c, bins, select).cpu().numpy()
            assert np.array_equal(got[:-1].reshape(c, bins, 3), want), what
            assert got[-1] == want_skipped, what
            if h * w >= 8:
                taken = int(want[:, :, 0].sum())
                assert want_skipped == 6 and (taken == N * h * w - 6 if select == 0 else 0 < taken < N * h * w - 6)
            meter = ops.CalibrationMeter(c, bins=bins, ignore_index=IGNORE, select=("all", "defects")[select])
            meter.update_confidence(ld, cd, td)
            res = meter.compute()
            assert np.array_equal(res["hist"], want) and res["skipped"] == want_skipped, what
            assert res["counted"] == 0 and res["nonfinite"] == 0 and res["nll"].tolist() == [0.0]


def test_histogram_sums_above_32_bits_accumulates_and_repeats():
    n, h, w, c, bins = 2, 300, 300, 4, 15
    labels = torch.full((n, h, w), 2, dtype=torch.uint8, device=DEV)
    conf = torch.ones((n, h, w), dtype=torch.float32, device=DEV)
    target = torch.full((n, h, w), 2, dtype=torch.int64, device=DEV)
    got = _hist_through_c(labels, conf, target, c, bins, 0).cpu().numpy()
    want = np.zeros((c, bins, 3), np.int64)
    want[2, bins - 1] = (n * h * w, n * h * w, n * h * w * 65536)
    assert want[2, bins - 1, 2] == 11796480000 > 2 ** 32
    assert np.array_equal(got[:-1].reshape(c, bins, 3), want) and got[-1] == 0
    # two updates accumulate; two fresh runs are equal
    rng = np.random.default_rng(7)
    conf2 = _planted_conf(rng, (N, 33, 65), bins)
    target2, labels2 = _planted_maps(rng, (N, 33, 65), c)
    ld, cd, td = _dev(labels2), _dev(conf2), _dev(target2)
    one, skipped = CR.histogram(labels2, conf2, target2, c, bins, IGNORE, 0)
    acc = _hist_through_c(labels, conf, target, c, bins, 0)
    acc = _hist_through_c(ld, cd, td, c, bins, 0, hist=acc).cpu().numpy()
    assert np.array_equal(acc[:-1].reshape(c, bins, 3), want + one) and acc[-1] == skipped
    first = _hist_through_c(ld, cd, td, c, bins, 0)
    again = _hist_through_c(ld, cd, td, c, bins, 0)
    assert torch.equal(first, again) and np.array_equal(first.cpu().numpy()[:-1].reshape(c, bins, 3), one)


# ------------------------------------------------------------------------------------------------ sweep
def _temperatures(k):
    return [0.7] if k == 1 else SC.temperature_grid(0.25, 4.0, k)


def _sweep_inputs(kind, c, h, w):
    z = TS._logits(kind, c, h, w).copy()
    rng = np.random.default_rng(c * 100 + h)
    target, _ = _planted_maps(rng, (N, h, w), c)
    if h * w >= 8 and kind == "normal":                  # the last image carries a NaN and an Inf logit
        z[N - 1, 0, 0, 1], z[N - 1, c - 1, h - 1, 0] = np.nan, np.inf
    return z, target


def _check_sweep(z, target, c, k, select, what):
    temps = _temperatures(k)
    inv_t = [CR.inv_t32(t) for t in temps]
    meter = ops.CalibrationMeter(c, temperatures=temps, ignore_index=IGNORE, select=("all", "defects")[select])
    meter.update(_dev(z), _dev(target))
    res = meter.compute()
    nll, scale, counted, nonfinite = CR.sweep64(z, target, IGNORE, select, inv_t)
    assert (res["counted"], res["nonfinite"]) == (counted, nonfinite), what
    host = CR.sweep32(z, target, IGNORE, select, inv_t)
    ref = (torch.from_numpy(nll), torch.from_numpy(scale))
    worst = R64.assert_measured(torch.from_numpy(res["nll"]), ref, torch.from_numpy(host), what, extra=R64.SUM_EPS)
    host_rel, kernel_rel, allowed = R64.MEASURED[what]
    print(f"REF64 {what}: pixels {counted}, host err {host_rel / U:.2f} u, kernel err {kernel_rel / U:.2f} u, allowed "
          f"{allowed / U:.2f} u of S, worst err / bound {worst:.3f}")
    again = ops.CalibrationMeter(c, temperatures=temps, ignore_index=IGNORE, select=("all", "defects")[select])
    again.update(_dev(z), _dev(target))
    assert again.compute()["nll"].tobytes() == res["nll"].tobytes(), what      # two runs: the same bits
    return res, ref, host


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("c", [2, 4, 8])
def test_sweep_against_float64(c, k):
    for h, w in SHAPES:
        z, target = _sweep_inputs("normal", c, h, w)
        for select in (0, 1):
            res, _, _ = _check_sweep(z, target, c, k, select, f"tsweep c{c} K{k} {h}x{w} select{select}")
            if h * w >= 8:
                assert res["nonfinite"] == 2 and 0 < res["counted"] < N * h * w


@pytest.mark.parametrize("h, w", [(33, 65), (16, 20)])
def test_sweep_pm80_at_a_quarter_stays_finite(h, w):
    z, target = _sweep_inputs("pm80", 4, h, w)
    target[0, 0, 0] = 1                                  # class 0 at +80, the target 160 below: a term of 640
    res, ref, host = _check_sweep(z, target, 4, 5, 0, f"tsweep pm80 c4 K5 {h}x{w}")
    assert np.isfinite(res["nll"]).all() and res["nll"][0] >= 640.0
    assert ref[0][0] >= 640.0                            # T = 0.25 is the grid's first point
    # teeth: the restatement without its max subtraction does not pass the same bound
    planted = CR.sweep32(z, target, IGNORE, 0, [CR.inv_t32(t) for t in _temperatures(5)], subtract_max=False)
    with pytest.raises(AssertionError):
        R64.assert_measured(torch.from_numpy(planted), ref, torch.from_numpy(host), "planted: no max subtraction",
                            extra=R64.SUM_EPS)


def test_sweep_bits_do_not_depend_on_the_loads_and_accumulate():
    """hw % 4 == 0: 16-byte loads; the same logits at an address that is no multiple of 16 take the scalar loads to the
    same bits.  A second call adds to nll and counted."""
    c, h, w, k = 4, 16, 20, 5
    z, target = _sweep_inputs("normal", c, h, w)
    inv = (ctypes.c_float * k)(*[float(CR.inv_t32(t)) for t in _temperatures(k)])
    td = _dev(target)
    flat = torch.zeros(z.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = _dev(z).reshape(-1)
    lib = L.lib()
    nbytes = lib.unet_temperature_sweep_workspace(N, h * w, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def run(logits, out=None):
        out = torch.zeros(k + 2, dtype=torch.float64, device=DEV) if out is None else out
        L.check(lib.unet_temperature_sweep(VP(logits.data_ptr()), VP(td.data_ptr()), N, c, h * w, IGNORE, 0, inv, k,
                                           VP(out.data_ptr()), VP(out[k:].data_ptr()), VP(ws.data_ptr()), nbytes, None),
                "unet_temperature_sweep")
        return out

    vec, scalar = run(_dev(z)), run(flat[1:])
    assert flat[1:].data_ptr() % 16 != 0 and torch.equal(vec, scalar)
    counts = vec[k:].view(torch.int64).tolist()
    nll, _, counted, nonfinite = CR.sweep64(z, target, IGNORE, 0, list(inv))
    assert counts == [counted, nonfinite]
    twice = run(_dev(z), out=vec.clone())
    assert twice[k:].view(torch.int64).tolist() == [2 * counted, 2 * nonfinite]
    assert torch.equal(twice[:k], vec[:k] + vec[:k])


# ------------------------------------------------------------------------------------------------ a planted temperature
@pytest.mark.parametrize("seed", range(6))
def test_planted_temperature_is_recovered(seed):
    rng = np.random.default_rng(seed)
    z = (2 * rng.standard_normal((2, 4, 64, 64))).astype(np.float32)
    p = torch.softmax(torch.from_numpy(z).double(), 1).numpy()
    target = (rng.random((2, 64, 64))[:, None] > np.cumsum(p, 1)).sum(1).clip(0, 3)      # inverse CDF of softmax(z)
    logits = (np.float32(3) * z).astype(np.float32)
    grid = SC.temperature_grid(0.25, 4.0, 32)
    ld, td = _dev(logits), _dev(target)
    first = ops.CalibrationMeter(4, bins=15, temperatures=grid)
    first.update(ld, td)
    before = first.compute()
    fit = SC.fit_temperature(grid, before["nll"])
    second = ops.CalibrationMeter(4, bins=15, temperatures=[fit["value"]], temperature=fit["value"])
    second.update(ld, td)
    after = second.compute()
    ece_before = SC.reliability(before["hist"].sum(0))["ece"]
    ece_after = SC.reliability(after["hist"].sum(0))["ece"]
    nll_1 = ops.CalibrationMeter(4, temperatures=[1.0])
    nll_1.update(ld, td)
    nll_at_1 = nll_1.compute()["nll"][0]
    assert before["counted"] == after["counted"] == 2 * 64 * 64
    assert not fit["at_edge"] and 2.8 <= fit["value"] <= 3.25
    assert ece_after < ece_before / 4
    assert after["nll"][0] < nll_at_1

    # against the restatement's fit.  With equal steps h in log T the vertex is x1 + (h / 2) A / B, A = y0 - y2, B = y0 - 2 y1
    # + y2 > 0.  The sweep may be off by d = max_k allowed_k S_k on each y (the bound of test_sweep_against_float64), so A
    # moves by at most 2 d and B by at most 4 d: |dx| <= (h / 2) (2 d B + 4 d |A|) / (B (B - 4 d)), and T by expm1 of that.
    inv_grid = [CR.inv_t32(t) for t in grid]
    nll, scale, _, _ = CR.sweep64(logits, target, IGNORE, 0, inv_grid)
    host = CR.sweep32(logits, target, IGNORE, 0, inv_grid)
    want = SC.fit_temperature(grid, nll)
    i = want["index"]
    assert fit["index"] == i
    allowed = [(max(4 * abs(host[k] - nll[k]) / scale[k], R64.MEASURED_FLOOR) + R64.SUM_EPS) * scale[k] for k in (i - 1, i, i + 1)]
    d = max(allowed)
    a, b = nll[i - 1] - nll[i + 1], nll[i - 1] - 2 * nll[i] + nll[i + 1]
    assert b > 4 * d
    step = math.log(grid[i + 1] / grid[i])
    bound = math.expm1(0.5 * step * (2 * d * b + 4 * d * abs(a)) / (b * (b - 4 * d)))
    rel = abs(fit["value"] - want["value"]) / want["value"]
    print(f"REF64 tfit seed {seed}: T {fit['value']:.6f} restatement {want['value']:.6f} relative difference {rel:.3e} "
          f"bound {bound:.3e}; ECE {ece_before:.4f} -> {ece_after:.4f}; NLL/pixel {nll_at_1 / 8192:.4f} -> "
          f"{after['nll'][0] / 8192:.4f}")
    assert rel <= bound


# ------------------------------------------------------------------------------------------------ tiled
def test_blended_logits_give_the_predictors_labels_and_confidence():
    from tiaozhanbei_unet_amd import SegmentationUNet
    from tiaozhanbei_unet_amd.tiling import TiledPredictor
    torch.manual_seed(3)
    model = SegmentationUNet(3, 4, precision="fp32").to(DEV)
    predictor = TiledPredictor(model, (32, 32), min_overlap=8, batch_size=4)
    frame = torch.randn((3, 70, 90), device=DEV)
    labels, conf, plan = predictor(frame)
    logits, plan2 = predictor.blended_logits(frame)
    assert plan == plan2 and len(plan["origins_y"]) > 1 and len(plan["origins_x"]) > 1
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (4, 70, 90)
    got_l, got_c = ops.seg_confidence(logits.unsqueeze(0))
    assert torch.equal(got_l[0], labels) and torch.equal(got_c[0], conf)


# ------------------------------------------------------------------------------------------------ CLI
RESULT_KEYS = {"evaluation_args", "class_names", "mode", "pixels", "skipped", "nonfinite", "temperature", "before", "after"}
GROUP_KEYS = {"pixels", "accuracy", "mean_confidence", "confidence_minus_accuracy", "ece", "mce", "bins"}


def _checkpoint_of_one_epoch(module, save, *argv):
    exp = module.main(["--epochs", "1", "--val_freq", "1", "--save_freq", "1", "--batch_size", "4", "--num_workers", "0",
                       "--save_dir", str(save), *argv])
    ckpt = os.path.join(exp, "checkpoints", "checkpoint_epoch_0.pth")
    assert os.path.exists(ckpt)
    return ckpt


def _check_results(save, mode, class_names, pixels, bins=15, steps=32):
    res = json.load(open(save / "calibration_results.json"))
    assert set(res) == RESULT_KEYS
    assert res["mode"] == mode and res["class_names"] == class_names and res["nonfinite"] == 0
    assert res["pixels"] + res["skipped"] == pixels
    t = res["temperature"]
    assert {"value", "at_edge", "grid", "nll_per_pixel"} <= set(t)
    assert len(t["grid"]) == len(t["nll_per_pixel"]) == steps and t["grid"][0] <= t["value"] <= t["grid"][-1]
    assert all(math.isfinite(v) and v >= 0 for v in t["nll_per_pixel"] + [t["nll_at_value"]])
    for part in ("before", "after"):
        assert set(res[part]) == {"overall", "defects", "per_class"} and list(res[part]["per_class"]) == class_names
        groups = [res[part]["overall"], res[part]["defects"]] + list(res[part]["per_class"].values())
        for g in groups:
            assert set(g) == GROUP_KEYS and len(g["bins"]) == bins
            assert sum(b["count"] for b in g["bins"]) == g["pixels"]
            assert 0.0 <= g["ece"] <= g["mce"] + 1e-12 and g["mce"] <= 1.0
        assert res[part]["overall"]["pixels"] == res["pixels"]
        assert sum(g["pixels"] for g in res[part]["per_class"].values()) == res["pixels"]
        assert sum(g["pixels"] for g in list(res[part]["per_class"].values())[1:]) == res[part]["defects"]["pixels"]
    assert res["after"]["overall"]["accuracy"] == res["before"]["overall"]["accuracy"]      # the labels do not move
    return res


def _round_trip(tmp_path, common, mode, class_names, pixels, model_args):
    """eval_calibration --save_calibrated, then eval_calibration on the calibrated checkpoint: the second fit is 1 to
    within a grid step (unless the first sat on an edge of the range), and its `before` is the first run's `after`"""
    from tiaozhanbei_unet_amd.train_gear import build_seg_model
    from tiaozhanbei_unet_amd.utils import load_checkpoint
    out = tmp_path / f"calibrated_{mode}.pth"
    eval_calibration.main(common + ["--save_dir", str(tmp_path / mode), "--save_calibrated", str(out)])
    res = _check_results(tmp_path / mode, mode, class_names, pixels)
    saved = torch.load(out, map_location="cpu", weights_only=True)
    assert saved["temperature"] == res["temperature"]["value"] and set(saved["calibration"]) == {"overall", "defects", "per_class"}
    model = build_seg_model(model_args, len(class_names), torch.device(DEV))
    load_checkpoint(model, None, str(out), torch.device(DEV))
    again = [a if a != common[common.index("--checkpoint") + 1] else str(out) for a in common]
    eval_calibration.main(again + ["--save_dir", str(tmp_path / (mode + "_again"))])
    res2 = _check_results(tmp_path / (mode + "_again"), mode, class_names, pixels)
    ratio = res["temperature"]["resolution"]
    diff = abs(res2["before"]["overall"]["ece"] - res["after"]["overall"]["ece"])
    print(f"calibration round trip ({mode}): T {res['temperature']['value']:.4f} (at_edge {res['temperature']['at_edge']}), "
          f"then {res2['temperature']['value']:.4f}; ECE {res['before']['overall']['ece']:.4f} -> "
          f"{res['after']['overall']['ece']:.4f}, the calibrated checkpoint's own {res2['before']['overall']['ece']:.4f} "
          f"(difference {diff:.2e})")
    if not res["temperature"]["at_edge"]:
        assert 1.0 / ratio <= res2["temperature"]["value"] <= ratio
    return out


MODEL_ARGS = argparse.Namespace(model="seg_unet", bilinear=False, dropout=0.1, precision="fp32")


@pytest.fixture(scope="module")
def gear_run(tmp_path_factory):
    """a synthetic Gear tree and a checkpoint of one epoch on it, shared by the frame and the tiled case (never modified)"""
    from tiaozhanbei_unet_amd import gear_dataset as G
    from tiaozhanbei_unet_amd import train_gear
    base = tmp_path_factory.mktemp("gear_calibration")
    root = G.write_synthetic_gear(str(base / "gear"))
    ckpt = _checkpoint_of_one_epoch(train_gear, base / "runs", "--data_root", root, "--image_size", "64")
    ds = G.GearDataset(root, "test", (64, 64), raw=True)
    _images, _polys, sizes, _paths = G.collate_raw([ds[i] for i in range(len(ds))])
    common = ["--dataset", "gear", "--checkpoint", ckpt, "--data_root", root, "--image_size", "64", "--batch_size", "3",
              "--num_workers", "0"]
    return {"root": root, "common": common, "names": ["background"] + list(ds.class_names), "images": len(ds),
            "sizes": [(int(h), int(w)) for h, w in sizes]}


# a model of one epoch is far from calibrated, either way: the frame cases search 0.01 .. 4 (a grid ratio of 1.21), so that
# the fit has a chance to be interior and the second run's temperature is held to 1
WIDE = ["--temperature_range", "0.01", "4"]


def test_eval_calibration_cli_gear_frame(gear_run, tmp_path, capsys):
    g = gear_run
    capsys.readouterr()
    calibrated = _round_trip(tmp_path, g["common"] + WIDE, "frame", g["names"], g["images"] * 64 * 64, MODEL_ARGS)
    text = capsys.readouterr().out
    assert "Fitted temperature" in text and "ECE" in text
    print(text[text.index("calibration round trip"):].splitlines()[0])
    # an existing CLI takes the calibrated checkpoint as it is
    eval_detection.main(["--dataset", "gear", "--checkpoint", str(calibrated), "--data_root", g["root"], "--image_size", "64",
                         "--batch_size", "3", "--num_workers", "0", "--save_dir", str(tmp_path / "det")])
    assert json.load(open(tmp_path / "det" / "detection_results.json"))["images"] == g["images"]


def test_eval_calibration_cli_gear_tiled(gear_run, tmp_path):
    g = gear_run
    assert len(set(g["sizes"])) > 1                      # every image at its own size
    res_dir = _round_trip(tmp_path, g["common"] + ["--tiled", "--tile", "64", "64", "--min_overlap", "8"], "tiled", g["names"],
                          sum(h * w for h, w in g["sizes"]), MODEL_ARGS)
    assert os.path.exists(res_dir)


def test_eval_calibration_cli_kolektorsdd(tmp_path):
    from tiaozhanbei_unet_amd import kolektorsdd_dataset as K
    from tiaozhanbei_unet_amd import train_kolektorsdd
    root = K.write_synthetic_kolektorsdd(str(tmp_path / "kol"), n_folders=6, per_folder=5)
    ckpt = _checkpoint_of_one_epoch(train_kolektorsdd, tmp_path / "runs", "--data_root", root, "--image_height", "64",
                                    "--image_width", "32")
    ds = K.KolektorSDDDataset(root, "test", (64, 32), raw=True)
    common = ["--dataset", "kolektorsdd", "--checkpoint", ckpt, "--data_root", root, "--image_height", "64", "--image_width",
              "32", "--batch_size", "2", "--num_workers", "0"]
    calibrated = _round_trip(tmp_path, common + WIDE, "frame", list(K.CLASS_NAMES), len(ds) * 64 * 32, MODEL_ARGS)
    eval_detection.main(["--dataset", "kolektorsdd", "--checkpoint", str(calibrated), "--data_root", root, "--image_height",
                         "64", "--image_width", "32", "--batch_size", "2", "--num_workers", "0", "--save_dir",
                         str(tmp_path / "det")])
    assert json.load(open(tmp_path / "det" / "detection_results.json"))["images"] == len(ds)
    with pytest.raises(SystemExit):
        eval_calibration.main(["--dataset", "kolektorsdd", "--checkpoint", ckpt, "--tiled"])
