"""Confidence calibration without a GPU: seg_calibration's host arithmetic (ECE, MCE, pooling, the temperature grid and
fit, the fold of 1 / T into a checkpoint's head) on hand-written inputs, the numpy restatement tests/_calibration_ref.py
that tests/test_gpu_calibration.py holds the device to, the flags of the eval_calibration CLI, and the C entries'
refusals ahead of any HIP call."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _calibration_ref as CR
from tiaozhanbei_unet_amd import eval_calibration, eval_regions, seg_calibration as SC

Q = 65536


# ------------------------------------------------------------------------------------------------ reliability
def _hist(rows):
    """[(count, correct, confidence as a fraction of 65536 per pixel)] -> [bins, 3]"""
    return np.array([[n, k, n * q] for n, k, q in rows], np.int64)


def test_ece_mce_on_a_hand_written_histogram():
    # 4 bins; bin 0 empty, bin 1: 10 pixels, 4 right, confidence 0.375; bin 2 empty; bin 3: 30 pixels, 27 right, 0.875
    r = SC.reliability(_hist([(0, 0, 0), (10, 4, Q * 3 // 8), (0, 0, 0), (30, 27, Q * 7 // 8)]))
    assert r["pixels"] == 40
    assert [b["count"] for b in r["bins"]] == [0, 10, 0, 30]
    assert [(b["lo"], b["hi"]) for b in r["bins"]] == [(0.0, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0)]
    empty = r["bins"][0]
    assert (empty["accuracy"], empty["confidence"], empty["gap"]) == (0.0, 0.0, 0.0)
    assert r["bins"][1]["accuracy"] == 0.4 and r["bins"][1]["confidence"] == 0.375
    assert r["bins"][1]["gap"] == pytest.approx(-0.025, abs=1e-15)           # underconfident
    assert r["bins"][3]["accuracy"] == 0.9 and r["bins"][3]["gap"] == pytest.approx(-0.025, abs=1e-15)
    assert r["ece"] == pytest.approx(0.25 * 0.025 + 0.75 * 0.025, abs=1e-15)
    assert r["mce"] == pytest.approx(0.025, abs=1e-15)
    assert r["accuracy"] == 31 / 40
    assert r["mean_confidence"] == pytest.approx((10 * 0.375 + 30 * 0.875) / 40, abs=1e-15)
    assert r["confidence_minus_accuracy"] == pytest.approx(r["mean_confidence"] - 31 / 40, abs=1e-15)
    # overconfident: the sign turns, ECE weighs by the bin's share, MCE takes the worst bin
    r = SC.reliability(_hist([(20, 10, Q // 8), (0, 0, 0), (0, 0, 0), (60, 30, Q)]))
    assert r["bins"][0]["gap"] == pytest.approx(0.125 - 0.5) and r["bins"][3]["gap"] == pytest.approx(0.5)
    assert r["ece"] == pytest.approx(0.25 * 0.375 + 0.75 * 0.5) and r["mce"] == pytest.approx(0.5)
    assert r["confidence_minus_accuracy"] > 0
    # nothing at all: zeros, never NaN
    r = SC.reliability(np.zeros((15, 3), np.int64))
    assert r["pixels"] == 0 and r["ece"] == 0.0 and r["mce"] == 0.0 and r["confidence_minus_accuracy"] == 0.0
    assert all(math.isfinite(v) for b in r["bins"] for v in b.values())
    one = SC.reliability(_hist([(7, 7, Q)]))                                   # one bin
    assert one["ece"] == 0.0 and one["bins"][0]["lo"] == 0.0 and one["bins"][0]["hi"] == 1.0


def test_per_class_pooling_with_an_empty_class():
    names = ["background", "pitting", "spalling", "scrape"]
    h = np.zeros((4, 2, 3), np.int64)
    h[0] = _hist([(0, 0, 0), (10000, 9990, Q)])                                  # background swamps everything
    h[1] = _hist([(10, 2, Q // 4), (10, 6, Q * 3 // 4)])
    h[3] = _hist([(0, 0, 0), (20, 10, Q)])                                     # class 2 is never predicted
    s = SC.calibration_summary(h, names)
    assert list(s["per_class"]) == names and set(s) == {"overall", "defects", "per_class"}
    assert s["per_class"]["spalling"]["pixels"] == 0 and s["per_class"]["spalling"]["ece"] == 0.0
    assert s["overall"]["pixels"] == 10040 and s["defects"]["pixels"] == 40
    d = s["defects"]                                                           # classes 1..3 pooled bin by bin
    assert [b["count"] for b in d["bins"]] == [10, 30]
    assert d["bins"][1]["accuracy"] == 16 / 30
    assert d["bins"][1]["confidence"] == pytest.approx((10 * 0.75 + 20 * 1.0) / 30)
    assert d["ece"] == pytest.approx(0.25 * abs(0.25 - 0.2) + 0.75 * abs((10 * 0.75 + 20) / 30 - 16 / 30))
    assert s["overall"]["ece"] < 0.02 < d["ece"]                               # what the pooling is for
    assert s["per_class"]["scrape"]["mce"] == pytest.approx(0.5)
    with pytest.raises(ValueError):
        SC.calibration_summary(h, names[:3])


# ------------------------------------------------------------------------------------------------ temperature
def test_temperature_grid():
    g = SC.temperature_grid(0.25, 4.0, 32)
    assert len(g) == 32 and g[0] == 0.25 and g[-1] == 4.0
    ratios = [b / a for a, b in zip(g, g[1:])]
    assert max(ratios) - min(ratios) < 1e-12 and ratios[0] == pytest.approx(16 ** (1 / 31))
    assert SC.temperature_grid(1.0, 4.0, 3) == [1.0, 2.0, 4.0]
    for bad in ((0.0, 4.0, 8), (2.0, 2.0, 8), (4.0, 2.0, 8), (-1.0, 2.0, 8), (1.0, float("inf"), 8), (1.0, 2.0, 1)):
        with pytest.raises(ValueError):
            SC.temperature_grid(*bad)


@pytest.mark.parametrize("t_star", [0.3, 1.0, 2.9, 3.05, 3.7])
def test_fit_recovers_the_vertex_of_an_exact_parabola(t_star):
    grid = SC.temperature_grid(0.25, 4.0, 32)
    nll = [5.0 + 3.0 * (math.log(t) - math.log(t_star)) ** 2 for t in grid]
    fit = SC.fit_temperature(grid, nll)
    assert not fit["at_edge"] and 0 < fit["index"] < 31
    assert fit["value"] == pytest.approx(t_star, rel=1e-9)
    assert fit["resolution"] == pytest.approx(16 ** (1 / 31))


def test_fit_reports_the_edges_and_clamps():
    grid = SC.temperature_grid(0.25, 4.0, 8)
    up = SC.fit_temperature(grid, [float(i) for i in range(8)])                # decreasing towards LO
    assert up == {"value": 0.25, "at_edge": True, "index": 0, "resolution": pytest.approx(16 ** (1 / 7))}
    down = SC.fit_temperature(grid, [float(-i) for i in range(8)])
    assert down["value"] == 4.0 and down["at_edge"] and down["index"] == 7
    # a parabola whose vertex lies outside the range: still an edge
    assert SC.fit_temperature(grid, [(math.log(t) - math.log(9.0)) ** 2 for t in grid])["at_edge"]
    # three collinear points at the (first) minimum: the grid point; a kinked minimum stays between its neighbours
    flat = SC.fit_temperature(grid, [3.0, 1.0, 1.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    assert flat["index"] == 1 and not flat["at_edge"] and grid[0] <= flat["value"] <= grid[2]
    kink = SC.fit_temperature(grid, [9.0, 8.0, 1.0, 1.0 + 1e-9, 9.0, 9.0, 9.0, 9.0])
    assert kink["index"] == 2 and grid[1] <= kink["value"] <= grid[3]
    one = SC.fit_temperature([2.0], [1.0])
    assert one["value"] == 2.0 and one["at_edge"]
    for bad in (([1.0, 2.0], [1.0]), ([2.0, 1.0], [1.0, 2.0]), ([1.0, 2.0], [1.0, float("nan")]), ([0.0, 1.0], [1.0, 2.0])):
        with pytest.raises(ValueError):
            SC.fit_temperature(*bad)


# ------------------------------------------------------------------------------------------------ checkpoint
def test_calibrated_checkpoint_on_a_hand_made_state_dict():
    g = torch.Generator().manual_seed(0)
    state = {"inc.double_conv.0.weight": torch.randn(8, 3, 3, 3, generator=g),
             "inc.double_conv.1.running_mean": torch.randn(8, generator=g),
             "inc.double_conv.1.num_batches_tracked": torch.tensor(7),
             "outc.conv.weight": torch.randn(4, 8, 1, 1, generator=g), "outc.conv.bias": torch.randn(4, generator=g)}
    ckpt = {"epoch": 3, "model_state_dict": state, "optimizer_state_dict": {"state": {}, "param_groups": []}, "loss": 0.5}
    t = 2.75
    out = SC.calibrated_checkpoint(ckpt, t, {"overall": {"ece": 0.01}})
    assert set(out) == set(ckpt) | {"temperature", "calibration"}
    assert out["temperature"] == t and out["calibration"] == {"overall": {"ece": 0.01}}
    assert out["epoch"] == 3 and out["loss"] == 0.5 and out["optimizer_state_dict"] is ckpt["optimizer_state_dict"]
    new = out["model_state_dict"]
    assert list(new) == list(state)
    for k in SC.HEAD_KEYS:
        want = (state[k].double() / t).float()
        assert new[k].dtype == torch.float32 and torch.equal(new[k], want) and not torch.equal(new[k], state[k])
        assert float((new[k].double() * t - state[k].double()).abs().max()) <= 2.0 ** -24 * t * float(state[k].abs().max())
    for k in state:
        if k not in SC.HEAD_KEYS:
            assert new[k].dtype == state[k].dtype and new[k].numpy().tobytes() == state[k].numpy().tobytes(), k
    assert torch.equal(ckpt["model_state_dict"]["outc.conv.weight"], state["outc.conv.weight"])      # the input is intact
    # a bf16 head is divided in float64 and cast back to bf16
    half = dict(state, **{k: state[k].bfloat16() for k in SC.HEAD_KEYS})
    folded = SC.fold_temperature(half, t)
    assert folded["outc.conv.weight"].dtype == torch.bfloat16
    assert torch.equal(folded["outc.conv.weight"], (half["outc.conv.weight"].double() / t).bfloat16())
    assert SC.fold_temperature(state, 1.0)["outc.conv.bias"].numpy().tobytes() == state["outc.conv.bias"].numpy().tobytes()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            SC.fold_temperature(state, bad)
    with pytest.raises(KeyError):
        SC.fold_temperature({"outc_seg.conv.weight": state["outc.conv.weight"]}, 2.0)


def test_calibrated_checkpoint_survives_torch_save_and_weights_only_load(tmp_path):
    state = {"outc.conv.weight": torch.ones(2, 4, 1, 1), "outc.conv.bias": torch.zeros(2)}
    ckpt = {"epoch": 0, "model_state_dict": state, "optimizer_state_dict": {}, "loss": 0.0}
    summary = SC.calibration_summary(np.ones((2, 3, 3), np.int64), ["a", "b"])
    torch.save(SC.calibrated_checkpoint(ckpt, 2.0, summary), tmp_path / "c.pth")
    back = torch.load(tmp_path / "c.pth", map_location="cpu", weights_only=True)       # what utils.load_checkpoint does
    assert back["temperature"] == 2.0 and back["calibration"] == summary
    assert torch.equal(back["model_state_dict"]["outc.conv.weight"], torch.full((2, 4, 1, 1), 0.5))


# ------------------------------------------------------------------------------------------------ CLI
def test_flag_defaults_and_refusals(capsys):
    base = ["--checkpoint", "m.pth"]
    args = eval_calibration.parse_args(["--dataset", "gear"] + base)
    assert (args.bins, args.temperature_range, args.temperature_steps, args.fit_on, args.save_calibrated) == \
        (15, [0.25, 4.0], 32, "all", None)
    assert (args.tiled, args.tile, args.min_overlap, args.split, args.precision) == (False, [512, 512], 64, "test", "fp32")
    args = eval_calibration.parse_args(["--dataset", "kolektorsdd"] + base)
    assert args.tile == [1024, 512] and not args.tiled and args.bins == 15
    args = eval_calibration.parse_args(["--dataset", "gear"] + base + [
        "--tiled", "--tile", "64", "96", "--min_overlap", "8", "--bins", "64", "--temperature_range", "0.5", "8",
        "--temperature_steps", "3", "--fit_on", "defects", "--save_calibrated", "out.pth", "--split", "val"])
    assert (args.tiled, args.tile, args.min_overlap, args.bins, args.temperature_range, args.temperature_steps) == \
        (True, [64, 96], 8, 64, [0.5, 8.0], 3)
    assert (args.fit_on, args.save_calibrated, args.split) == ("defects", "out.pth", "val")
    for dataset in eval_regions.DATASETS:
        names = [n for n, _ in eval_calibration.flags_of(dataset)]
        shared = [n for n, _ in eval_regions.flags_of(dataset) if n not in ("--min_region_pixels", "--coverage_thresholds")]
        assert names == shared + ["--tiled", "--tile", "--min_overlap", "--bins", "--temperature_range",
                                  "--temperature_steps", "--fit_on", "--save_calibrated"]
    for dataset in eval_regions.DATASETS:
        for bad in (["--bins", "0"], ["--bins", "65"], ["--temperature_range", "0", "4"], ["--temperature_range", "2", "2"],
                    ["--temperature_range", "4", "0.25"], ["--temperature_range", "-1", "2"], ["--temperature_steps", "2"],
                    ["--temperature_steps", "33"], ["--fit_on", "background"], ["--min_overlap", "-1"],
                    ["--tile", "0", "64"]):
            with pytest.raises(SystemExit):
                eval_calibration.parse_args(["--dataset", dataset] + base + bad)
    with pytest.raises(SystemExit):
        eval_calibration.parse_args(["--dataset", "gear"] + base + ["--tiled", "--tile", "64", "64", "--min_overlap", "64"])
    with pytest.raises(SystemExit):
        eval_calibration.parse_args(["--dataset", "gear"])                     # --checkpoint is required
    capsys.readouterr()
    with pytest.raises(SystemExit):
        eval_calibration.parse_args(["--dataset", "kolektorsdd"] + base + ["--tiled"])
    assert "full-resolution" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        eval_calibration.main(["--dataset", "gear", "--device", "cpu"] + base)
    assert "no CPU path" in str(e.value)


def test_help_carries_the_three_cautions(capsys):
    with pytest.raises(SystemExit):
        eval_calibration.parse_args(["--dataset", "gear", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "never on the split you report" in text and "head's rounding" in text and "has not been measured" in text


# ------------------------------------------------------------------------------------------------ library
def test_library_exports_the_calibration_entry_points():
    from tiaozhanbei_unet_amd import _lib, ops
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in ("unet_seg_confidence_scaled", "unet_reliability_histogram", "unet_temperature_sweep",
                 "unet_temperature_sweep_workspace"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name
    assert ops.CalibrationMeter.__module__ == "tiaozhanbei_unet_amd.evaluation"
    assert hasattr(ops.seg_confidence, "__call__")


def test_bad_arguments_are_refused_on_the_host():
    """decided before any HIP call: the status -2, not a launch (the pointers are never followed)"""
    from tiaozhanbei_unet_amd import _lib
    lib = _lib.lib()
    p, null = ctypes.c_void_p(256), None
    inv = (ctypes.c_float * 33)(*([1.0] * 33))
    assert lib.unet_temperature_sweep_workspace(2, 64, 5) > 0

    def conf(logits=p, n=2, c=4, hw=64, inv_t=1.0, labels=p, cf=p):
        return lib.unet_seg_confidence_scaled(logits, n, c, hw, inv_t, labels, cf, None)

    def hist(labels=p, cf=p, target=p, n=2, hw=64, c=4, bins=15, select=0, out=p, skipped=p):
        return lib.unet_reliability_histogram(labels, cf, target, n, hw, c, bins, 255, select, out, skipped, None)

    def sweep(logits=p, target=p, n=2, c=4, hw=64, select=0, inv_t=inv, k=5, nll=p, counted=p, ws=p, nbytes=1 << 20):
        return lib.unet_temperature_sweep(logits, target, n, c, hw, 255, select, inv_t, k, nll, counted, ws, nbytes, None)

    for c in (1, 9):
        assert conf(c=c) == -2 and hist(c=c) == -2 and sweep(c=c) == -2, c
        assert b"2..8 classes" in lib.unet_last_error()
    for bins in (0, 65):
        assert hist(bins=bins) == -2, bins
        assert b"1..64 bins" in lib.unet_last_error()
    for k in (0, 33):
        assert sweep(k=k) == -2, k
        assert lib.unet_temperature_sweep_workspace(2, 64, k) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert conf(inv_t=bad) == -2, bad
        assert b"inv_t" in lib.unet_last_error()
        one = (ctypes.c_float * 3)(1.0, bad, 1.0)
        assert sweep(inv_t=one, k=3) == -2, bad
        assert b"inv_t[1]" in lib.unet_last_error()
    assert conf(logits=null) == -2 and conf(labels=null, cf=null) == -2
    for name in ("labels", "cf", "target", "out", "skipped"):
        assert hist(**{name: null}) == -2, name
    for name in ("logits", "target", "inv_t", "nll", "counted", "ws"):
        assert sweep(**{name: null}) == -2, name
    assert b"null pointer" in lib.unet_last_error()
    for kw in (dict(n=0), dict(hw=0)):
        assert conf(**kw) == -2 and hist(**kw) == -2 and sweep(**kw) == -2, kw
    assert hist(select=2) == -2 and sweep(select=-1) == -2 and sweep(n=65536) == -2
    assert sweep(nbytes=8) == -3                        # too small a workspace is its own status


def test_python_surface_validates_before_the_library(monkeypatch):
    from tiaozhanbei_unet_amd import _lib, ops
    from tiaozhanbei_unet_amd.sheets import inverse_temperature

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    assert inverse_temperature(4.0) == 0.25 and inverse_temperature(3.0) == float(np.float32(1.0 / 3.0))
    for bad in (0.0, -2.0, float("nan"), float("inf"), 1e-40, 1e46):
        with pytest.raises(ValueError):
            inverse_temperature(bad)
    for kw in (dict(num_classes=1), dict(num_classes=9), dict(bins=0), dict(bins=65), dict(temperatures=()),
               dict(temperatures=[1.0] * 33), dict(temperatures=[1.0, 0.0]), dict(temperature=-1.0), dict(select="background")):
        with pytest.raises(ValueError):
            ops.CalibrationMeter(**{"num_classes": 4, **kw})
    meter = ops.CalibrationMeter(4, bins=10, temperatures=(0.5, 1.0, 2.0))
    empty = meter.compute()
    assert empty["hist"].shape == (4, 10, 3) and not empty["hist"].any() and empty["nll"].tolist() == [0.0, 0.0, 0.0]
    assert (empty["skipped"], empty["counted"], empty["nonfinite"]) == (0, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meter.update(torch.zeros((1, 4, 2, 2)), torch.zeros((1, 2, 2), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_confidence(torch.zeros((1, 4, 2, 2)), temperature=2.0)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_histogram_on_planted_pixels():
    bins, c = 10, 4
    conf = np.array([0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), -0.5, 1.5, np.nan, 0.95, 0.95, 0.3],
                    np.float32)
    labels = np.array([0, 1, 1, 1, 2, 2, 3, 1, 0, 7], np.uint8)
    target = np.array([0, 1, 2, 1, 2, 2, 3, 255, -1, 0], np.int64)
    assert CR.quantise(conf).tolist() == [0, Q, Q // 2, Q // 2, 0, Q, 0, 62259, 62259, 19661]
    hist, skipped = CR.histogram(labels, conf, target, c, bins, 255, 0)
    assert skipped == 3                                                        # target 255, target -1, label 7
    assert hist[0, 0].tolist() == [1, 1, 0]                                    # conf 0 -> bin 0
    assert hist[1, 9].tolist() == [1, 1, Q]                                    # conf 1 -> the last bin, not bin `bins`
    assert hist[1, 5].tolist() == [2, 1, Q]                                    # 0.5 and its lower neighbour: q ties to even
    assert hist[2, 0].tolist() == [1, 1, 0] and hist[2, 9].tolist() == [1, 1, Q]      # -0.5 and 1.5 clamp
    assert hist[3, 0].tolist() == [1, 1, 0]                                    # NaN -> 0
    assert int(hist[:, :, 0].sum()) == 7
    only, skipped1 = CR.histogram(labels, conf, target, c, bins, 255, 1)
    assert skipped1 == 3 and int(only[:, :, 0].sum()) == 6 and not only[0].any()      # the background pixel is left out
    one_bin, _ = CR.histogram(labels, conf, target, c, 1, 255, 0)
    assert one_bin[:, 0, 0].tolist() == [1, 3, 2, 1]
    # the bin of k / bins is k: q = rint(65536 k / bins) and (q * bins) >> 16 never falls below k
    for b in (10, 15, 64):
        for k in range(b):
            q = int(CR.quantise(np.float32(k / b)))
            assert min(b - 1, (q * b) >> 16) in (k - 1, k), (b, k)             # (fp32 k / b may round below k / b)


def test_restatement_sweep_and_its_planted_defect():
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((2, 4, 5, 6)) * 3).astype(np.float32)
    t = rng.integers(0, 4, (2, 5, 6))
    t[0, 0, :3] = (255, -1, 4)
    inv_t = [CR.inv_t32(v) for v in (0.25, 1.0, 3.0)]
    nll, scale, counted, nonfinite = CR.sweep64(z, t, 255, 0, inv_t)
    assert counted == 57 and nonfinite == 0
    keep = (t >= 0) & (t < 4)
    lp = torch.log_softmax(torch.from_numpy(z).double(), 1).numpy()
    want = -np.take_along_axis(lp, np.clip(t, 0, 3)[:, None], 1)[:, 0][keep].sum()
    assert nll[1] == pytest.approx(want, rel=1e-12) and (scale >= nll).all()
    host = CR.sweep32(z, t, 255, 0, inv_t)
    assert np.abs(host - nll).max() <= 2.0 ** -20 * scale.max()
    z[1, 2, 0, 0], z[1, 0, 1, 1] = np.nan, np.inf
    _, _, counted, nonfinite = CR.sweep64(z, t, 255, 0, inv_t)
    assert (counted, nonfinite) == (55, 2)
    _, _, defects, _ = CR.sweep64(z, t, 255, 1, inv_t)
    assert defects < counted
    big = np.where(rng.random((1, 4, 4, 4)) < 0.5, 80.0, -80.0).astype(np.float32)
    big[0, :, 0, 0] = (80.0, -80.0, -80.0, -80.0)
    tb = np.zeros((1, 4, 4), np.int64)
    tb[0, 0, 0] = 1                                                            # the target 160 below the maximum
    nll, scale, _, _ = CR.sweep64(big, tb, 255, 0, [CR.inv_t32(0.25)])
    assert nll[0] >= 640.0 and np.isfinite(CR.sweep32(big, tb, 255, 0, [CR.inv_t32(0.25)])).all()
    assert not np.isfinite(CR.sweep32(big, tb, 255, 0, [CR.inv_t32(0.25)], subtract_max=False)).all()
    # the scaled confidence: at inv_t = 1 the plain one, bit for bit on the host too
    import _segvis_ref as S
    assert np.array_equal(CR.conf_scaled32(z[:1], np.float32(1.0)), S.conf32(z[:1]))
    assert np.abs(CR.conf_scaled64(z[:1], inv_t[2]) -
                  torch.softmax(torch.from_numpy(z[:1]).double() * float(inv_t[2]), 1).max(1)[0].numpy()).max() <= 1e-15
    assert CR.conf_scaled_derived(4) == pytest.approx((8 * np.exp(-1.0) + 4) * CR.U)


def test_restatement_recovers_the_planted_temperature():
    """the issue's recipe on the host: T between 3.00 and 3.08, ECE 0.19-0.21 before against 0.009-0.017 after"""
    grid = SC.temperature_grid(0.25, 4.0, 32)
    inv_grid = [CR.inv_t32(t) for t in grid]
    for seed in (0, 5):
        rng = np.random.default_rng(seed)
        z = (2 * rng.standard_normal((2, 4, 64, 64))).astype(np.float32)
        p = torch.softmax(torch.from_numpy(z).double(), 1).numpy()
        target = (rng.random((2, 64, 64))[:, None] > np.cumsum(p, 1)).sum(1).clip(0, 3)
        logits = (np.float32(3) * z).astype(np.float32)
        nll, _, counted, _ = CR.sweep64(logits, target, 255, 0, inv_grid)
        fit = SC.fit_temperature(grid, nll)
        assert counted == 2 * 64 * 64 and not fit["at_edge"] and 3.0 <= fit["value"] <= 3.08
        labels = np.argmax(logits, 1)
        ece = []
        for t in (1.0, fit["value"]):
            conf = CR.conf_scaled64(logits, CR.inv_t32(t)).astype(np.float32)
            ece.append(SC.reliability(CR.histogram(labels, conf, target, 4, 15, 255, 0)[0].sum(0))["ece"])
        assert 0.19 <= ece[0] <= 0.21 and 0.009 <= ece[1] <= 0.017
