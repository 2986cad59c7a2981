"""CPU checks of the view ensembling: the tap table of tests/_views_ref.py against exact rational arithmetic (and the two
32-bit divisions csrc/views.hip forms it with against the table), the reference merge on hand cases, the export and
host-side refusals of unet_view_merge, views.plan_views, and the flags and refusals of the predict_views / eval_views
CLIs."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _views_ref as VR
from tiaozhanbei_unet_amd import _lib, eval_detection, eval_views, ops, predict_tiled, predict_views, views

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = [(5, 3), (3, 5), (9, 18), (7, 1), (1, 7), (16384, 8192)]            # (N outputs, M view samples)


# ------------------------------------------------------------------------------------------------ the tap table
@pytest.mark.parametrize("n, m", AXES, ids=[f"{n}from{m}" for n, m in AXES])
def test_taps_against_exact_rational_arithmetic(n, m):
    """before the clamp p / 65536 lies in (x - 2^-16, x] for x = (i + 1/2) M / N - 1/2; after it 0 <= i0 <= i1 <= M - 1"""
    ulp = Fraction(1, 65536)
    for i in range(n):
        x = (Fraction(2 * i + 1, 2) * m) / n - Fraction(1, 2)
        p = Fraction(VR.raw_tap(i, n, m), 65536)
        assert x - ulp < p <= x, (i, n, m)
    i0, i1, f = VR.taps(n, m)
    assert (0 <= i0).all() and (i0 <= i1).all() and (i1 <= m - 1).all() and (i1 - i0 <= 1).all()
    assert (0 <= f).all() and (f <= 0xFFFF).all()
    assert (f[i1 == i0] == 0).all() and (i0[i1 == i0] == m - 1).all()      # no second tap: only on the last sample, clamped
    r0, r1, rf = VR.taps(n, m, flip=True)
    assert np.array_equal(r0, m - 1 - i0) and np.array_equal(r1, m - 1 - i1) and np.array_equal(rf, f)


def test_an_axis_of_the_frames_own_length_has_no_fractions():
    for n in (1, 2, 7, 64, 1000, 16384):
        i0, i1, f = VR.taps(n, n)
        assert np.array_equal(i0, np.arange(n)) and not f.any()
        assert np.array_equal(i1, np.minimum(np.arange(n) + 1, n - 1))
        # the formula itself says the same: M == N is no exception to it
        assert all(VR.raw_tap(i, n, n) == i << 16 for i in (0, n // 2, n - 1))


def test_known_taps():
    # 2 -> 4 samples: centres at -0.25, 0.25, 0.75, 1.25, the ends clamped
    i0, i1, f = VR.taps(4, 2)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and f.tolist() == [0, 16384, 49152, 0]
    # 4 -> 2: centres at 0.5 and 2.5
    i0, i1, f = VR.taps(2, 4)
    assert i0.tolist() == [0, 2] and i1.tolist() == [1, 3] and f.tolist() == [32768, 32768]
    i0, i1, f = VR.taps(7, 1)
    assert not i0.any() and not i1.any() and not f.any()


def _device_floor(i, n, m):
    """csrc/views.hip's tap_divide in Python: two divisions whose operands stay below 2^32"""
    t = (2 * i + 1) * m
    assert t < 1 << 29
    q, r = divmod(t, n)
    s = r << 15
    assert s < 1 << 29 and q << 15 < 1 << 31
    q2, rem = divmod(s, n)
    return (q << 15) + q2, rem


@pytest.mark.parametrize("n, m", AXES + [(16384, 16384), (1, 16384), (16384, 1), (16383, 16384), (1920, 1440), (1080, 1620)])
def test_the_kernels_two_divisions_and_its_steps_give_the_same_taps(n, m):
    step_q, step_r = divmod(m << 16, n)
    assert step_q < 1 << 31
    big, rem = _device_floor(0, n, m)
    for i in range(n):
        assert (big, rem) == _device_floor(i, n, m) and big - 32768 == VR.raw_tap(i, n, m), (i, n, m)
        assert big + step_q + 1 < 1 << 32                               # the step past the last pixel stays in 32 bits
        big, rem = big + step_q, rem + step_r                           # the 4-pixel lanes step instead of dividing
        if rem >= n:
            big, rem = big + 1, rem - n


# ------------------------------------------------------------------------------------------------ the reference merge
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _logits(c, h, w, seed):
    return (np.random.default_rng(seed).standard_normal((c, h, w)) * 4.0).astype(np.float32)


def test_one_view_of_the_frames_size_returns_its_bits():
    z = _logits(3, 5, 7, 0)
    z[0, 0, 0], z[1, 2, 3] = -0.0, np.float32(1e-42)                   # a copy keeps a signed zero and a denormal
    merged, labels, agreement = VR.merge([z], [(0, 0)], (5, 7))
    assert np.array_equal(_bits(merged), _bits(z))
    assert np.array_equal(labels, np.argmax(z, axis=0)) and (agreement == 1).all() and agreement.dtype == np.uint8
    labels2, conf, agreement2, merged2 = VR.predict([z], [(0, 0)], (5, 7))
    assert np.array_equal(labels2, labels) and np.array_equal(merged2, merged) and conf.dtype == np.float32
    assert conf.shape == (5, 7) and float(conf.min()) >= 1 / 3 - 1e-6 and float(conf.max()) <= 1.0


def test_two_equal_views_return_the_same_bits():
    z = _logits(4, 6, 5, 1)
    merged, labels, agreement = VR.merge([z, z.copy()], [(0, 0), (0, 0)], (6, 5))
    assert np.array_equal(_bits(merged), _bits(z)) and (agreement == 2).all()       # (a + a) / 2 is exact
    four, _, agreement = VR.merge([z] * 4, [(0, 0)] * 4, (6, 5))
    assert np.array_equal(_bits(four), _bits(z)) and (agreement == 4).all()


def test_a_mirrored_view_flagged_as_such_returns_the_firsts_bits():
    z = _logits(3, 6, 8, 2)
    for (fx, fy), mirrored in (((1, 0), z[:, :, ::-1]), ((0, 1), z[:, ::-1]), ((1, 1), z[:, ::-1, ::-1])):
        merged, labels, agreement = VR.merge([z, mirrored], [(0, 0), (fx, fy)], (6, 8))
        assert np.array_equal(_bits(merged), _bits(z)), (fx, fy)
        assert (agreement == 2).all()
        assert np.array_equal(_bits(VR.view_value(mirrored, (6, 8), fx, fy)), _bits(z))
    # interpolated views mirror back too: the view of the mirrored image, flagged, is the mirror of the plain view's value
    small = _logits(3, 4, 5, 3)
    plain = VR.view_value(small, (7, 9))
    assert np.array_equal(_bits(VR.view_value(small[:, :, ::-1], (7, 9), True, False)), _bits(plain))
    assert np.array_equal(_bits(VR.view_value(small[:, ::-1], (7, 9), False, True)), _bits(plain))
    # without the flag it is not
    assert not np.array_equal(VR.view_value(small[:, :, ::-1], (7, 9)), plain)


def test_a_one_pixel_view_is_constant_over_the_frame():
    z = np.array([[[1.5]], [[-2.25]], [[0.75]]], np.float32)
    val = VR.view_value(z, (4, 6))
    assert val.shape == (3, 4, 6) and (val == z).all()
    merged, labels, agreement = VR.merge([_logits(3, 4, 6, 4), z], [(0, 0), (1, 1)], (4, 6))
    assert np.array_equal(merged, ((_logits(3, 4, 6, 4) + z) / np.float32(2)).astype(np.float32))


def test_an_exact_tie_of_the_first_and_the_last_class_resolves_to_the_first():
    for c in (2, 3, 8):
        z = _logits(c, 4, 4, c)
        z[0] = z[c - 1] = z.max(axis=0) + np.float32(1.0)
        small = z[:, ::2, ::2].copy()
        merged, labels, agreement = VR.merge([z, small], [(0, 0), (0, 0)], (4, 4))
        assert np.array_equal(_bits(merged[0]), _bits(merged[c - 1])) and (merged[0] == merged.max(axis=0)).all()
        assert (labels == 0).all() and (agreement == 2).all()


def test_interpolated_values_round_every_operation_once():
    """2 x 2 -> 4 x 4 by hand at the pixel (1, 2): fy = 16384 (0.25), fx = 49152 (0.75)"""
    z = np.array([[[0.1, 0.7], [1.3, -2.9]]], np.float32)
    f = np.float32
    q = f(2.0 ** -16)
    top = f(f(f(16384) * z[0, 0, 0]) + f(f(49152) * z[0, 0, 1])) * q
    bot = f(f(f(16384) * z[0, 1, 0]) + f(f(49152) * z[0, 1, 1])) * q
    want = f(f(f(49152) * f(top)) + f(f(16384) * f(bot))) * q
    assert VR.view_value(z, (4, 4))[0, 1, 2] == f(want)
    assert abs(float(want) - (0.75 * (0.25 * 0.1 + 0.75 * 0.7) + 0.25 * (0.25 * 1.3 + 0.75 * -2.9))) < 1e-6


# ------------------------------------------------------------------------------------------------ exports, refusals
def test_the_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    makefile = open(os.path.join(ROOT, "tiaozhanbei_unet_amd", "csrc", "Makefile")).read()
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    assert re.search(r"\bunet_view_merge\(", header) and "typedef struct unet_merge_view" in header
    assert "unet_view_merge" in _lib.SIGNATURES and len(_lib.SIGNATURES["unet_view_merge"][1]) == 10
    assert hasattr(handle, "unet_view_merge") and not hasattr(handle, "unet_view_merge_workspace")
    handle.unet_abi_version.restype = ctypes.c_int32
    assert handle.unet_abi_version() == 1
    assert " views.hip" in makefile
    for obj in ("build/views.o", "build/stamps/views.o"):      # what make would run; the diagnostic build too
        line = subprocess.run(["make", "-C", _lib.CSRC, "-n", "-B", obj], capture_output=True, text=True, check=True).stdout
        assert re.search(rf" -ffp-contract=off .*-c views\.hip -o {obj}\n", line), line
    assert ctypes.sizeof(_lib.MergeView) == 24
    for name in ("plan_views", "merge_views", "ViewEnsemble"):
        assert hasattr(views, name) and not hasattr(ops, name), name


def _descs(*items):
    return (_lib.MergeView * len(items))(*[_lib.MergeView(*it) for it in items])


def test_refusals_are_decided_on_the_host():
    """dummy device pointers: every call below is refused before anything could read them"""
    lib = _lib.lib()
    dummy = ctypes.c_void_p(16)
    good = (16, 7, 9, 0, 0)

    def merge(views=None, nv=None, c=3, h=7, w=9, merged=dummy, labels=dummy, conf=dummy, agreement=dummy, null=False):
        items = [good] if views is None else views
        return lib.unet_view_merge(None if null else _descs(*items), len(items) if nv is None else nv, c, h, w, merged,
                                   labels, conf, agreement, None)

    assert merge(null=True) == -2 and b"null view array" in lib.unet_last_error()
    assert merge(views=[good, (0, 7, 9, 0, 0)]) == -2 and b"view 1 has a null pointer" in lib.unet_last_error()
    for nv in (0, 17, -1):
        assert merge(views=[good] * 17, nv=nv) == -2 and b"views (1..16)" in lib.unet_last_error(), nv
    for c in (1, 9, 0, -2):
        assert merge(c=c) == -2 and b"2..8 classes" in lib.unet_last_error(), c
    for kw in (dict(h=0), dict(w=0), dict(h=16385), dict(w=16385), dict(h=-7)):
        assert merge(**kw) == -2 and b"a frame of" in lib.unet_last_error(), kw
    for hv, wv in ((0, 9), (7, 0), (16385, 9), (7, 16385), (-1, 9)):
        assert merge(views=[good, (16, hv, wv, 0, 0)]) == -2 and b"view 1 of" in lib.unet_last_error(), (hv, wv)
    assert merge(merged=None, labels=None, conf=None, agreement=None) == -2 and b"every output is null" in lib.unet_last_error()
    for fx, fy in ((2, 0), (0, 2), (-1, 0), (0, -1), (256, 1)):
        assert merge(views=[(16, 7, 9, fx, fy)]) == -2 and b"flips" in lib.unet_last_error(), (fx, fy)


def test_the_wrapper_checks_shapes_and_dtypes_before_the_device():
    torch = pytest.importorskip("torch")
    z = torch.zeros((3, 7, 9))
    for bad in (z[0], z.double(), "logits"):
        with pytest.raises(ValueError, match="float32"):
            views.merge_views([bad], [(0, 0)], (7, 9))
    with pytest.raises(ValueError, match="0 views"):
        views.merge_views([], [], (7, 9))
    with pytest.raises(ValueError, match="17 views"):
        views.merge_views([z] * 17, [(0, 0)] * 17, (7, 9))
    with pytest.raises(ValueError, match="pairs"):
        views.merge_views([z, z], [(0, 0)], (7, 9))
    with pytest.raises(ValueError, match="classes"):
        views.merge_views([z, torch.zeros((4, 7, 9))], [(0, 0), (1, 0)], (7, 9))
    with pytest.raises(ValueError, match="switched off"):
        views.merge_views([z], [(0, 0)], (7, 9), labels=False, conf=False, agreement=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        views.merge_views([z], [(0, 0)], (7, 9))
    with pytest.raises(ValueError):
        views.ViewEnsemble(None, [])
    with pytest.raises(ValueError, match="uint8"):
        views.ViewEnsemble(None, [(1.0, 0, 0)]).view_logits(torch.zeros((7, 9, 3)), (7, 9))


# ------------------------------------------------------------------------------------------------ the plan of views
def test_plan_views_order_duplicates_and_refusals():
    assert views.plan_views([1], "none") == [(1.0, 0, 0)]
    assert views.plan_views([1], "h") == [(1.0, 0, 0), (1.0, 1, 0)]
    assert views.plan_views([1], "v") == [(1.0, 0, 0), (1.0, 0, 1)]
    assert views.plan_views([1], "all") == [(1.0, 0, 0), (1.0, 1, 0), (1.0, 0, 1), (1.0, 1, 1)]
    assert views.plan_views([0.75, 1, 1.5], "h") == [(0.75, 0, 0), (0.75, 1, 0), (1.0, 0, 0), (1.0, 1, 0), (1.5, 0, 0),
                                                      (1.5, 1, 0)]
    assert views.plan_views([2, 0.5, 2.0, 0.5], "v") == [(2.0, 0, 0), (2.0, 0, 1), (0.5, 0, 0), (0.5, 0, 1)]      # duplicates go
    for scales, flips in (([0.75, 1, 1.5], "h"), ([1], "all"), ([2, 0.5, 2.0], "v"), ([0.5, 0.6, 0.7, 0.8], "all")):
        got = views.plan_views(scales, flips)
        assert got == VR.plan_views(scales, flips)
        assert all(type(s) is float and type(fx) is int and type(fy) is int for s, fx, fy in got)
    assert len(views.plan_views([0.5, 0.6, 0.7, 0.8], "all")) == 16
    with pytest.raises(ValueError, match="at most 16"):
        views.plan_views([0.5, 0.6, 0.7, 0.8, 0.9], "all")
    for bad in (0.49, 2.01, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            views.plan_views([1, bad], "h")
    with pytest.raises(ValueError, match="flips"):
        views.plan_views([1], "both")
    with pytest.raises(ValueError, match="no scale"):
        views.plan_views([], "h")


# ------------------------------------------------------------------------------------------------ CLI flags
BASE = ["--task", "gear", "--checkpoint", "c.pth", "--input", "photos"]
EVAL = ["--dataset", "gear", "--checkpoint", "c.pth"]


def test_predict_views_flags():
    got = vars(predict_views.parse_args(BASE))
    tiled = vars(predict_tiled.parse_args(BASE))
    assert set(got) == set(tiled) | {"view_scales", "view_flips", "views"}
    assert all(got[k] == tiled[k] for k in tiled)      # predict_tiled's flags and defaults
    assert (got["view_scales"], got["view_flips"], got["views"]) == ([1.0], "h", [(1.0, 0, 0), (1.0, 1, 0)])
    assert [name for name, _ in predict_views.FLAGS] == [name for name, _ in predict_tiled.FLAGS] + ["--view_scales",
                                                                                                      "--view_flips"]
    own = vars(predict_views.parse_args(BASE + ["--view_scales", "0.75", "1", "1.5", "--view_flips", "all", "--scale", "2",
                                                "--tile", "64", "32", "--min_overlap", "8"]))
    assert own["view_scales"] == [0.75, 1.0, 1.5] and len(own["views"]) == 12 and own["views"][4] == (1.0, 0, 0)
    assert (own["scale"], own["tile"], own["min_overlap"]) == (2.0, [64, 32], 8)
    assert vars(predict_views.parse_args(BASE + ["--scale", "2", "--view_scales", "2"]))["views"][0] == (2.0, 0, 0)   # 4 is inside
    none = vars(predict_views.parse_args(BASE + ["--view_flips", "none"]))
    assert none["views"] == [(1.0, 0, 0)]


@pytest.mark.parametrize("extra", [["--view_scales", "0.4"], ["--view_scales", "1", "2.5"], ["--view_scales"],
                                   ["--scale", "2.5", "--view_scales", "2"], ["--scale", "4", "--view_scales", "1", "1.25"],
                                   ["--view_scales", "0.5", "0.6", "0.7", "0.8", "0.9", "--view_flips", "all"],
                                   ["--view_flips", "both"], ["--scale", "0"], ["--min_overlap", "512"],
                                   ["--image_size", "64", "64"], ["--batch_size", "0"]])
def test_predict_views_refuses(extra):
    with pytest.raises(SystemExit):
        predict_views.parse_args(BASE + extra)


def test_eval_views_flags():
    got = vars(eval_views.parse_args(EVAL))
    det = vars(eval_detection.parse_args(EVAL + ["--tiled"]))
    assert set(got) == set(det) | {"view_scales", "view_flips", "views"}
    assert all(got[k] == det[k] for k in det)          # eval_detection --tiled's flags and defaults; tiled is implied
    assert got["tiled"] is True and got["tile"] == [512, 512] and got["min_overlap"] == 64
    assert (got["view_scales"], got["view_flips"], got["views"]) == ([1.0], "h", [(1.0, 0, 0), (1.0, 1, 0)])
    # the plain view moves to the front, the others keep their order
    own = vars(eval_views.parse_args(EVAL + ["--view_scales", "0.75", "1", "1.5", "--view_flips", "h", "--tile", "64", "64",
                                             "--min_overlap", "8", "--max_false_alarms", "0.5"]))
    assert own["views"] == [(1.0, 0, 0), (0.75, 0, 0), (0.75, 1, 0), (1.0, 1, 0), (1.5, 0, 0), (1.5, 1, 0)]
    assert (own["tile"], own["min_overlap"], own["max_false_alarms"]) == ([64, 64], 8, 0.5)


@pytest.mark.parametrize("argv", [["--dataset", "kolektorsdd", "--checkpoint", "c.pth"],
                                  EVAL + ["--view_scales", "0.75", "1.5"],            # no plain view
                                  EVAL + ["--view_scales", "1", "0.4"], EVAL + ["--view_scales", "1", "2.5"],
                                  EVAL + ["--view_scales", "1", "0.6", "0.7", "0.8", "0.9", "--view_flips", "all"],
                                  EVAL + ["--view_flips", "diag"], EVAL + ["--min_overlap", "512"],
                                  EVAL + ["--tile", "0", "64"], EVAL + ["--min_region_pixels", "0"],
                                  EVAL + ["--coverage_thresholds", "1.5"], EVAL + ["--max_false_alarms", "-1"],
                                  ["--checkpoint", "c.pth"]])
def test_eval_views_refuses(argv):
    with pytest.raises(SystemExit):
        eval_views.parse_args(argv)


def test_both_clis_refuse_the_cpu():
    with pytest.raises(SystemExit) as e:
        predict_views.main(BASE + ["--device", "cpu"])
    assert "no CPU path" in str(e.value)
    with pytest.raises(SystemExit) as e:
        eval_views.main(EVAL + ["--device", "cpu"])
    assert "no CPU path" in str(e.value)


def test_comparison_and_agreement_summary_on_hand_records():
    """two truth regions, three predicted ones: the first covers its truth region, the others touch nothing of their class"""
    def rec(image, cls, root, size, conf_q=0):
        return [image, cls, root, size, 0, 0, 0, 0, 0, 0, conf_q, conf_q]

    truth = np.array([rec(0, 1, 0, 10), rec(1, 2, 5, 4)], np.int64)
    pred = np.array([rec(0, 1, 0, 10, 10 * 65536), rec(0, 2, 40, 5, 5 * 32768), rec(1, 1, 9, 2, 2 * 16384)], np.int64)
    pairs = np.array([[0, 0, 0, 10], [1, 5, 9, 2]], np.int64)
    got = {"truth": truth, "pred": pred, "pairs": pairs}
    summary = eval_views.agreement_summary(got, np.array([1.0, 0.5, 0.25]), 0.5)
    assert summary == {"coverage_threshold": 0.5, "matched_regions": 1, "matched_mean": 1.0, "false_alarms": 2,
                       "false_alarm_mean": 0.375}
    none = eval_views.agreement_summary({"truth": truth[:0], "pred": pred[:0], "pairs": pairs[:0]}, np.zeros(0), 0.5)
    assert none["matched_mean"] is None and none["false_alarm_mean"] is None
    from tiaozhanbei_unet_amd import seg_detection
    res = seg_detection.detection_results(truth, pred, pairs, 2, 3, [0.5], ["background", "a", "b"], 0.1)
    cmp = eval_views.compare(res, res)
    assert list(cmp) == ["0.5"] and cmp["0.5"]["single"] == cmp["0.5"]["ensemble"]
    assert set(cmp["0.5"]["single"]) == {"average_precision", "recall_within_false_alarm_budget", "recall_at_best_f1",
                                         "min_confidence_within_false_alarm_budget", "min_confidence_at_best_f1",
                                         "panoptic_quality"}
    assert cmp["0.5"]["single"]["recall_at_best_f1"] == 0.5 and cmp["0.5"]["single"]["min_confidence_at_best_f1"] == 1.0
    table = eval_views.format_comparison(cmp, summary, 6)
    assert "6 views" in table and "average_precision" in table and "false alarms (2) 0.3750" in table
