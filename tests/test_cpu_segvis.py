"""The segmentation prediction sheets without a GPU: tests/_segvis_ref.py (the numpy restatement that
tests/test_gpu_segvis.py holds the device to) against matplotlib's own tables and index arithmetic, the product's
tables against the restatement, the flags of the two visualiser CLIs against the reference's (pinned as data), the
per_row geometry, and argument validation ahead of any library call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _segvis_ref as S
from conftest import ROOT

REFERENCE_VIS_COMMON = {  # reference visualize.py:20-72 and visualize_kolektorsdd.py:21-73 (--checkpoint is required)
    "split": "test", "model": "seg_unet", "bilinear": False, "dropout": 0.1, "num_samples": 10, "batch_size": 4,
    "num_workers": 4, "device": "auto", "seed": 42, "save_individual": False, "save_grid": False,
    "show_confidence": False, "figsize": [15, 5], "grid_size": [2, 5],
}
REFERENCE_GEAR_VIS_FLAGS = {"data_root": "datasets/Gear", "image_size": 512, "save_dir": None, "always_save": True,
                            **REFERENCE_VIS_COMMON}
REFERENCE_KOLEKTOR_VIS_FLAGS = {"data_root": "datasets/KolektorSDD", "image_height": 1024, "image_width": 512,
                                "save_dir": "visualizations", **REFERENCE_VIS_COMMON}


# the tab10 entry of class i under imshow(vmin=0, vmax=C-1), recorded from matplotlib 3.10.8 for every C that
# ops.class_palette accepts (C = 2, 3, 4, 8 are the issue's list), and figures of its viridis table: the anchors of
# test_tables_against_recorded_values, which needs no matplotlib
SCALED_ENTRIES_ALL = {2: [0, 9], 3: [0, 5, 9], 4: [0, 3, 6, 9], 5: [0, 2, 5, 7, 9], 6: [0, 2, 4, 6, 8, 9],
                      7: [0, 1, 3, 5, 6, 8, 9], 8: [0, 1, 2, 4, 5, 7, 8, 9], 9: [0, 1, 2, 3, 5, 6, 7, 8, 9],
                      10: [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]}
VIRIDIS_POINTS = {0: [68, 1, 84], 64: [58, 82, 139], 128: [32, 144, 140], 192: [94, 201, 97], 255: [253, 231, 36]}
VIRIDIS_CRC32 = 2310558353                  # zlib.crc32 of the 768 bytes
VIRIDIS_CHANNEL_SUMS = [21233, 34987, 27987]


# ------------------------------------------------------------------------------------------------ tables
def test_tables_against_recorded_values():
    """holds where matplotlib is missing and the three tests below skip: the restatement and the product against
    values written down here"""
    import zlib
    from tiaozhanbei_unet_amd import ops
    assert {c: SCALED_ENTRIES_ALL[c] for c in S.SCALED_ENTRIES} == S.SCALED_ENTRIES
    for c, entries in SCALED_ENTRIES_ALL.items():
        for table in (S.class_palette(c, "scaled"), ops.class_palette(c, "scaled").numpy()):
            assert table[:c].tolist() == [list(ops.TAB10[e]) for e in entries], c
            assert (table[c:] == 255).all()
        for table in (S.class_palette(c, "index"), ops.class_palette(c, "index").numpy()):
            assert table[:c].tolist() == [list(t) for t in ops.TAB10[:c]] and (table[c:] == 255).all()
    assert ops.TAB10[0] == (31, 119, 180) and ops.TAB10[9] == (23, 190, 207) and S.TAB10.tolist() == [list(t) for t in ops.TAB10]
    for table in (S.viridis_lut(), ops.viridis_lut().numpy()):
        assert table.shape == (256, 3) and table.dtype == np.uint8
        for i, rgb in VIRIDIS_POINTS.items():
            assert table[i].tolist() == rgb, i
        assert zlib.crc32(table.tobytes()) == VIRIDIS_CRC32
        assert table.astype(np.int64).sum(0).tolist() == VIRIDIS_CHANNEL_SUMS


@pytest.mark.parametrize("mode", ["index", "scaled"])
@pytest.mark.parametrize("c", [2, 3, 4, 5, 6, 7, 8, 9, 10])     # every count ops.class_palette accepts
def test_palette_equals_matplotlib_tab10(c, mode):
    pytest.importorskip("matplotlib")
    from matplotlib import colormaps
    from matplotlib.colors import Normalize
    tab10 = colormaps["tab10"]
    ids = np.arange(c)
    want = tab10(ids, bytes=True) if mode == "index" else tab10(Normalize(vmin=0, vmax=c - 1)(ids), bytes=True)
    got = S.class_palette(c, mode)
    assert got.shape == (256, 3) and got.dtype == np.uint8
    assert np.array_equal(got[:c], np.asarray(want)[:, :3])
    assert (got[c:] == 255).all()
    if mode == "scaled":
        assert [S.tab10_entry(i, c, mode) for i in range(c)] == SCALED_ENTRIES_ALL[c]
    assert np.array_equal(S.TAB10, tab10(np.arange(10), bytes=True)[:, :3])


def test_viridis_bytes_equal_matplotlib():
    pytest.importorskip("matplotlib")
    from matplotlib import colormaps
    want = colormaps["viridis"](np.arange(256), bytes=True)[:, :3]
    got = S.viridis_lut()
    assert np.array_equal(got, want)
    assert got[0].tolist() == [68, 1, 84] and got[128].tolist() == [32, 144, 140] and got[255].tolist() == [253, 231, 36]


def test_lut_index_rule_equals_matplotlib():
    pytest.importorskip("matplotlib")
    from matplotlib import colormaps
    viridis = colormaps["viridis"]
    points = np.array([0.0, 0.5, 0.999, 1.0, 3.0 / 256.0], np.float32)
    idx, drawn = S.lut_index(points)
    assert idx.tolist() == [0, 128, 255, 255, 3] and drawn.all()
    plane = np.random.default_rng(0).random((37, 53)).astype(np.float32)
    plane[0, :5] = points
    for v in (points, plane):
        assert np.array_equal(S.lut_panel(v, S.viridis_lut()), viridis(v, bytes=True)[..., :3])
    # outside the range and non-finite: under -> entry 0, over -> entry 255 (matplotlib's defaults), non-finite white
    odd = np.array([-0.5, 0.0, 1.0, 1.5, np.nan, np.inf, -np.inf], np.float32)
    idx, drawn = S.lut_index(odd)
    assert idx[:4].tolist() == [0, 0, 255, 255] and drawn.tolist() == [True] * 4 + [False] * 3
    assert np.array_equal(S.lut_panel(odd[:4], S.viridis_lut()), viridis(odd[:4], bytes=True)[..., :3])
    assert (S.lut_panel(odd[4:], S.viridis_lut()) == 255).all()


def test_product_tables_equal_the_restatement_without_matplotlib():
    from tiaozhanbei_unet_amd import ops
    for name in ("ops.py", "sheets.py", "seg_visualize.py", "visualize_gear.py", "visualize_kolektorsdd.py", "_viridis.py"):
        src = open(os.path.join(ROOT, "tiaozhanbei_unet_amd", name)).read()
        assert not re.search(r"^\s*(import|from)\s+matplotlib", src, re.M), name
    assert "matplotlib" not in open(os.path.join(ROOT, "tests", "_segvis_ref.py")).read().split('"""', 2)[2]
    for mode in ("index", "scaled"):
        for c in range(2, 11):
            got = ops.class_palette(c, mode)
            assert got.dtype == torch.uint8 and not got.is_cuda
            assert np.array_equal(got.numpy(), S.class_palette(c, mode)), (c, mode)
    assert np.array_equal(ops.viridis_lut().numpy(), S.viridis_lut())
    assert np.array_equal(np.array(ops.TAB10, np.uint8), S.TAB10)
    for bad in ((1, "index"), (11, "index"), (3, "tab20")):
        with pytest.raises(ValueError):
            ops.class_palette(*bad)


# ------------------------------------------------------------------------------------------------ CLIs
def _cli(name):
    import importlib
    return importlib.import_module(f"tiaozhanbei_unet_amd.{name}")


@pytest.mark.parametrize("name, reference", [("visualize_gear", REFERENCE_GEAR_VIS_FLAGS),
                                             ("visualize_kolektorsdd", REFERENCE_KOLEKTOR_VIS_FLAGS)])
def test_visualiser_flags_match_reference(name, reference):
    cli = _cli(name)
    args = vars(cli.parse_args(["--checkpoint", "ckpt.pth"]))
    for k, v in reference.items():
        assert args[k] == v, k
    assert set(args) - set(reference) == {"checkpoint", "precision", "synthetic"}
    assert args["precision"] == "fp32" and args["synthetic"] is False
    kw = dict(cli.FLAGS)
    assert kw["--split"]["choices"] == ["test", "val", "train"] and kw["--model"]["choices"] == ["unet", "seg_unet"]
    assert kw["--figsize"]["nargs"] == 2 and kw["--grid_size"]["nargs"] == 2
    assert "unused" in kw["--figsize"]["help"] and "native resolution" in kw["--figsize"]["help"]
    with pytest.raises(SystemExit):                    # --checkpoint is required, as in the reference
        cli.parse_args([])
    b = cli.parse_args(["--checkpoint", "c.pth", "--grid_size", "1", "3", "--figsize", "4", "4", "--split", "train",
                        "--save_grid", "--save_individual", "--show_confidence", "--synthetic", "--precision", "bf16"])
    assert b.grid_size == [1, 3] and b.split == "train" and b.save_grid and b.save_individual and b.show_confidence
    with pytest.raises(SystemExit) as e:
        cli.main(["--device", "cpu", "--checkpoint", "ckpt.pth"])
    assert "no CPU path" in str(e.value)


def test_library_exports_the_segvis_entry_points():
    from tiaozhanbei_unet_amd import _lib
    _lib.build(force=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)                # loading needs no GPU
    for name in ("unet_seg_confidence", "unet_seg_render_sheet"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES, name
    assert ctypes.sizeof(_lib.SegPanel) == 24


def test_unsupported_shapes_are_refused_on_the_host():
    """decided before anything reaches the device: the status, not a launch"""
    from tiaozhanbei_unet_amd import _lib
    lib = _lib.lib()
    dummy = ctypes.c_void_p(256)                       # only checked for NULL: the shape is refused first
    for c in (1, 9):
        assert lib.unet_seg_confidence(dummy, 2, c, 64, dummy, dummy, None) == -2, c
        assert b"2..8 classes" in lib.unet_last_error()
    panels = (_lib.SegPanel * 9)()
    three = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.unet_seg_render_sheet(dummy, panels, 9, 1, 4, 4, 0, 1, three, three, dummy, dummy, dummy, None) == -2
    assert lib.unet_seg_render_sheet(dummy, panels, 1, 65536, 4, 4, 0, 1, three, three, dummy, dummy, dummy, None) == -2
    assert lib.unet_seg_render_sheet(dummy, panels, 1, 4, 16384, 16384, 0, 1, three, three, dummy, dummy, dummy, None) == -2
    assert b"2^31" in lib.unet_last_error()
    assert lib.unet_seg_render_sheet(dummy, panels, 1, 1, 4, 4, 0, 0, three, three, dummy, dummy, dummy, None) == -1


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("n, per_row", [(1, 1), (3, 2), (5, 2), (5, 5), (3, 5), (4, 2)])
@pytest.mark.parametrize("g", [0, 4])
def test_per_row_assembly_geometry(n, per_row, g):
    h, w, c = 5, 7, 4
    rng = np.random.default_rng(n * 10 + per_row)
    images = (rng.standard_normal((n, 3, h, w)) * 1.5).astype(np.float32)
    labels = rng.integers(0, c, (n, h, w)).astype(np.uint8)
    conf = rng.random((n, h, w)).astype(np.float32)
    cols = [("image",), ("classes", labels), ("overlay", labels, 0.4), ("lut", conf)]
    palette, lut = S.class_palette(c, "scaled"), S.viridis_lut()
    sheet = S.render_seg_sheet(images, cols, gutter=g, per_row=per_row, palette=palette, lut=lut)
    rows = -(-n // per_row)
    assert sheet.shape == (rows * h + (rows - 1) * g, per_row * 4 * w + (per_row * 4 - 1) * g, 3)
    assert sheet.shape == S.sheet_shape(n, 4, h, w, g, per_row) and sheet.dtype == np.uint8
    covered = np.zeros(sheet.shape[:2], bool)
    for i in range(n):
        for j, col in enumerate(cols):
            y, x = (i // per_row) * (h + g), ((i % per_row) * 4 + j) * (w + g)
            assert np.array_equal(sheet[y:y + h, x:x + w], S.panel(col, images, i, palette, lut)), (i, j)
            covered[y:y + h, x:x + w] = True
    assert covered.sum() == n * 4 * h * w
    assert (sheet[~covered] == 255).all()              # gutters, and the cells past n in the last row
    if n % per_row:
        assert (sheet[(rows - 1) * (h + g):, (n % per_row) * 4 * (w + g):] == 255).all()
    one = S.render_seg_sheet(images[:1], cols[:1], gutter=g, per_row=per_row)
    assert one.shape == (h, per_row * w + (per_row - 1) * g, 3)


def test_panel_rules_on_planted_pixels():
    palette = S.class_palette(4, "index")
    img = np.zeros((3, 1, 4), np.float32)
    labels = np.array([[0, 1, 3, 255]], np.uint8)
    base = S.R.image_panel(img)
    over = S.overlay_panel(img, labels, 0.4, palette)
    assert S.R.alpha8(0.4) == 102
    assert np.array_equal(over[0, 0], base[0, 0])                              # nothing on the background
    for x, l in ((1, 1), (2, 3), (3, 255)):
        want = [(102 * int(palette[l][c]) + 153 * int(base[0, x, c]) + 127) // 255 for c in range(3)]
        assert over[0, x].tolist() == want
    assert np.array_equal(S.overlay_panel(img, labels, 0.0, palette), base)
    assert np.array_equal(S.overlay_panel(img, labels, 1.0, palette)[0, 1:], palette[[1, 3, 255]])
    assert np.array_equal(S.classes_panel(labels, palette)[0], palette[[0, 1, 3, 255]])
    masks = np.array([[-1, 2, 256, 255]], np.int64)                            # an int64 mask: outside 0..255 -> 255
    assert S.label_bytes(masks).tolist() == [[255, 2, 255, 255]]
    assert (S.classes_panel(masks, palette)[0, [0, 2, 3]] == 255).all()


def test_confidence_restatement_and_its_planted_defects():
    rng = np.random.default_rng(3)
    z = (rng.standard_normal((2, 4, 5, 6)) * 4).astype(np.float32)
    t = torch.from_numpy(z)
    assert np.array_equal(S.labels64(z), torch.argmax(t, 1).numpy().astype(np.uint8))
    want = torch.softmax(t.double(), 1).max(1)[0].numpy()
    assert np.abs(S.conf64(z) - want).max() <= 1e-15
    rel = np.abs(S.conf32(z).astype(np.float64) - S.conf64(z)) / S.conf64(z)
    total, terms = S.conf_bound(4, rel.max())
    assert set(terms) == {"subtraction", "additions", "division", "expf"} and rel.max() <= total
    tie = z.copy()
    tie[:, 3] = tie[:, 1] = np.maximum(tie.max(1), 1.0) + 1.0                   # classes 1 and 3 tie for the maximum
    assert (S.labels64(tie) == 1).all() and (S.labels64(tie, last_wins=True) == 3).all()
    big = np.where(rng.random(z.shape) < 0.5, 80.0, -80.0).astype(np.float32)
    big[:, 0, 0, 0], big[:, 1:, 0, 0] = 80.0, -80.0
    assert np.isfinite(S.conf32(big)).all()
    bad = S.conf32(big, subtract_max=False)                                    # 1 / sum_j expf(z_j)
    err = np.abs(bad.astype(np.float64) - S.conf64(big)) / S.conf64(big)
    assert not (err <= S.conf_bound(4, 0.0)[0]).all()


# ------------------------------------------------------------------------------------------------ validation
def test_arguments_are_validated_before_any_library_call(monkeypatch):
    from tiaozhanbei_unet_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    n, h, w = 2, 4, 6
    x = torch.zeros((n, 3, h, w))
    lab = torch.zeros((n, h, w), dtype=torch.uint8)
    conf = torch.zeros((n, h, w))
    good = [("image",), ("classes", lab), ("overlay", lab, 0.4), ("lut", conf)]
    bad_calls = [
        dict(images=torch.zeros((n, 1, h, w))), dict(images=torch.zeros((n, 3, h))), dict(images=torch.zeros((0, 3, h, w))),
        dict(images=torch.zeros((n, 3, h, w), dtype=torch.int32)),
        dict(columns=[]), dict(columns=[("image",)] * 9), dict(columns=[("hot", conf)]), dict(columns=[("image", x)]),
        dict(columns=[("classes",)]), dict(columns=[("overlay", lab)]), dict(columns=[("lut", conf, 1.0)]),
        dict(columns=[("classes", conf)]), dict(columns=[("lut", lab)]), dict(columns=[("classes", lab[:1])]),
        dict(columns=[("lut", conf.reshape(n, 1, h, w))]), dict(columns=[("overlay", lab, 1.5)]),
        dict(columns=[("overlay", lab, -0.1)]), dict(columns=[("classes", lab == 0)]),
        dict(gutter=-1), dict(gutter=1.5), dict(per_row=0), dict(per_row=-2),
        dict(palette=torch.zeros((10, 3), dtype=torch.uint8)), dict(lut=torch.zeros((256, 3))),
        dict(images=torch.zeros(1).expand(1, 3, 32768, 32768), columns=[("image",)]),      # 2^31 bytes and more
    ]
    for kw in bad_calls:
        call = dict(images=x, columns=good)
        call.update(kw)
        with pytest.raises(ValueError):
            ops.render_seg_sheet(call.pop("images"), call.pop("columns"), **call)
    # well-formed arguments on the host: the package's refusal of CPU tensors, still ahead of the library
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_seg_sheet(x, good, gutter=0, per_row=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seg_confidence(torch.zeros((n, 3, h, w)))
