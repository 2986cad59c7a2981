"""The visualisation sheet without a GPU: tests/_render_ref.py (the numpy restatement that tests/test_gpu_render.py
holds the device to) against matplotlib's own arithmetic, byte for byte -- the two colour tables, gray / hot panels of
random, constant, bin-boundary, NaN / inf-bearing and all-NaN planes, image / unit panels through ScalarMappable, the
overlay against plain integers, the sheet geometry -- and planted defects that the same comparison must reject."""
import warnings

import numpy as np
import pytest
import torch

import _render_ref as R

H, W = 37, 53


def _rng(seed):
    return np.random.default_rng(seed)


def _boundary_plane(lo=-1.25, hi=3.5):
    """lo + k (hi - lo) / 256 for k = 0 .. 256: pixels exactly on the borders between table entries."""
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    return (lo + np.arange(257) * (hi - lo) / 256).astype(np.float32).reshape(1, -1)


def _planes():
    x = _rng(0).standard_normal((H, W)).astype(np.float32)
    bad = x.copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[H - 1, W - 1] = np.nan, np.inf, -np.inf, np.nan
    return {"random": x, "constant": np.full((4, 5), 0.3, np.float32), "boundary": _boundary_plane(),
            "boundary_rounded": _boundary_plane(0.1, 0.7),       # no fp32 range: the pixels lie a rounding off the borders
            "nonfinite": bad, "all_nan": np.full((3, 3), np.nan, np.float32)}


PLANES = _planes()


def _mpl_map(x, name):
    """matplotlib's rendering of one plane, masked pixels composited to white."""
    from matplotlib import colormaps
    from matplotlib.colors import Normalize
    xm = np.ma.masked_invalid(x.astype(np.float64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rgba = colormaps[name](Normalize()(xm), bytes=True)
    out = rgba[..., :3].copy()
    out[np.ma.getmaskarray(xm)] = 255
    return out


@pytest.mark.parametrize("name", ["gray", "hot"])
def test_lut_bytes_equal_matplotlib(name):
    pytest.importorskip("matplotlib")
    from matplotlib import colormaps
    want = colormaps[name](np.arange(256), bytes=True)[:, :3]
    assert np.array_equal(R.LUTS[name], want)
    from tiaozhanbei_unet_amd import ops
    assert np.array_equal(np.array(ops.colormap_lut(name), np.uint8), want)      # the product's own tables
    if name == "gray":
        assert (want[:, 0] != np.arange(256)).any(), "the gray table is not simply k"


def test_product_builds_its_tables_without_matplotlib():
    import os
    from conftest import ROOT
    files = [os.path.join(ROOT, "tiaozhanbei_unet_amd", "ops.py"), os.path.join(ROOT, "tiaozhanbei_unet_amd", "sheets.py"),
             os.path.join(ROOT, "tiaozhanbei_unet_amd", "test.py"), os.path.join(ROOT, "tests", "_render_ref.py")]
    for path in files:
        src = open(path).read()
        assert "import matplotlib" not in src and "from matplotlib" not in src, path
    from tiaozhanbei_unet_amd import ops
    for name in ("gray", "hot"):
        assert np.array_equal(np.array(ops.colormap_lut(name), np.uint8), R.LUTS[name])
    with pytest.raises(ValueError):
        ops.colormap_lut("viridis")


@pytest.mark.parametrize("name", ["gray", "hot"])
@pytest.mark.parametrize("plane", sorted(PLANES))
def test_map_panels_equal_matplotlib(plane, name):
    pytest.importorskip("matplotlib")
    x = PLANES[plane]
    got = R.map_panel(x, name)
    assert got.dtype == np.uint8 and np.array_equal(got, _mpl_map(x, name))
    if plane == "constant":
        assert (got == ((10, 0, 0) if name == "hot" else (0, 0, 0))).all()        # LUT[0]
    if plane == "all_nan":
        assert (got == 255).all()
    if plane == "nonfinite":
        assert (got[0, 0] == 255).all() and (got[1, 1] == 255).all() and (got[2, 2] == 255).all()
    if plane == "boundary":
        idx, _ = R.map_index(x)
        assert idx.min() == 0 and idx.max() == 255 and len(np.unique(idx)) == 256


def test_panel_range_skips_non_finite_pixels():
    t = np.stack([PLANES["nonfinite"], PLANES["random"]])
    got = R.panel_range(t)
    fin = PLANES["random"].copy()
    fin[0, 0] = fin[1, 1] = fin[2, 2] = fin[H - 1, W - 1] = fin[5, 5]
    assert got[0, 0] == fin.min() and got[0, 1] == fin.max()
    assert got[1, 0] == PLANES["random"].min() and got[1, 1] == PLANES["random"].max()
    assert np.isnan(R.panel_range(PLANES["all_nan"][None])).all()


def _mpl_rgb(v):
    """ScalarMappable's bytes of an (H, W, 3) float32 picture in [0, 1]."""
    from matplotlib.cm import ScalarMappable
    return ScalarMappable().to_rgba(v, bytes=True)[..., :3]


def test_image_and_unit_panels_equal_matplotlib():
    pytest.importorskip("matplotlib")
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, H, W), generator=g) * 1.5                       # N(0, 1.5): both clamps are hit
    v = torch.clamp(x * torch.tensor(R.STD).view(3, 1, 1) + torch.tensor(R.MEAN).view(3, 1, 1), 0, 1)   # fp32, as the reference
    assert (v == 0).any() and (v == 1).any()
    assert np.array_equal(R.image_panel(x.numpy()), _mpl_rgb(v.numpy().transpose(1, 2, 0)))
    u = torch.randn((3, H, W), generator=g) * 1.5
    assert np.array_equal(R.unit_panel(u.numpy()), _mpl_rgb(torch.clamp(u, 0, 1).numpy().transpose(1, 2, 0)))
    nan = np.full((3, 2, 2), np.nan, np.float32)
    assert (R.unit_panel(nan) == 0).all() and (R.image_panel(nan) == 0).all()


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_overlay_is_the_integer_blend(alpha):
    rng = _rng(4)
    img = (rng.standard_normal((3, 9, 11)) * 1.5).astype(np.float32)
    amap = rng.random((9, 11)).astype(np.float32)
    amap[3, 4] = np.nan
    got = R.overlay_panel(img, amap, alpha)
    base, heat = R.image_panel(img), R.map_panel(amap, "hot")
    a8 = {0.0: 0, 0.5: 128, 1.0: 255}[alpha]
    assert R.alpha8(alpha) == a8
    for y in range(9):
        for x in range(11):
            for c in range(3):
                want = int(base[y, x, c]) if (y, x) == (3, 4) else \
                    (a8 * int(heat[y, x, c]) + (255 - a8) * int(base[y, x, c]) + 127) // 255
                assert int(got[y, x, c]) == want
    if alpha == 0.0:
        assert np.array_equal(got, base)
    if alpha == 1.0:
        keep = np.ones((9, 11), bool)
        keep[3, 4] = False
        assert np.array_equal(got[keep], heat[keep])


def _columns(n, h, w, seed):
    rng = _rng(seed)
    return [("image", (rng.standard_normal((n, 3, h, w)) * 1.5).astype(np.float32)),
            ("gray", (rng.random((n, 1, h, w)) > 0.7).astype(np.float32)),
            ("hot", rng.random((n, 1, h, w)).astype(np.float32)),
            ("unit", (rng.standard_normal((n, 3, h, w)) * 0.5 + 0.5).astype(np.float32))]


@pytest.mark.parametrize("g", [0, 1, 4])
def test_sheet_geometry_and_gutters(g):
    n, h, w = 3, 5, 7
    cols = _columns(n, h, w, 5)
    sheet = R.render_sheet(cols, gutter=g)
    assert sheet.shape == (n * h + (n - 1) * g, 4 * w + 3 * g, 3) and sheet.dtype == np.uint8
    covered = np.zeros(sheet.shape[:2], bool)
    for i in range(n):
        for j, col in enumerate(cols):
            y, x = i * (h + g), j * (w + g)
            assert np.array_equal(sheet[y:y + h, x:x + w], R.panel(col, i))
            covered[y:y + h, x:x + w] = True
    assert covered.sum() == n * 4 * h * w
    assert (sheet[~covered] == 255).all() and (~covered).sum() == sheet.shape[0] * sheet.shape[1] - n * 4 * h * w


def test_planted_defects_are_rejected():
    """Each defect a kernel could have changes the bytes (or the shape) that np.array_equal compares on the GPU."""
    rng = _rng(6)
    u = rng.random((3, H, W)).astype(np.float32)
    assert not np.array_equal(R.unit_panel(u), R.unit_panel(u, rounding=True))              # round instead of truncate
    b = PLANES["boundary_rounded"]
    assert not np.array_equal(R.map_panel(b, "hot"), R.map_panel(b, "hot", index_dtype=np.float32))   # index from fp32
    x = PLANES["random"]
    hi = np.unravel_index(np.argmax(x), x.shape)
    assert R.map_index(x, clip_hi=256)[0][hi] == 256 and R.map_index(x)[0][hi] == 255         # a clip that lets 256 through
    assert not np.array_equal(R.map_panel(x, "hot"), R.map_panel(x, "hot", clip_hi=256))
    bad = PLANES["nonfinite"]
    assert not np.array_equal(R.map_panel(bad, "hot"), R.map_panel(bad, "hot", finite_range=False))   # a range with inf
    panels = [[R.panel(c, i) for c in _columns(2, 5, 7, 7)] for i in range(2)]
    assert not np.array_equal(R.assemble(panels, 1, 4), R.assemble(panels, 4, 1))           # a swapped gutter axis
    sq = [row[:2] for row in panels]
    assert not np.array_equal(R.assemble(sq, 1, 4), R.assemble(sq, 4, 1))


def test_cli_takes_the_overlay_flag():
    from tiaozhanbei_unet_amd import test as test_cli
    a = test_cli.parse_args(["--checkpoint", "x.pth"])
    assert a.vis_overlay_alpha is None and a.save_visualizations is False and a.max_vis_samples == 20
    b = test_cli.parse_args(["--checkpoint", "x.pth", "--save_visualizations", "--vis_overlay_alpha", "0.5",
                             "--max_vis_samples", "3"])
    assert b.vis_overlay_alpha == 0.5 and b.save_visualizations and b.max_vis_samples == 3
    with pytest.raises(SystemExit):
        test_cli.parse_args(["--checkpoint", "x.pth", "--vis_overlay_alpha", "1.5"])
    assert callable(test_cli.save_visualizations)
