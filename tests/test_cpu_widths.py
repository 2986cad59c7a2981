"""CPU checks of the building blocks at channel widths that are not multiples of 64: they construct like the reference's
(no ValueError), keep its state_dict layout, and the segment map of a narrow skip is what the kernels assume."""
import pytest

from oracle import weights as W

NARROW = [
    ("double_conv", (3, 32)),
    ("double_conv", (3, 16)),
    ("double_conv", (40, 96, 48)),
    ("down", (96, 160)),
    ("up", (160, 80, False)),
    ("up", (192, 96, True)),
    ("outconv", (48, 2)),
]


def _block(kind, args, precision):
    import tiaozhanbei_unet_amd as P
    cls = {"double_conv": P.DoubleConv, "down": P.Down, "up": P.Up, "outconv": P.OutConv}[kind]
    return cls(*args, precision=precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,args", NARROW, ids=[f"{k}_{'_'.join(map(str, a))}" for k, a in NARROW])
def test_narrow_blocks_keep_the_reference_state_dict(kind, args, precision):
    m = _block(kind, args, precision)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    want = [(k, tuple(s)) for k, s in W.block_spec(kind, *args).items()]
    assert got == want
    m.load_state_dict(W.make_state(W.block_spec(kind, *args), 0))


def test_up_records_the_skip_split_of_a_narrow_skip():
    import tiaozhanbei_unet_amd as P
    assert P.Up(160, 80, False).conv.skip_split == 80
    assert P.Up(192, 96, True).conv.skip_split == 96
    assert P.Up(384, 192, False).conv.skip_split == 0
    assert P.Up(1024, 512, False).conv.skip_split == 0


def test_segment_map():
    from tiaozhanbei_unet_amd import ops
    assert ops.seg_cols(128, 0) == 128 and ops.seg_cols(40, 0) == 64
    assert ops.seg_cols(160, 80) == 256 and ops.seg_cols(96, 48) == 128 and ops.seg_cols(48, 24) == 128
    # skip 80 + up 80: columns [0, 80) -> 0..79, [80, 128) zero, [128, 208) -> 80..159, [208, 256) zero
    cols = [ops.seg_col(q, 80, 160) for q in range(256)]
    assert cols[:80] == list(range(80))
    assert cols[80:128] == [-1] * 48
    assert cols[128:208] == list(range(80, 160))
    assert cols[208:] == [-1] * 48
    # contiguous map: columns past the parameter's are zero
    assert [ops.seg_col(q, 0, 40) for q in range(64)] == list(range(40)) + [-1] * 24
    # every parameter column appears exactly once
    for c0, ci in ((24, 48), (48, 96), (96, 192), (80, 160), (1, 2)):
        hits = [ops.seg_col(q, c0, ci) for q in range(ops.seg_cols(ci, c0))]
        assert sorted(h for h in hits if h >= 0) == list(range(ci))


def test_remap_descriptor_layout_matches_the_header():
    import ctypes
    from tiaozhanbei_unet_amd import _lib as L
    assert ctypes.sizeof(L.RemapDesc) == 48
    assert L.RemapDesc.rows.offset == 16 and L.RemapDesc.op.offset == 40
