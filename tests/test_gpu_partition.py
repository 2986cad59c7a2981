"""Every bf16 persistent launcher at several CU budgets, on non-square frames, against a float64 reference.

Each persistent kernel sizes its work split from unet_cu_budget() (CU count minus unet_set_reserved_cus(), rounded down
to a multiple of 8, at least 8; ddp.configure_overlap() reserves CUs on every multi-GPU run).  The budget decides how
many work items a block walks and whether its last round is ragged, the channel-tile interleave co_il, block-mode or
per-tile BatchNorm partials (zdiv), the tpb >= 2 floor and the empty tile ranges padded to a multiple of 8 of the ws
kernels, the split-K count with the narrow (split < 16) or wide reduce and xcd_chunk of the weight gradients, and the
nsplit clamp of convt_wgrad_ws.  The inference entry point unet_conv3x3_bias_relu (BatchNorm(eval) folded into the
weights; families bias_relu / bias_relu2) runs in every kernel variant dispatch<> selects for it, each of which adds the
shift (+ ReLU) with a bias index of its own.  Each case runs at budgets {full, full-8, 136, 40, 24, 8} and asserts, at every one:

  * the profiling bracket is the expected kernel (a case cannot silently move to another kernel);
  * every output passes the float64 comparator of _ref64 (half a bf16 ulp + 2^-18 S; fp32 outputs 2^-18 S);
  * conv / convT forward, data-gradient and dz outputs are bit-identical across budgets, weight gradients and
    statistics sums agree within the fp32 bound;
  * n_parts stays within the cap the API reports;
  * no store lands outside its buffer: every output, partials buffer and workspace sits between two sentinel-filled
    margins that must be untouched afterwards, and so must the partials rows past n_parts.

The branch each budget reaches is restated in plan() below (the same integer formulas as the launchers) and
test_partition_table_reaches_every_budget_branch (no GPU) asserts that the table reaches all of them.
"""
import ctypes as C
import os
import time

import pytest
import torch

import _ref64 as R
from oracle import weights as W

BUDGETS = ("full", "full-8", 136, 40, 24, 8)
MARGIN = 8192                      # sentinel elements before and after every guarded buffer
SENT16, SENT32, SENT8 = 0x7FA5, 0x7FA5A5A5, 0xA5


def cdiv(a, b):
    return -(-a // b)


def ceil8(a):
    return cdiv(a, 8) * 8


# ------------------------------------------------------------------ the case table
# family, kernel bracket, shape, note.  Shapes: N, channels, H, W of the launch frame.  Dispatch rules (conv_api.hip
# dispatch<bf16, 9>, conv3_pdma.hip launch_pdma, wgrad.hip run<>): 64 input channels on one source -> conv3_ws.hip:
# conv3_ws16_kernel on 16-aligned dense frames and conv3_ws_kernel otherwise (one bracket name, "conv3_ws_kernel");
# >= 128 input channels on 16-aligned frames -> launch_pdma<128> if c_out % 128 == 0 else <64>; in launch_pdma
# "pp" = BN == 128 && Ctot >= 512 (ping-pong), "pair" = BN == 64 && !pp && Ctot == 128 (pdma64x2), else lock-step --
# the three share the bracket of their BN.  Weight gradients: wgrad16_variant() 1 (c_out % 128 == 0, w > 16),
# 2 (c_out % 128 == 0, w <= 16, images paired), otherwise wgrad_dma.
CASES = [
    # ---- unet_conv3x3_stats
    ("stats", "conv3_pdma128_kernel", dict(n=3, ci=256, co=128, h=48, w=32),
     "Ctot 256 -> lock-step pdma128; 18 items: fewer than the 24 blocks at full, 3 ragged rounds at 8"),
    ("stats", "conv3_pdma128_kernel", dict(n=1, ci=256, co=256, h=64, w=128),
     "nCo 2: co_il 2 and block-mode partials at full (64 items, 64 blocks), per-tile ragged at 24 / 40; "
     "block mode needs n_tiles * co_il % blocks == 0, so its item count is a multiple of 8 (not ragged at 8)"),
    ("stats", "conv3_pdma128_kernel", dict(n=1, ci=512, co=128, h=32, w=80),
     "Ctot 512 -> ping-pong (pp128); 10 items"),
    ("stats", "conv3_pdma64_kernel", dict(n=3, ci=128, co=64, h=80, w=16),
     "Ctot 128 -> 64: pair (pdma64x2); 15 items"),
    ("stats", "conv3_pdma64_kernel", dict(n=3, ci=256, co=64, h=32, w=48),
     "Ctot 256 -> 64: lock-step pdma64; 18 items"),
    ("stats", "conv3_ws_kernel", dict(n=3, ci=64, co=64, h=32, w=80),
     "16-aligned -> ws16; 30 tiles: tpb floor 2 and one empty padded range at full, ragged last range at 8"),
    ("stats", "conv3_ws_kernel", dict(n=1, ci=64, co=128, h=96, w=48),
     "ws16, two channel groups; 18 tiles x 2"),
    ("stats", "conv3_ws_kernel", dict(n=5, ci=64, co=64, h=40, w=24),
     "ragged frame -> conv3_ws_kernel (per-lane geometry); 30 tiles"),
    # ---- unet_conv3x3: accumulate, two sources with a centre-pad offset, two destinations
    ("fwd_acc", "conv3_pdma128_kernel", dict(n=3, ci=256, co=128, h=32, w=48),
     "accumulate=1 on pdma128 (dst += conv); 18 items"),
    ("fwd_acc", "conv3_ws_kernel", dict(n=3, ci=64, co=64, h=48, w=80),
     "accumulate=1 on ws16; 45 tiles"),
    ("fwd2", "conv3_pdma128_kernel", dict(n=3, c0=128, c1=128, co=128, h=48, w=32, h1=40, w1=24, oy=4, ox=4),
     "second source at an offset: pdma_dense_src = 0; 18 items"),
    ("dgrad2", "conv3_pdma128_kernel", dict(n=1, cy=256, c0=128, c1=128, h=32, w=80, h1=30, w1=72, oy=1, ox=4),
     "two destinations, the second cropped at an offset: pdma_dense = 0; 10 x 2 items"),
    # ---- unet_conv3x3_bias_relu: inference, BatchNorm(eval) folded into the weights, shift (+ ReLU) in the epilogue of
    # every kernel dispatch<> selects (each epilogue has its own hand-written bias index)
    ("bias_relu", "conv3_pdma128_kernel", dict(n=1, ci=256, co=256, h=32, w=48),
     "lock-step pdma128, two channel tiles: 12 items, co_il 2 on 16 blocks down to budget 24, co_il 1 ragged at 8"),
    ("bias_relu", "conv3_pdma128_kernel", dict(n=1, ci=512, co=128, h=32, w=80),
     "Ctot 512 -> ping-pong: the epilogue runs once per half; 10 items"),
    ("bias_relu", "conv3_pdma64_kernel", dict(n=3, ci=128, co=64, h=80, w=16), "pair (pdma64x2); 15 items"),
    ("bias_relu", "conv3_pdma64_kernel", dict(n=3, ci=256, co=64, h=32, w=48, relu=0),
     "lock-step pdma64, relu = 0 (shift only); 18 items"),
    ("bias_relu", "conv3_pdma64_kernel", dict(n=1, ci=256, co=192, h=32, w=48),
     "c_out 192 -> 64-channel tiles, three of them; 6 x 3 items"),
    ("bias_relu", "conv3_ws_kernel", dict(n=3, ci=64, co=64, h=32, w=80), "ws16, one channel group; 30 tiles"),
    ("bias_relu", "conv3_ws_kernel", dict(n=1, ci=64, co=128, h=96, w=48), "ws16, two channel groups; 18 tiles x 2"),
    ("bias_relu", "conv3_ws_kernel", dict(n=5, ci=64, co=64, h=40, w=24), "ragged frame -> conv3_ws_kernel; 30 tiles"),
    ("bias_relu2", "conv3_pdma128_kernel", dict(n=3, c0=128, c1=128, co=128, h=48, w=32, h1=40, w1=24, oy=4, ox=4),
     "skip-concat (every Up block in eval mode), second source at an offset, lock-step; 18 items"),
    ("bias_relu2", "conv3_pdma128_kernel", dict(n=1, c0=256, c1=256, co=128, h=32, w=80, h1=24, w1=72, oy=4, ox=4),
     "skip-concat on the ping-pong kernel (Ctot 512); 10 items"),
    # ---- unet_conv3x3_dgrad_bnrelu
    ("dgrad_bn", "conv3_pdma128_bnbwd_kernel", dict(n=3, cy=256, cx=128, h=48, w=32), "pdma128_bnbwd; 18 items"),
    ("dgrad_bn", "conv3_pdma128_bnbwd_kernel", dict(n=1, cy=512, cx=128, h=32, w=80), "pp128_bnbwd; 10 items"),
    ("dgrad_bn", "conv3_pdma64_bnbwd_kernel", dict(n=3, cy=128, cx=64, h=80, w=16), "pdma64x2_bnbwd; 15 items"),
    ("dgrad_bn", "conv3_ws_bnbwd_kernel", dict(n=3, cy=64, cx=64, h=32, w=80), "ws16 bnbwd; 30 tiles"),
    ("dgrad_bn", "conv3_ws_bnbwd_kernel", dict(n=5, cy=64, cx=64, h=40, w=24), "ws bnbwd, ragged frame; 30 tiles"),
    # ---- unet_conv3x3_wgrad
    ("wgrad", "wgrad16_kernel (+ reduce)", dict(n=3, c0=128, c1=0, co=128, h=20, w=48),
     "variant 1; 30 tiles: split 30 (wide reduce, xcd_chunk) at full, 4 (narrow, no xcd_chunk) at 8"),
    ("wgrad", "wgrad16_kernel (+ reduce)", dict(n=5, c0=64, c1=0, co=128, h=24, w=16),
     "variant 2 (paired images, w <= 16), odd N: the last pair is half empty; 18 tiles"),
    ("wgrad", "wgrad_dma_kernel (+ reduce)", dict(n=3, c0=128, c1=0, co=64, h=24, w=40),
     "64 gradient rows -> wgrad_dma; 27 tiles: split 27 wide at full, 7 narrow at 8"),
    ("wgrad", "wgrad16_kernel (+ reduce)", dict(n=3, c0=128, c1=128, co=128, h=48, w=32, h1=40, w1=24, oy=4, ox=4),
     "two column sources, the second at an offset"),
    # ---- transposed convolution
    ("convt_fwd", "convt_ws_kernel", dict(n=3, ci=128, co=64, h=24, w=40), "convt_ws<128>; 23 tiles"),
    ("convt_fwd", "convt_ws_kernel", dict(n=1, ci=256, co=128, h=40, w=56), "convt_ws<256>; 18 tiles x 2 groups"),
    ("convt_fwd", "convt_gemm_kernel", dict(n=3, ci=512, co=256, h=8, w=24), "convt_gemm (budget-independent)"),
    ("convt_fwd", "convt_gemm_kernel", dict(n=1, ci=1024, co=512, h=12, w=20), "convt_gemm, 1024 -> 512"),
    ("convt_dgrad", "convt_dgrad_ws_kernel", dict(n=3, ci=128, co=64, h=24, w=40), "convt_dgrad_ws<64>; 23 tiles"),
    ("convt_dgrad", "convt_dgrad_ws_kernel", dict(n=1, ci=256, co=128, h=40, w=48), "convt_dgrad_ws<128>; 30 tiles"),
    ("convt_dgrad", "convt_gemm_dgrad_kernel", dict(n=3, ci=512, co=256, h=8, w=24), "convt_gemm dgrad"),
    ("convt_dgrad_bn", "convt_dgrad_ws_bnbwd_kernel", dict(n=3, ci=128, co=64, h=24, w=40), "bnrelu form; 23 tiles"),
    ("convt_wgrad", "convt_wgrad_ws_kernel (+ reduce)", dict(n=3, ci=128, co=64, h=24, w=32),
     "<128>: nsplit 512 clamped to 72 tiles at full, 15 at 8"),
    ("convt_wgrad", "convt_wgrad_ws_kernel (+ reduce)", dict(n=1, ci=256, co=128, h=40, w=64), "<256>: 80 tiles"),
    ("convt_wgrad", "convt_wgrad_ws_kernel (+ reduce)", dict(n=1, ci=512, co=256, h=16, w=32), "<512>: 16 tiles"),
    ("convt_wgrad", "convt_wgrad_ws_kernel (+ reduce)", dict(n=1, ci=1024, co=512, h=16, w=16), "<1024>, w 16: 8 tiles"),
]
IDS = [f"{c[0]}-{c[1].split()[0]}-" + "x".join(str(v) for v in c[2].values()) for c in CASES]


# ------------------------------------------------------------------ restatement of the launchers' partition (coverage)
def plan(case, budget):
    """the budget branches a launch of this case takes (conv3_pdma.hip launch_pdma, conv3_ws.hip unet_internal_conv3_ws, convt_ws.hip
    launch_convt_ws / launch_convt_dgrad_ws, wgrad.hip make_plan / make_plan16 / launch_convt_wgrad_ws), as a set of tags"""
    fam, kern, s, _ = case
    tags = set()

    def rounds(items, blocks):
        tags.add("several_items" if items > blocks else "fewer_items_than_blocks" if items < blocks else "one_item")
        if items > blocks and items % blocks:
            tags.add("ragged_last_round")

    if kern.startswith("conv3_pdma"):
        co = s["cx"] if fam == "dgrad_bn" else (s["c0"] + s["c1"] if fam == "dgrad2" else s["co"])
        bn = 128 if co % 128 == 0 else 64
        n_tiles = s["n"] * cdiv(s["h"], 16) * cdiv(s["w"], 16)
        nco = co // bn
        ctot = s["ci"] if "ci" in s else s["cy"] if "cy" in s else s["c0"] + s["c1"]
        tags.add("pp" if bn == 128 and ctot >= 512 else "pair" if bn == 64 and ctot == 128 else "lockstep")
        tags.add(f"nco{nco}")
        if s.get("c1") and fam != "dgrad2":
            tags.add("two_sources")
        work = n_tiles * nco
        blocks = min(budget, ceil8(work))
        rounds(work, blocks)
        co_il = 1
        while co_il * 2 <= 4 and nco % (co_il * 2) == 0 and blocks % (co_il * 2 * 8) == 0:
            co_il *= 2
        tags.add(f"co_il{co_il}")
        if fam in ("stats", "dgrad_bn"):
            tags.add("zdiv_block" if (n_tiles * co_il) % blocks == 0 else "zdiv_tile")
    elif kern.startswith("conv3_ws"):
        co = s.get("co", s.get("cx"))
        tiles = s["n"] * cdiv(s["h"], 16) * cdiv(s["w"], 16)
        tags.add(f"ws16_groups{co // 64}" if s["h"] % 16 == 0 and s["w"] % 16 == 0 else "ws_ragged_frame")
        tpb = cdiv(tiles * (co // 64), budget)
        if tpb < 2:
            tags.add("tpb_floor")
        tpb = max(tpb, 2)
        if ceil8(cdiv(tiles, tpb)) * tpb >= tiles + tpb:
            tags.add("empty_ranges")
        tags.add("several_items")
        if tiles % tpb:
            tags.add("ragged_last_round")
    elif kern == "convt_ws_kernel":
        tiles = cdiv(s["n"] * s["h"] * s["w"], 128)
        tpb = cdiv(tiles * (4 * s["co"] // 256), budget)
        if tpb < 2:
            tags.add("tpb_floor")
        tpb = max(tpb, 2)
        if ceil8(cdiv(tiles, tpb)) * tpb >= tiles + tpb:
            tags.add("empty_ranges")
        tags.add("several_items")
        if tiles % tpb:
            tags.add("ragged_last_round")
    elif kern.startswith("convt_dgrad_ws"):
        tiles = cdiv(s["n"] * s["h"] * s["w"], 128 if s["co"] <= 64 else 64)
        tpb = cdiv(tiles, min(256, budget))
        if tpb < 2:
            tags.add("tpb_floor")
        tpb = max(tpb, 2)
        tags.add("several_items")
        if tiles % tpb:
            tags.add("ragged_last_round")
    elif kern.startswith("wgrad"):
        ctot, co = s["c0"] + s["c1"], s["co"]
        if kern.startswith("wgrad16"):
            paired = s["w"] <= 16
            ntiles = (cdiv(s["n"], 2) if paired else s["n"]) * cdiv(s["h"], 4) * (1 if paired else cdiv(s["w"], 32))
            nrc = (co // 128) * (ctot // 64)
            want = max(1, budget // nrc)
        else:
            ntiles = s["n"] * cdiv(s["h"], 8) * cdiv(s["w"], 16)
            nrc = (co // 64) * (ctot // 64)
            want = max(1, 2 * budget // nrc)
        if want > ntiles:
            tags.add("split_clamped")
        want = min(want, ntiles)
        split = cdiv(ntiles, cdiv(ntiles, want))
        tags.add("reduce_wide" if split >= 16 else "reduce_narrow")
        tags.add("xcd_chunk" if split * nrc >= 16 else "no_xcd_chunk")
    elif kern.startswith("convt_wgrad_ws"):
        tiles = s["n"] * s["h"] * s["w"] // 32
        nsplit = max(1, 2 * budget // (s["ci"] // 128) ** 2)
        tags.add("nsplit_clamped" if nsplit > tiles else "nsplit_budget")
    return tags


def budget_value(b, full):
    return full if b == "full" else full - 8 if b == "full-8" else b


def test_partition_table_reaches_every_budget_branch():
    """(no GPU) the table, at the budgets of the test and a 256-CU device, reaches every budget-dependent branch"""
    seen = set()
    for case in CASES:
        for b in BUDGETS:
            seen |= {(case[1].split("_kernel")[0].split()[0][:10], t) for t in plan(case, budget_value(b, 256))}
    tags = {t for _, t in seen}
    want = {"several_items", "fewer_items_than_blocks", "ragged_last_round", "co_il1", "co_il2", "zdiv_block",
            "zdiv_tile", "tpb_floor", "empty_ranges", "reduce_wide", "reduce_narrow", "xcd_chunk", "no_xcd_chunk",
            "split_clamped", "nsplit_clamped", "nsplit_budget"}
    assert want <= tags, sorted(want - tags)
    # every persistent case walks several items per block at budget 8, ragged unless it is the block-mode row
    for case in CASES:
        if "gemm" in case[1] or "wgrad" in case[1]:
            continue
        t = plan(case, 8)
        assert "several_items" in t, (case[1], case[2], t)
        assert "ragged_last_round" in t or "block-mode" in case[3], (case[1], case[2], t)
    # the inference epilogue (bias_relu / bias_relu2) is entered in every kernel variant dispatch<> can select for it
    fold = set()
    for case in CASES:
        if case[0].startswith("bias_relu"):
            bn = case[1].split("_")[1] if "pdma" in case[1] else "ws"
            fold |= {(bn, t) for b in BUDGETS for t in plan(case, budget_value(b, 256))}
    want = {("pdma128", "lockstep"), ("pdma128", "nco2"), ("pdma128", "pp"), ("pdma128", "co_il2"), ("pdma128", "co_il1"),
            ("pdma64", "pair"), ("pdma64", "lockstep"), ("pdma64", "nco3"), ("ws", "ws16_groups1"), ("ws", "ws16_groups2"),
            ("ws", "ws_ragged_frame")}
    assert want <= fold, sorted(want - fold)
    two = [plan(c, 256) for c in CASES if c[0] == "bias_relu2"]
    assert any({"two_sources", "lockstep"} <= t for t in two) and any({"two_sources", "pp"} <= t for t in two)
    assert sum(1 for c in CASES if c[0].startswith("bias_relu") and c[2].get("relu", 1) == 0) == 1
    # the weight-gradient cases stay within the K the CPU self-test plants its missing block at
    for fam, _, s, _ in CASES:
        if fam in ("wgrad", "convt_wgrad"):
            assert s["n"] * s["h"] * s["w"] <= R.MAX_WGRAD_K


# ------------------------------------------------------------------ GPU plumbing
def dev():
    return torch.device("cuda:0")


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return C.c_void_p(t.data_ptr())


class Guards:
    """buffers allocated between two sentinel-filled margins; check() asserts the margins are untouched"""

    def __init__(self):
        self.items = []

    def alloc(self, numel, dtype, what):
        ity = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[dtype]
        sent = {torch.int16: SENT16, torch.int32: SENT32, torch.uint8: SENT8}[ity]
        buf = torch.empty(numel + 2 * MARGIN, dtype=dtype, device=dev())
        iv = buf.view(ity)
        iv.fill_(sent)
        self.items.append((what, iv, numel, sent))
        return buf[MARGIN:MARGIN + numel]

    def nhwc(self, n, c, h, w, what, fill=None, dtype=torch.bfloat16):
        t = self.alloc(n * c * h * w, dtype, what).view(n, h, w, c).permute(0, 3, 1, 2)
        if fill is not None:
            t.copy_(fill)
        return t

    def check(self, tail=()):
        """margins untouched; `tail`: (what, offset, length) element ranges inside a buffer that must be untouched too"""
        torch.cuda.synchronize()
        for what, iv, numel, sent in self.items:
            for lo, hi, side in ((0, MARGIN, "before"), (MARGIN + numel, 2 * MARGIN + numel, "after")):
                bad = (iv[lo:hi] != sent).nonzero()
                assert bad.numel() == 0, f"{what}: {bad.numel()} stores in the guard {side} the buffer (first at " \
                                         f"element {int(bad[0]) - (lo if side == 'after' else MARGIN)} of the margin)"
        for what, off, length in tail:
            iv, sent = next((i, v) for w, i, _, v in self.items if w == what)
            seg = iv[MARGIN + off:MARGIN + off + length]
            bad = (seg != sent).nonzero()
            assert bad.numel() == 0, f"{what}: {bad.numel()} stores past n_parts (first at element {off + int(bad[0])})"


def rnd(tag, shape, scale=1.0):
    return (W.make_input("part:" + tag, shape) * scale).to(torch.bfloat16).float()


def to_nhwc(t):
    return t.to(dev()).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def views(L, items):
    arr = L.View2()
    for i, it in enumerate(items):
        arr[i] = L.View(None, 0, 0, 0, 0, 0) if it is None else L.View(it[0].data_ptr(), it[0].shape[1],
                                                                        it[0].shape[2], it[0].shape[3], it[1], it[2])
    return arr


def bn_coefs(y, cx):
    gamma = rnd("gamma", (cx,), 0.5) + 1.0
    beta = rnd("beta", (cx,), 0.3)
    yd = y.double()
    mean = yd.mean((0, 2, 3))
    istd = 1.0 / torch.sqrt(yd.var((0, 2, 3), unbiased=False) + 1e-5)
    scale = gamma.double() * istd
    shift = beta.double() - mean * scale
    return torch.stack([mean, istd, scale, shift]).float()


# ------------------------------------------------------------------ per-family: inputs + reference, launch
def eval_coeffs(L, co, tag):
    """per-channel BatchNorm(eval) parameters, all distinct, with a shift of the order of the activations (sigma ~ 1: a
    bias from the wrong lane or channel tile moves an element by many bounds), and (scale, shift) as
    unet_bn_eval_coeffs returns them, read back -- the reference takes those, so that kernel's rounding (held to its own
    bound here) stays out of the convolution's"""
    gamma = W.make_input("part:" + tag + "gamma", (co,), kind="uniform") + 0.5
    beta = W.make_input("part:" + tag + "beta", (co,))
    rm = W.make_input("part:" + tag + "rm", (co,)) * 0.5
    rv = W.make_input("part:" + tag + "rv", (co,), kind="uniform") * 1.5 + 0.25
    g, b, m, v = (t.float().to(dev()).contiguous() for t in (gamma, beta, rm, rv))
    ss = torch.empty((2, co), dtype=torch.float32, device=dev())
    L.check(L.lib().unet_bn_eval_coeffs(co, p(g), p(b), p(m), p(v), C.c_float(1e-5), p(ss[0]), p(ss[1]), st()), "coeffs")
    scale, shift = ss[0].cpu(), ss[1].cpu()
    want = R.bn_eval_coeffs(gamma.float(), beta.float(), rm.float(), rv.float())
    R.assert_fp32(scale, want["scale"], "unet_bn_eval_coeffs scale")
    R.assert_fp32(shift, want["shift"], "unet_bn_eval_coeffs shift")
    assert float(shift.abs().mean()) > 0.3 and shift.unique().numel() == co and scale.unique().numel() == co
    return scale, shift


def make_case(fam, s, L=None):
    """CPU inputs (bf16-exact fp32) and the float64 references {name: (ref, S, kind, mask)}"""
    tag = fam + str(sorted(s.items()))
    inp, ref = {}, {}
    n, h, w = s["n"], s["h"], s["w"]
    if fam in ("stats", "fwd_acc"):
        ci, co = s["ci"], s["co"]
        inp["x"] = rnd(tag + "x", (n, ci, h, w))
        inp["w"] = rnd(tag + "w", (co, ci, 3, 3), 1 / (3 * ci ** 0.5))
        r, S = R.conv3x3(inp["x"], inp["w"])
        if fam == "fwd_acc":
            inp["old"] = rnd(tag + "old", (n, co, h, w))
            r, S = r + inp["old"].double(), S + inp["old"].double().abs()
        ref["y"] = (r, S, "bf16", None)
    elif fam == "fwd2":
        c0, c1, co = s["c0"], s["c1"], s["co"]
        inp["x2"], inp["x1"] = rnd(tag + "x2", (n, c0, h, w)), rnd(tag + "x1", (n, c1, s["h1"], s["w1"]))
        inp["w"] = rnd(tag + "w", (co, c0 + c1, 3, 3), 1 / (3 * (c0 + c1) ** 0.5))
        x1p = torch.nn.functional.pad(inp["x1"], [s["ox"], w - s["w1"] - s["ox"], s["oy"], h - s["h1"] - s["oy"]])
        r, S = R.conv3x3(torch.cat([inp["x2"], x1p], 1), inp["w"])
        ref["y"] = (r, S, "bf16", None)
    elif fam in ("bias_relu", "bias_relu2"):
        co = s["co"]
        if fam == "bias_relu":
            ctot = s["ci"]
            inp["x"] = xs = rnd(tag + "x", (n, ctot, h, w))
        else:
            c0, c1, ctot = s["c0"], s["c1"], s["c0"] + s["c1"]
            inp["x2"], inp["x1"] = rnd(tag + "x2", (n, c0, h, w)), rnd(tag + "x1", (n, c1, s["h1"], s["w1"]))
            x1p = torch.nn.functional.pad(inp["x1"], [s["ox"], w - s["w1"] - s["ox"], s["oy"], h - s["h1"] - s["oy"]])
            xs = torch.cat([inp["x2"], x1p], 1)
        inp["w"] = W.make_input("part:" + tag + "w", (co, ctot, 3, 3)).float() * (1 / (3 * ctot ** 0.5))     # fp32 operand
        inp["scale"], inp["shift"] = eval_coeffs(L, co, tag)
        r, S = R.conv3x3_bias_relu(xs, inp["w"], inp["scale"], inp["shift"], torch.bfloat16, relu=bool(s.get("relu", 1)))
        if s.get("relu", 1):
            assert 0.2 < float((r == 0).double().mean()) < 0.8, "the ReLU must clip a good part of the output, not all"
        ref["y"] = (r, S, "bf16", None)
    elif fam == "dgrad2":
        cy, c0, c1 = s["cy"], s["c0"], s["c1"]
        inp["dy"] = rnd(tag + "dy", (n, cy, h, w))
        inp["w"] = rnd(tag + "w", (cy, c0 + c1, 3, 3), 1 / (3 * cy ** 0.5))
        r, S = R.conv3x3_dgrad(inp["dy"], inp["w"])
        oy, ox, h1, w1 = s["oy"], s["ox"], s["h1"], s["w1"]
        ref["d2"] = (r[:, :c0], S[:, :c0], "bf16", None)
        ref["d1"] = (r[:, c0:, oy:oy + h1, ox:ox + w1], S[:, c0:, oy:oy + h1, ox:ox + w1], "bf16", None)
    elif fam in ("dgrad_bn", "convt_dgrad_bn"):
        if fam == "dgrad_bn":
            cy, cx = s["cy"], s["cx"]
            inp["dy"] = rnd(tag + "dy", (n, cy, h, w))
            inp["w"] = rnd(tag + "w", (cy, cx, 3, 3), 1 / (3 * cy ** 0.5))
            r, S = R.conv3x3_dgrad(inp["dy"], inp["w"])
        else:
            cx, co = s["ci"], s["co"]
            inp["dy"] = rnd(tag + "dy", (n, co, 2 * h, 2 * w))
            inp["w"] = rnd(tag + "w", (cx, co, 2, 2), 0.1)
            r, S = R.convt2x2_dgrad(inp["dy"], inp["w"])
        inp["y"] = rnd(tag + "y", (n, cx, h, w), 1.3) + 0.2
        inp["y"] = inp["y"].to(torch.bfloat16).float()
        inp["coef"] = bn_coefs(inp["y"], cx)
        on, clear = R.bn_relu_mask(inp["y"], inp["coef"][2], inp["coef"][3])
        assert float((~clear).double().mean()) < 1e-3, "too many ReLU decisions at rounding level"
        ref["dz"] = (r * on, S * on, "bf16", clear)
    elif fam == "wgrad":
        c0, c1, co = s["c0"], s["c1"], s["co"]
        inp["x2"] = rnd(tag + "x2", (n, c0, h, w))
        xs = inp["x2"]
        if c1:
            inp["x1"] = rnd(tag + "x1", (n, c1, s["h1"], s["w1"]))
            x1p = torch.nn.functional.pad(inp["x1"], [s["ox"], w - s["w1"] - s["ox"], s["oy"], h - s["h1"] - s["oy"]])
            xs = torch.cat([xs, x1p], 1)
        inp["dy"] = rnd(tag + "dy", (n, co, h, w))
        r, S = R.conv3x3_wgrad(xs, inp["dy"])
        ref["dw"] = (r, S, "fp32", None)
    elif fam == "convt_fwd":
        ci, co = s["ci"], s["co"]
        inp["x"] = rnd(tag + "x", (n, ci, h, w))
        inp["w"] = rnd(tag + "w", (ci, co, 2, 2), 0.1)
        inp["b"] = W.make_input("part:" + tag + "b", (co,)) * 0.5       # fp32 operand
        r, S = R.convt2x2(inp["x"], inp["w"], inp["b"])
        ref["y"] = (r, S, "bf16", None)
    elif fam == "convt_dgrad":
        ci, co = s["ci"], s["co"]
        inp["dy"] = rnd(tag + "dy", (n, co, 2 * h, 2 * w))
        inp["w"] = rnd(tag + "w", (ci, co, 2, 2), 0.1)
        r, S = R.convt2x2_dgrad(inp["dy"], inp["w"])
        ref["dx"] = (r, S, "bf16", None)
    elif fam == "convt_wgrad":
        ci, co = s["ci"], s["co"]
        inp["x"] = rnd(tag + "x", (n, ci, h, w))
        inp["dy"] = rnd(tag + "dy", (n, co, 2 * h, 2 * w))
        (dw, db) = R.convt2x2_wgrad(inp["x"], inp["dy"])
        ref["dw"] = dw + ("fp32", None)
        ref["db"] = db + ("fp32", None)
    return inp, ref


def launch(L, ops, fam, s, d, G):
    """run the entry point once on guarded outputs; returns ({name: output}, [(what, n_parts, cap, row_elems)])"""
    lib, dt = L.lib(), L.UNET_BF16
    n, h, w = s["n"], s["h"], s["w"]
    out, parts = {}, []
    if fam in ("stats", "fwd_acc", "fwd2"):
        co = s["co"]
        if fam == "fwd2":
            src = views(L, [(d["x2"], 0, 0), (d["x1"], s["oy"], s["ox"])])
        else:
            src = views(L, [(d["x"], 0, 0), None])
        y = G.nhwc(n, co, h, w, "y", fill=d.get("old"))
        if fam == "stats":
            cap = lib.unet_conv3x3_stats_max_parts(n, h, w)
            part = G.alloc(cap * 2 * co, torch.float32, "partials")
            nparts = C.c_int32(-1)
            L.check(lib.unet_conv3x3_stats(dt, n, h, w, src, p(d["wp"]), co, p(y), p(part), C.byref(nparts), st()), "stats")
            parts.append(("partials", nparts.value, cap, 2 * co))
            out["sums"] = part[:max(nparts.value, 0) * 2 * co].view(-1, 2, co).double().sum(0).cpu()
        else:
            L.check(lib.unet_conv3x3(dt, n, h, w, src, p(d["wp"]), co, views(L, [(y, 0, 0), None]), co,
                                     1 if fam == "fwd_acc" else 0, L.K_CONV_FWD, st()), "conv3x3")
        out["y"] = y
    elif fam in ("bias_relu", "bias_relu2"):
        co = s["co"]
        if fam == "bias_relu2":
            src = views(L, [(d["x2"], 0, 0), (d["x1"], s["oy"], s["ox"])])
        else:
            src = views(L, [(d["x"], 0, 0), None])
        y = G.nhwc(n, co, h, w, "y")
        L.check(lib.unet_conv3x3_bias_relu(dt, n, h, w, src, p(d["wp"]), co, p(y), p(d["shift"]), int(s.get("relu", 1)),
                                           st()), "conv3x3 bias relu")
        out["y"] = y
    elif fam == "dgrad2":
        c0, c1 = s["c0"], s["c1"]
        d2 = G.nhwc(n, c0, h, w, "d2")
        d1 = G.nhwc(n, c1, s["h1"], s["w1"], "d1")
        L.check(lib.unet_conv3x3(dt, n, h, w, views(L, [(d["dy"], 0, 0), None]), p(d["wp"]), c0 + c1,
                                 views(L, [(d2, 0, 0), (d1, s["oy"], s["ox"])]), c0, 0, L.K_CONV_DGRAD, st()), "dgrad2")
        out["d2"], out["d1"] = d2, d1
    elif fam in ("dgrad_bn", "convt_dgrad_bn"):
        cx = s.get("cx", s.get("ci"))
        dz = G.nhwc(n, cx, h, w, "dz")
        coef = d["coef"]
        if fam == "dgrad_bn":
            cap = lib.unet_conv3x3_stats_max_parts(n, h, w)
        else:
            cap = lib.unet_convt2x2_dgrad_bnrelu_max_parts()
        part = G.alloc(cap * 2 * cx, torch.float32, "partials")
        nparts = C.c_int32(-1)
        if fam == "dgrad_bn":
            L.check(lib.unet_conv3x3_dgrad_bnrelu(dt, n, h, w, p(d["dy"]), s["cy"], p(d["wp"]), cx, p(d["y"]), p(coef[2]),
                                                  p(coef[3]), p(coef[0]), p(dz), p(part), C.byref(nparts), st()), "dgrad bn")
        else:
            L.check(lib.unet_convt2x2_dgrad_bnrelu(dt, n, h, w, p(d["dy"]), s["co"], p(d["wp"]), p(d["y"]), p(coef[2]),
                                                   p(coef[3]), p(coef[0]), p(dz), cx, p(part), C.byref(nparts), st()),
                    "convt dgrad bn")
        parts.append(("partials", nparts.value, cap, 2 * cx))
        out["dz"] = dz
        out["sums"] = part[:max(nparts.value, 0) * 2 * cx].view(-1, 2, cx).double().sum(0).cpu()
    elif fam == "wgrad":
        c0, c1, co = s["c0"], s["c1"], s["co"]
        src = views(L, [(d["x2"], 0, 0), (d["x1"], s["oy"], s["ox"]) if c1 else None])
        dw = G.alloc(co * (c0 + c1) * 9, torch.float32, "dw").view(co, c0 + c1, 3, 3)
        need = lib.unet_conv3x3_wgrad_workspace(n, h, w, c0 + c1, co)
        ws = G.alloc(need, torch.uint8, "workspace")
        L.check(lib.unet_conv3x3_wgrad(dt, n, h, w, src, p(d["dy"]), co, p(dw), c0 + c1, p(ws), need, st()), "wgrad")
        out["dw"] = dw
    elif fam == "convt_fwd":
        ci, co = s["ci"], s["co"]
        y = G.nhwc(n, co, 2 * h, 2 * w, "y")
        L.check(lib.unet_convt2x2_fwd(dt, n, h, w, p(d["x"]), ci, p(d["wp"]), p(d["b"]), p(y), co, st()), "convt fwd")
        out["y"] = y
    elif fam == "convt_dgrad":
        ci, co = s["ci"], s["co"]
        dx = G.nhwc(n, ci, h, w, "dx")
        L.check(lib.unet_convt2x2_dgrad(dt, n, h, w, p(d["dy"]), co, p(d["wp"]), p(dx), ci, st()), "convt dgrad")
        out["dx"] = dx
    elif fam == "convt_wgrad":
        ci, co = s["ci"], s["co"]
        dw = G.alloc(ci * co * 4, torch.float32, "dw").view(ci, co, 2, 2)
        db = G.alloc(co, torch.float32, "db")
        need = lib.unet_convt2x2_wgrad_workspace(n, h, w, ci, co)
        ws = G.alloc(need, torch.uint8, "workspace")
        L.check(lib.unet_convt2x2_wgrad(dt, n, h, w, p(d["x"]), ci, p(d["dy"]), co, p(dw), p(db), p(ws), need, st()),
                "convt wgrad")
        out["dw"], out["db"] = dw, db
    return out, parts


def to_device(L, ops, fam, s, inp):
    d = {}
    for k, v in inp.items():
        if k in ("w", "b", "coef", "scale", "shift"):
            d[k] = v.to(dev()).contiguous()
        else:
            d[k] = to_nhwc(v)
    if "w" in inp:
        wd = d["w"]
        if fam in ("bias_relu", "bias_relu2"):
            co, ctot = wd.shape[0], wd.shape[1]
            d["wp"] = torch.empty(9 * co * ctot, dtype=torch.bfloat16, device=dev())
            L.check(L.lib().unet_pack_conv_weight_folded(p(wd), p(d["scale"]), p(d["wp"]), co, ctot, co, ctot, L.UNET_BF16,
                                                         st()), "fold")
        elif fam in ("stats", "fwd_acc", "fwd2"):
            d["wp"] = ops.pack_weight(wd, L.PACK_CONV_FWD, wd.shape[0], wd.shape[1], torch.bfloat16)
        elif fam in ("dgrad2", "dgrad_bn"):
            d["wp"] = ops.pack_weight(wd, L.PACK_CONV_DGRAD, wd.shape[1], wd.shape[0], torch.bfloat16)
        elif fam == "convt_fwd":
            d["wp"] = ops.pack_weight(wd, L.PACK_CONVT_FWD, wd.shape[1], wd.shape[0], torch.bfloat16)
        else:
            d["wp"] = ops.pack_weight(wd, L.PACK_CONVT_DGRAD, wd.shape[0], wd.shape[1], torch.bfloat16)
    return d


def stat_refs(fam, out, d):
    """float64 (sum, S) of the two partial-sum statistics over the outputs as stored"""
    if fam == "stats":
        y = out["y"].double().cpu()
        s0 = R.sums_over_pixels(y)
        s1 = R.sums_over_pixels(y * y)
    else:
        dz = out["dz"].double().cpu()
        mean = d["coef"][0].double().cpu()[None, :, None, None]
        yc = d["y"].double().cpu() - mean
        s0 = R.sums_over_pixels(dz)
        s1 = ((dz * yc).sum((0, 2, 3)), (dz.abs() * (d["y"].double().cpu().abs() + mean.abs())).sum((0, 2, 3)))
    return torch.stack([s0[0], s1[0]]), torch.stack([s0[1], s1[1]])


_REFS = {}


@pytest.fixture(scope="module")
def hip():
    from tiaozhanbei_unet_amd import _lib, ops
    return _lib, ops


@pytest.fixture
def budget(hip):
    """set_budget(b) -> the budget in force; reserved CUs go back to 0 whatever happens"""
    L, _ = hip
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L.check(L.lib().unet_set_reserved_cus(0), "reserved 0")
    full = L.lib().unet_get_cu_budget()

    def set_budget(b):
        want = budget_value(b, full)
        L.check(L.lib().unet_set_reserved_cus(max(0, cus - want)), "reserve")
        got = L.lib().unet_get_cu_budget()
        assert got == want, (b, want, got)
        return got
    try:
        yield full, set_budget
    finally:
        L.lib().unet_set_reserved_cus(0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_persistent_launcher_across_cu_budgets(hip, budget, case):
    L, ops = hip
    O = ops
    fam, kern, s, _ = case
    full, set_budget = budget
    t0 = time.time()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    key = (fam, tuple(sorted(s.items())))
    if key not in _REFS:
        _REFS[key] = make_case(fam, s, L)
    inp, ref = _REFS[key]
    d = to_device(L, ops, fam, s, inp)
    torch.cuda.synchronize()
    first, worst, seen, per_budget = None, {"bf16": 0.0, "fp32": 0.0}, set(), {}
    for b in BUDGETS:
        bv = set_budget(b)
        if bv in seen:
            continue
        seen.add(bv)
        G = Guards()
        O.prof_enable(True)
        try:
            out, parts = launch(L, ops, fam, s, d, G)
            torch.cuda.synchronize()
        finally:
            O.prof_collect()
            O.prof_enable(False)
        names = set(O.prof_kernels())
        assert names == {kern}, f"budget {bv}: brackets {names}, expected {kern}"
        tail = []
        for what, np_, cap, row in parts:
            assert 0 < np_ <= cap, f"budget {bv}: n_parts {np_} outside (0, {cap}]"
            tail.append((what, np_ * row, (cap - np_) * row))
        G.check(tail)
        at = f"[budget {bv}] {fam} {kern}"
        for name, (r, S, kind, mask) in ref.items():
            fn = R.assert_bf16 if kind == "bf16" else R.assert_fp32
            got = fn(out[name].float(), (r, S), f"{at} {name}", mask)
            worst[kind] = max(worst[kind], got)
            per_budget[bv] = max(per_budget.get(bv, 0.0), got)
        if "sums" in out:
            sr, sS = stat_refs(fam, out, d)
            worst["fp32"] = max(worst["fp32"], R.assert_fp32(out["sums"], (sr, sS), f"{at} statistics sums"))
        host = {k: v.detach().cpu().clone() for k, v in out.items()}
        if first is None:
            first = (bv, host)
            continue
        for name, v in host.items():
            kind = ref[name][2] if name in ref else "fp32"
            if kind == "bf16":
                assert torch.equal(v, first[1][name]), f"{at} {name}: differs from budget {first[0]} (must be bit-identical)"
            else:
                v0 = first[1][name].double()
                Sx = ref[name][1] if name in ref else stat_refs(fam, out, d)[1]
                R.assert_fp32(v.double(), (v0, 2 * Sx), f"{at} {name} vs budget {first[0]}")
    print(f"[{fam} {kern} {s}] budgets {sorted(seen)}: worst err/bound bf16 {worst['bf16']:.3f} fp32 {worst['fp32']:.3f} "
          f"per budget {' '.join(f'{b}:{v:.3f}' for b, v in sorted(per_budget.items()))} ({time.time() - t0:.1f} s)")
