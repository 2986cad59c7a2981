"""Eval-mode inference held to float64: unet_conv3x3_bias_relu (BatchNorm(eval) folded into the weights, shift + ReLU in
the epilogue of whichever kernel dispatch<> selects) at the sizes where the epilogues' hand-written bias indices can go
wrong without the small cases noticing, and the bf16 models in eval() under no_grad against the fp32 oracle.

Kernel level (comparator of _ref64: half a bf16 ulp + 2^-18 S, fp32 2^-18 S; reference R.conv3x3_bias_relu on the
coefficients unet_bn_eval_coeffs returned):
  * one case per persistent family with more work items than blocks and, where the family has them, at least two
    channel tiles: the bias pointer is recomputed per work item from the channel tile, only this sees a stale one;
  * the register-staged kernels of launch3 (conv3m16_kernel, conv3_kernel) in fp32 and bf16 on frames that are not
    16-aligned, 128 / 192 / 256 input channels, 64 / 128 / 192 outputs; with those channel counts dispatch<> never takes
    igemm_kernel or a k4 == false form, so three small cases with 32 (fp32) and 32 + 32 (bf16, two sources) input
    channels enter igemm_kernel's 3x3 epilogue, one of them in its one-k-group form.
test_gpu_partition.py runs the same entry point in every kernel variant at six CU budgets on small frames.

Model level: AnomalyUNet(3) and UNet(3, 4), bf16, at 1x3x256x256 (every level 16-aligned down to 16x16: persistent
kernels throughout, the ping-pong kernel at the bottom) and 1x3x256x320 (the two deepest levels fall to the
register-staged kernels) -- the kernel brackets of each forward are asserted.  The bound is the oracle's own bf16 noise, measured in the test:
e_ref = max |oracle under bf16_storage() - fp32 oracle| per output, and the library must stay within 3 e_ref of the fp32
oracle (3: the folded path rounds w * scale to bf16 and skips the rounding of y, so its error is another draw of the
same size, and the maximum runs over 10^5 elements).  Thresholded masks and argmax must agree with the fp32 oracle
outside pixels whose fp32 margin is below 2 * 3 e_ref, and at most 1 % of the pixels may be excluded that way."""
import time

import pytest
import torch

import _ref64 as R
from oracle import unet_oracle as O
from oracle import weights as W
from test_gpu_partition import cdiv, dev, eval_coeffs, hip, p, st, views      # noqa: F401  (hip: the fixture)


def run_folded(L, ops, dtype, n, h, w, srcs, offs, wt, scale, shift, co, relu=1):
    """fold + unet_conv3x3_bias_relu -> (y, {bracket names})"""
    dt = ops._DT[dtype]
    xs = [(t.to(dev()).to(dtype).contiguous(memory_format=torch.channels_last)) for t in srcs]
    ctot = sum(t.shape[1] for t in srcs)
    wd, sc, sh = wt.to(dev()).contiguous(), scale.to(dev()).contiguous(), shift.to(dev()).contiguous()
    wq = torch.empty(9 * co * ctot, dtype=dtype, device=dev())
    L.check(L.lib().unet_pack_conv_weight_folded(p(wd), p(sc), p(wq), co, ctot, co, ctot, dt, st()), "fold")
    y = ops._nhwc_empty(n, co, h, w, dtype, dev())
    src = views(L, [(xs[0], 0, 0), (xs[1], offs[0], offs[1]) if len(xs) > 1 else None])
    ops.prof_enable(True)
    try:
        L.check(L.lib().unet_conv3x3_bias_relu(dt, n, h, w, src, p(wq), co, p(y), p(sh), relu, st()), "conv3x3 bias relu")
        torch.cuda.synchronize()
    finally:
        ops.prof_collect()
        ops.prof_enable(False)
    return y, set(ops.prof_kernels())


# ------------------------------------------------------------------ many work items per block
# family, bracket, (n, c0, c1, co, h, w), items per launch.  From BIG_CONV_CASES, TWO_SOURCE_CASES and the steady-state
# shapes of test_conv3x3_fused_bn_statistics (test_gpu_kernels.py), with the output widened to at least two channel
# tiles and n reduced to the smallest that keeps the items above one round of a 256-CU device.  The weight-stationary
# kernels walk tile ranges (their bias is per block): n keeps THREE tiles per block, the steady state of their ring.
MANY_ITEM_CASES = [
    ("pdma128 lock-step", "conv3_pdma128_kernel", (3, 128, 0, 256, 128, 128)),        # 192 tiles x 2 = 384 items
    ("pdma128 ping-pong", "conv3_pdma128_kernel", (9, 512, 0, 256, 64, 64)),          # 144 tiles x 2 = 288 items
    ("pdma64x2 pair", "conv3_pdma64_kernel", (2, 128, 0, 192, 128, 128)),             # 128 tiles x 3 = 384 items
    ("pdma64 lock-step", "conv3_pdma64_kernel", (2, 256, 0, 192, 128, 128)),          # 128 tiles x 3 = 384 items
    ("ws16", "conv3_ws_kernel", (10, 64, 0, 128, 128, 64)),                           # 320 tiles x 2 groups, 3 per block
    ("ws ragged frame", "conv3_ws_kernel", (3, 64, 0, 128, 200, 136)),                # 351 tiles x 2 groups, 3 per block
    ("two sources, lock-step", "conv3_pdma128_kernel", (3, 64, 64, 256, 112, 128)),   # 168 tiles x 2 = 336 items
    ("two sources, ping-pong", "conv3_pdma128_kernel", (33, 256, 256, 256, 32, 32)),  # 132 tiles x 2 = 264 items
]


def test_many_item_table_has_more_items_than_blocks():
    """(no GPU) every case exceeds one round of 256 blocks with >= 2 channel tiles"""
    for fam, kern, (n, c0, c1, co, h, w) in MANY_ITEM_CASES:
        tiles = n * cdiv(h, 16) * cdiv(w, 16)
        if "pdma" in kern:
            bn = 128 if co % 128 == 0 else 64
            assert co // bn >= 2 and tiles * (co // bn) > 256, fam
            assert ("ping-pong" in fam) == (bn == 128 and c0 + c1 >= 512), fam
            assert ("pair" in fam) == (bn == 64 and c0 + c1 == 128), fam
        else:
            assert c0 == 64 and c1 == 0 and co // 64 >= 2 and cdiv(tiles * (co // 64), 256) >= 3, fam
            assert ("ragged" in fam) == bool(h % 16 or w % 16), fam


@pytest.mark.gpu
@pytest.mark.parametrize("case", MANY_ITEM_CASES, ids=[c[0].replace(" ", "_").replace(",", "") for c in MANY_ITEM_CASES])
def test_folded_conv_many_work_items(hip, case):
    L, ops = hip
    fam, kern, (n, c0, c1, co, h, w) = case
    t0 = time.time()
    tag = f"inf:{case[2]}"
    srcs = [W.make_input(tag + "x0", (n, c0, h, w))]
    if c1:
        srcs.append(W.make_input(tag + "x1", (n, c1, h, w)))
    ctot = c0 + c1
    wt = W.make_input(tag + "w", (co, ctot, 3, 3)).float() * (1 / (3 * ctot ** 0.5))
    scale, shift = eval_coeffs(L, co, tag)
    y, names = run_folded(L, ops, torch.bfloat16, n, h, w, srcs, (0, 0), wt, scale, shift, co)
    assert names == {kern}, f"{fam}: brackets {names}, expected {kern}"
    ref = R.conv3x3_bias_relu(torch.cat(srcs, 1), wt, scale, shift, torch.bfloat16)
    assert 0.2 < float((ref[0] == 0).double().mean()) < 0.8
    worst = R.assert_bf16(y, ref, f"folded conv, {fam}")
    print(f"\nREF64 inference many-items [{fam}] {case[2]}: worst err/bound {worst:.3f} ({time.time() - t0:.1f} s)", flush=True)


# ------------------------------------------------------------------ the register-staged kernels (frames not 16-aligned)
STAGED_CASES = [  # n, ci, co, h, w
    (1, 128, 64, 9, 21), (2, 192, 128, 7, 13), (1, 256, 192, 20, 17), (1, 256, 128, 17, 35), (1, 192, 64, 33, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", STAGED_CASES, ids=str)
def test_folded_conv_register_staged_kernels(hip, dtype, case):
    """launch3: conv3m16_kernel (bf16, 128-channel tiles) and conv3_kernel (every other form), each with its own epilogue"""
    L, ops = hip
    n, ci, co, h, w = case
    tag = f"inf:staged{case}"
    x = W.make_input(tag + "x", (n, ci, h, w))
    wt = W.make_input(tag + "w", (co, ci, 3, 3)).float() * (1 / (3 * ci ** 0.5))
    scale, shift = eval_coeffs(L, co, tag)
    want = "conv3m16_kernel" if (dtype == torch.bfloat16 and co % 128 == 0) else "conv3_kernel"
    for relu in (1, 0):
        y, names = run_folded(L, ops, dtype, n, h, w, [x], (0, 0), wt, scale, shift, co, relu)
        assert names == {want}, f"brackets {names}, expected {want}"
        ref = R.conv3x3_bias_relu(x, wt, scale, shift, dtype, relu=bool(relu))
        fn = R.assert_bf16 if dtype == torch.bfloat16 else R.assert_fp32
        worst = fn(y, ref, f"folded conv {want} relu={relu}")
        print(f"\nREF64 inference staged [{want} {'bf16' if dtype == torch.bfloat16 else 'fp32'} relu={relu}] {case}: "
              f"worst err/bound {worst:.3f}", flush=True)


# igemm_kernel's 3x3 form (launch<T, 9, BN, KG>): fewer than 64 fp32 / 128 bf16 input channels where the weight-stationary
# kernel does not apply.  n, c0, c1, co, h, w
IGEMM_CASES = [
    (torch.float32, (1, 32, 0, 64, 9, 21)),         # launch<float, 9, 64, 4>
    (torch.float32, (2, 32, 0, 128, 7, 19)),        # launch<float, 9, 128, 4>
    (torch.bfloat16, (1, 32, 32, 64, 9, 21)),       # two sources, 32 + 32: k4 == false -> launch<bf16, 9, 64, 1>
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,case", IGEMM_CASES, ids=[f"{'fp32' if d == torch.float32 else 'bf16'}-{c}" for d, c in IGEMM_CASES])
def test_folded_conv_igemm_kernel(hip, dtype, case):
    L, ops = hip
    n, c0, c1, co, h, w = case
    tag = f"inf:igemm{case}"
    srcs = [W.make_input(tag + "x0", (n, c0, h, w))] + ([W.make_input(tag + "x1", (n, c1, h, w))] if c1 else [])
    wt = W.make_input(tag + "w", (co, c0 + c1, 3, 3)).float() * (1 / (3 * (c0 + c1) ** 0.5))
    scale, shift = eval_coeffs(L, co, tag)
    for relu in (1, 0):
        y, names = run_folded(L, ops, dtype, n, h, w, srcs, (0, 0), wt, scale, shift, co, relu)
        assert names == {"igemm_kernel"}, f"brackets {names}, expected igemm_kernel"
        ref = R.conv3x3_bias_relu(torch.cat(srcs, 1), wt, scale, shift, dtype, relu=bool(relu))
        fn = R.assert_bf16 if dtype == torch.bfloat16 else R.assert_fp32
        worst = fn(y, ref, f"folded conv igemm_kernel relu={relu}")
        print(f"\nREF64 inference staged [igemm_kernel {'bf16' if dtype == torch.bfloat16 else 'fp32'} relu={relu}] {case}: "
              f"worst err/bound {worst:.3f}", flush=True)


# ------------------------------------------------------------------ model level
MODELS = {"anomaly_unet": ("anomaly_unet", 3, 1, False), "unet4": ("unet", 3, 4, False)}
FRAMES = [(256, 256), (256, 320)]
MARGIN_FACTOR = 3.0
MAX_EXCLUDED = 0.01
STAGED = {"conv3_kernel", "conv3m16_kernel", "igemm_kernel"}
PERSISTENT = {"conv3_pdma128_kernel", "conv3_pdma64_kernel", "conv3_ws_kernel"}


def oracle_outputs(name, hw):
    """(state, x, fp32 oracle outputs, e_ref per output)"""
    spec = MODELS[name]
    state = W.make_state(W.state_spec(*spec), 0)
    x = W.make_input(f"inf:image{hw}", (1, 3) + hw)

    def fwd():
        if spec[0] == "unet":
            return (O.unet_forward(state, x, training=False),)
        return O.anomaly_unet_forward(state, x, training=False)
    with torch.no_grad():
        f32 = fwd()
        with O.bf16_storage():
            b16 = fwd()
    return state, x, f32, [float((a - b).abs().max()) for a, b in zip(f32, b16)]


@pytest.mark.gpu
@pytest.mark.parametrize("hw", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(MODELS))
def test_bf16_eval_inference_within_the_oracles_bf16_noise(name, hw):
    import tiaozhanbei_unet_amd as P
    spec = MODELS[name]
    state, x, f32, e_ref = oracle_outputs(name, hw)
    m = P.UNet(spec[1], spec[2], spec[3], precision="bf16") if spec[0] == "unet" else P.AnomalyUNet(spec[1], spec[3], precision="bf16")
    m.load_state_dict(state)
    m = m.to(dev()).eval()
    from tiaozhanbei_unet_amd import ops
    ops.prof_enable(True)
    try:
        with torch.no_grad():
            out = m(x.to(dev()))
        torch.cuda.synchronize()
    finally:
        ops.prof_collect()
        ops.prof_enable(False)
    kernels = set(ops.prof_kernels())
    # the code paths this frame is here for: 256x256 is 16-aligned at every level (persistent kernels only, the 512- and
    # 1024-channel layers of the bottleneck and up1 on conv3_pdma128_kernel's ping-pong form); at 256x320 the 32x40 and
    # 16x20 levels take the register-staged kernels
    assert PERSISTENT <= kernels, (hw, sorted(kernels))
    if hw == (256, 256):
        assert not (STAGED & kernels), (hw, sorted(kernels))
    else:
        assert "conv3m16_kernel" in kernels, (hw, sorted(kernels))
    out = [o.float().cpu() for o in (out if isinstance(out, (tuple, list)) else (out,))]
    names = ("logits",) if spec[0] == "unet" else ("recon", "amap")
    errs = [float((o - r).abs().max()) for o, r in zip(out, f32)]
    for nm, e, er in zip(names, errs, e_ref):
        print(f"\nREF64 inference model [{name} {hw[0]}x{hw[1]}] {nm}: e_ref {er:.3e} library err {e:.3e} = {e / er:.2f} e_ref",
              flush=True)
    if spec[0] == "unet":
        top = f32[0].topk(2, dim=1).values
        margin, got, want = top[:, 0] - top[:, 1], out[0].argmax(1), f32[0].argmax(1)
        e_dec = e_ref[0]
    else:
        margin, got, want = (f32[1] - 0.5).abs(), out[1] > 0.5, f32[1] > 0.5
        e_dec = e_ref[1]
    excluded = margin < 2 * MARGIN_FACTOR * e_dec
    share = float(excluded.double().mean())
    wrong = int(((got != want) & ~excluded).sum())
    print(f"REF64 inference model [{name} {hw[0]}x{hw[1]}] decisions: excluded share {share:.4%}, "
          f"{wrong} disagreements outside it, {int((got != want).sum())} inside or outside", flush=True)
    for nm, e, er in zip(names, errs, e_ref):
        assert er > 0 and e <= MARGIN_FACTOR * er, f"{nm}: library error {e:.3e} > 3 x e_ref {er:.3e}"
    assert share <= MAX_EXCLUDED, f"{share:.3%} of the pixels have an fp32 margin below 6 e_ref"
    assert wrong == 0, f"{wrong} decisions differ from the fp32 oracle outside the excluded pixels"
