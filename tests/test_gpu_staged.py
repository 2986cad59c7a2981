"""The register-staged and generic convolution kernels in their TRAINING forms against float64, element by element.

These kernels carry the whole fp32 ("parity") mode -- conv3_kernel<float> (conv3.hip) for every 3x3 forward and data
gradient, igemm_kernel<float, 1> (igemm.hip) for the transposed convolutions, wgrad_kernel<float, 9 | 4> and the two
reduce kernels (wgrad.hip) for every weight gradient -- and, in bf16, every layer with >= 128 input channels on a frame
that is not 16-aligned (conv3m16_kernel, conv3_kernel<bf16>), the igemm_kernel<T, 9> fallback and the KG == 1
instantiations.  Their tile is 8 x 16 pixels x 128 or 64 channels; the shapes below are the smallest that give several
tiles in both directions with a ragged right AND bottom edge, a frame smaller than one tile, N > 1, two or more channel
tiles and four or more K chunks.  Inputs are zero-mean and NOT pre-rounded to bf16: the fp32 kernels are held to 2^-18 S
on unrounded operands (see _ref64.py), the bf16 kernels to half a bf16 ulp + 2^-18 S on the operands as they read them.

Each case runs at the CU budgets {full, 8} (the weight-gradient split depends on it, nothing else may) and asserts:
  * the profiling bracket (and the launches per kernel class) are the expected ones: a case cannot move to another kernel;
  * every output against the float64 reference of its own dtype; accumulate forms against (old + ref, |old| + S) with
    `old` read back before the call;
  * unet_conv3x3_stats: 0 < n_parts <= the cap, the partial rows summed in float64 are the sums of the STORED y (so the
    pixels of an edge tile outside the frame add nothing), the rows past n_parts are untouched, y equals the plain call's;
  * no store outside a buffer: every output, partials buffer and workspace sits between sentinel margins, the workspaces
    sized to exactly what the query returns, and the part of a workspace past the slabs the launch needs stays untouched;
  * a second run is bit-identical; forward and data-gradient outputs are bit-identical across budgets, weight gradients
    agree within the fp32 bound.
route() restates dispatch<> (conv_api.hip), unet_internal_conv3 / launch3 (conv3.hip) and make_plan<TAPS> / run<>
(wgrad.hip) as integer formulas; test_staged_table_reaches_every_instantiation (no GPU) asserts what the table reaches.
"""
import ctypes as C
import os
import time

import pytest
import torch
import torch.nn.functional as F

import _ref64 as R
from oracle import weights as W
from test_gpu_partition import Guards, budget, budget_value, cdiv, dev, hip, p, st, views      # noqa: F401  (fixtures)

gpu = pytest.mark.gpu              # per test, not a module-level pytestmark: the table test below needs no GPU
BUDGETS = ("full", 8)
BF, FP = torch.bfloat16, torch.float32
DN = {BF: "bf16", FP: "fp32"}


def S_(n, c0, co, h, w, c1=0, **kw):
    return dict(n=n, c0=c0, c1=c1, co=co, h=h, w=w, **kw)


A = S_(2, 128, 128, 20, 40)                       # 3 x 3 tiles, both edges ragged, one 128-channel tile
TWO = S_(2, 64, 128, 19, 37, c1=64, h1=14, w1=30, oy=2, ox=3)
M16, C3, IG, WG = "conv3m16_kernel", "conv3_kernel", "igemm_kernel", "wgrad_kernel (+ reduce)"

# family, dtype, shape, expected bracket(s).  conv / two / convt: (forward, data gradient).  Shapes: n, c0 [+ c1], co, h, w
# (convt / convt_wgrad: c0 -> co channels, h x w the INPUT frame).
CASES = [
    # ---- unet_conv3x3, plain forward and plain data gradient
    ("conv", FP, A, (C3, C3)),
    ("conv", FP, S_(1, 256, 192, 17, 35), (C3, C3)),          # three 64-channel tiles (dgrad: two 128-channel tiles)
    ("conv", FP, S_(3, 128, 256, 7, 13), (C3, C3)),           # a frame inside one tile, two channel tiles
    ("conv", FP, S_(2, 256, 128, 88, 32), (C3, C3)),          # the Kolektor bottleneck frame
    ("conv", FP, S_(1, 64, 64, 32, 32), (C3, C3)),            # fp32 takes this family on aligned frames too
    ("conv", BF, A, (M16, M16)),
    ("conv", BF, S_(1, 256, 192, 17, 35), (C3, M16)),         # conv3_kernel<bf16, 64, 4> forward
    ("conv", BF, S_(3, 128, 256, 7, 13), (M16, M16)),
    ("conv", BF, S_(2, 256, 128, 88, 32), (M16, M16)),        # four bf16 chunks
    # ---- unet_conv3x3_stats: the conv3m16_kernel epilogue (bf16), the streaming fallback behind conv3_kernel (fp32)
    ("stats", FP, A, C3), ("stats", FP, S_(3, 128, 256, 7, 13), C3),
    ("stats", BF, A, M16), ("stats", BF, S_(3, 128, 256, 7, 13), M16),
    # ---- two sources at a centre-pad offset; two-destination data gradient with accumulate 0..3
    ("two", FP, TWO, (C3, C3)), ("two", BF, TWO, (M16, M16)),
    # ---- KG == 1 (channel counts that are multiples of 8 / 16 but not of 32 / 64): forward and accumulate = 1
    ("kg1", FP, S_(1, 72, 64, 9, 21), C3), ("kg1", FP, S_(1, 40, 128, 9, 21, c1=32), C3),
    ("kg1", BF, S_(1, 144, 128, 9, 21), C3), ("kg1", BF, S_(1, 80, 64, 9, 21, c1=64), C3),
    # ---- igemm_kernel<T, 9>, plain forward (the cases test_gpu_inference.py uses for the folded form)
    ("igemm9", FP, S_(1, 32, 64, 9, 21), IG), ("igemm9", FP, S_(2, 32, 128, 7, 19), IG),
    ("igemm9", BF, S_(1, 32, 64, 9, 21, c1=32), IG),
    # ---- unet_convt2x2_fwd / _dgrad on igemm_kernel<T, 1>: pixel-shuffle scatter + bias, four-tap gather
    ("convt", FP, S_(2, 128, 64, 5, 9), (IG, IG)), ("convt", FP, S_(1, 256, 128, 8, 16), (IG, IG)),
    ("convt", BF, S_(2, 128, 128, 5, 9), (IG, IG)),           # c_in != 2 c_out: not the streaming kernels
    # (the GEMM rows of the cases above, 4 c_out and c_in, are all multiples of 128: a 64-channel input adds the 64-row
    #  tile of the data gradient, igemm_kernel<T, 1, 64, 4>)
    ("convt", FP, S_(1, 64, 64, 5, 9), (IG, IG)), ("convt", BF, S_(1, 64, 64, 5, 9), (IG, IG)),
    # ---- unet_conv3x3_wgrad, fp32
    ("wgrad", FP, A, WG),                                     # 18 tiles: split 18 wide at full, 4 narrow (5 tiles each) at 8
    ("wgrad", FP, S_(3, 64, 64, 7, 13), WG),                  # 3 blocks: no xcd_chunk
    ("wgrad", FP, S_(5, 256, 256, 17, 35), WG),               # K = 2975; 4 x 4 channel tiles, split 23 of 2 tiles, 1 at 8
    ("wgrad", FP, S_(2, 64, 64, 12, 20, cparam=3), WG),       # the image layer: 3 channels padded to 64, dw[64][3][3][3]
    ("wgrad", FP, TWO, WG),
    # ---- unet_convt2x2_wgrad (+ the unet_internal_colsum bias gradient on the slab workspace)
    ("convt_wgrad", FP, S_(2, 128, 64, 5, 9), WG), ("convt_wgrad", FP, S_(1, 256, 128, 8, 16), WG),
    ("convt_wgrad", BF, S_(1, 128, 64, 9, 20), WG),
]


def case_id(c):
    s = c[2]
    ch = f"{s['c0']}+{s['c1']}" if s["c1"] else str(s["c0"])
    return f"{c[0]}-{DN[c[1]]}-{s['n']}x{ch}x{s['co']}x{s['h']}x{s['w']}"


IDS = [case_id(c) for c in CASES]


# ------------------------------------------------------------------ restatement of the dispatch (coverage, no GPU)
def conv3_route(dt, c0, c1, cout, h, w):
    """dispatch<T, 9> (conv_api.hip) + unet_internal_conv3 / launch3 (conv3.hip) -> (bracket, instantiation)"""
    kgc = 16 if dt == BF else 8
    ck4, ctot = 4 * kgc, c0 + c1
    assert cout % 64 == 0 and ctot % kgc == 0
    bn = 128 if cout % 128 == 0 else 64
    k4 = ctot % ck4 == 0 and (c1 == 0 or c0 % ck4 == 0)
    assert k4 or c1 == 0 or c0 % kgc == 0
    kg = 4 if k4 else 1
    if dt == BF:
        if ctot == 64 and c1 == 0:
            return "conv3_ws_kernel", "specialised"
        if k4 and ctot >= 128 and h % 16 == 0 and w % 16 == 0:
            return "conv3_pdma_kernel", "specialised"
    if ctot >= 2 * ck4:
        if dt == BF and bn == 128 and kg == 4:
            return M16, "launch3<bf16,128,4>"
        return C3, f"launch3<{DN[dt]},{bn},{kg}>"
    return IG, f"igemm<{DN[dt]},9,{bn},{kg}>"


def convt_route(dt, mode, ci, co):
    """unet_convt2x2_fwd / _dgrad (conv_api.hip) + dispatch<T, 1> -> (bracket, instantiation)"""
    if dt == BF and ci == 2 * co and (ci in (128, 256) if mode == "fwd" else co in (64, 128)):
        return "convt_ws_kernel", "specialised"
    if dt == BF and (co % 256 == 0 and ci >= 128 if mode == "fwd" else ci % 256 == 0 and co >= 64):
        return "convt_gemm_kernel", "specialised"
    ctot, cout = (ci, 4 * co) if mode == "fwd" else (co, ci)
    ck4 = 64 if dt == BF else 32
    assert ctot % ck4 == 0
    return IG, f"igemm<{DN[dt]},1,{128 if cout % 128 == 0 else 64},4>"


def wgrad_plan(taps, n, h, w, crow, ccol, bud):
    """make_plan<TAPS> + run<> (wgrad.hip) -> dict(split, tps, blocks, bytes)"""
    tx, ty = cdiv(w, 16), cdiv(h, 8 if taps == 9 else 4)
    nr, nc = crow // 64, ccol // 64
    ntiles = n * ty * tx
    want = min(max(1, 2 * bud // (nr * nc)), ntiles)
    tps = cdiv(ntiles, want)
    split = cdiv(ntiles, tps)
    return dict(split=split, tps=tps, blocks=split * nr * nc, bytes=split * taps * crow * ccol * 4)


def route(case, bud):
    """the instantiations and budget branches a case reaches at CU budget `bud`: set of tags"""
    fam, dt, s, _ = case
    c0, c1, co, h, w = s["c0"], s["c1"], s["co"], s["h"], s["w"]
    if fam in ("conv", "two"):
        return {conv3_route(dt, c0, c1, co, h, w), conv3_route(dt, co, 0, c0 + c1, h, w)}
    if fam in ("stats", "kg1", "igemm9"):
        return {conv3_route(dt, c0, c1, co, h, w)}
    if fam == "convt":
        return {convt_route(dt, "fwd", c0, co), convt_route(dt, "dgrad", c0, co)}
    taps = 9 if fam == "wgrad" else 4
    crow, ccol = (co, c0 + c1) if fam == "wgrad" else (c0, co)
    if fam == "wgrad" and dt == BF:
        return {("wgrad16 / wgrad_dma", "specialised")}
    if fam == "convt_wgrad" and dt == BF and c0 in (128, 256, 512, 1024) and 2 * co == c0 and \
            (w % 32 == 0 or (w == 16 and h % 2 == 0)) and (s["n"] * h * w) % 32 == 0:
        return {("convt_wgrad_ws_kernel", "specialised")}
    pl = wgrad_plan(taps, s["n"], h, w, crow, ccol, bud)
    return {(WG, f"wgrad<{DN[dt]},{taps}>"), (WG, "reduce_wide" if pl["split"] >= 16 else "reduce_narrow"),
            (WG, "xcd_chunk" if pl["blocks"] >= 16 else "no_xcd_chunk"),
            (WG, "tiles_per_split>1" if pl["tps"] > 1 else "tiles_per_split1")}


def test_staged_table_reaches_every_instantiation():
    """(no GPU) the table, at budgets {full, 8} of a 256-CU device, reaches every instantiation of the register-staged and
    generic kernels, names the bracket dispatch<> selects, and no case qualifies for a specialised family"""
    seen = set()
    for case in CASES:
        fam, dt, s, want = case
        for b in BUDGETS:
            r = route(case, budget_value(b, 256))
            assert all(inst != "specialised" for _, inst in r), (case_id(case), r)
            seen |= {inst for _, inst in r}
        if fam in ("conv", "two"):
            got = (conv3_route(dt, s["c0"], s["c1"], s["co"], s["h"], s["w"])[0],
                   conv3_route(dt, s["co"], 0, s["c0"] + s["c1"], s["h"], s["w"])[0])
        elif fam == "convt":
            got = (convt_route(dt, "fwd", s["c0"], s["co"])[0], convt_route(dt, "dgrad", s["c0"], s["co"])[0])
        else:
            (got,) = {k for k, _ in route(case, 256)}
        assert got == want, (case_id(case), got, want)
    want = {f"launch3<{t},{bn},{kg}>" for t in ("fp32", "bf16") for bn in (128, 64) for kg in (4, 1)}
    want |= {"igemm<fp32,9,64,4>", "igemm<fp32,9,128,4>", "igemm<bf16,9,64,1>"}
    want |= {f"igemm<{t},1,{bn},4>" for t in ("fp32", "bf16") for bn in (128, 64)}
    want |= {"wgrad<fp32,9>", "wgrad<fp32,4>", "wgrad<bf16,4>", "reduce_wide", "reduce_narrow", "xcd_chunk", "no_xcd_chunk",
             "tiles_per_split>1", "tiles_per_split1"}
    assert want <= seen, sorted(want - seen)
    for fam, dt, s, _ in CASES:
        # ragged frames for every bf16 3x3 case with >= 128 input channels (else it would be a persistent kernel's)
        if fam in ("conv", "stats", "two") and dt == BF:
            assert s["h"] % 16 or s["w"] % 16
        if fam in ("wgrad", "convt_wgrad"):
            assert s["n"] * s["h"] * s["w"] <= R.MAX_WGRAD_K
        assert s["n"] * max(s["c0"] + s["c1"], s["co"]) * s["h"] * s["w"] <= 2 * 256 * 88 * 32      # tests stay quick
    # the statistics cases: one that is mostly out-of-frame pixels of its only tile
    assert any(f == "stats" and s["h"] < 8 and s["w"] < 16 for f, _, s, _ in CASES)


# ------------------------------------------------------------------ inputs and references
def inp(tag, shape, scale=1.0):
    """zero-mean fp32, NOT rounded to bf16"""
    return W.make_input("staged:" + tag, shape) * scale


def to_nhwc(t, dt):
    return t.to(dev()).to(dt).contiguous(memory_format=torch.channels_last)


def cat_sources(s, x0, x1):
    if x1 is None:
        return x0
    oy, ox = s.get("oy", 0), s.get("ox", 0)
    return torch.cat([x0, F.pad(x1, [ox, s["w"] - x1.shape[3] - ox, oy, s["h"] - x1.shape[2] - oy])], 1)


def kind(dt):
    return "bf16" if dt == BF else "fp32"


class Step:
    """one launch form of a case: alloc(G, bv) -> guarded buffers o, call(o) launches (and may note results in o),
    after(o, earlier, at) -> [(what, offset, length)] ranges inside a buffer that must be untouched (earlier: the host
    outputs of the steps before this one at the same budget), refs(o) -> {name: (ref, S, kind)} evaluated after the launch;
    exact: the outputs do not depend on the budget"""

    def __init__(self, name, bracket, classes, alloc, call, refs, after=None, exact=True):
        self.name, self.bracket, self.classes = name, bracket, classes
        self.alloc, self.call, self.refs, self.after, self.exact = alloc, call, refs, after, exact


def drive(hipmod, budget, steps, label):
    """run every step at every budget, twice; all the assertions of the module docstring; prints the REF64 line"""
    L, ops = hipmod
    full, set_budget = budget
    t0 = time.time()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    worst, first = {}, {}
    for b in BUDGETS:
        bv = set_budget(b)
        earlier = {}
        for step in steps:
            runs = []
            for rep in range(2):
                G = Guards()
                o = step.alloc(G, bv)
                torch.cuda.synchronize()
                ops.prof_enable(True)
                try:
                    step.call(o)
                    torch.cuda.synchronize()
                finally:
                    cls = ops.prof_collect()
                    ops.prof_enable(False)
                at = f"[{label} budget {bv}] {step.name}"
                names = set(ops.prof_kernels())
                assert names == {step.bracket}, f"{at}: brackets {names}, expected {step.bracket}"
                launches = {k: v["launches"] for k, v in cls.items() if v["launches"]}
                assert launches == step.classes, f"{at}: launches per class {launches}, expected {step.classes}"
                G.check(step.after(o, earlier, at) if step.after else [])
                refs = step.refs(o)
                host = {k: o[k].detach().cpu().clone() for k in refs}
                runs.append((host, refs))
            (host, refs), (again, _) = runs
            for k in host:
                assert torch.equal(host[k], again[k]), f"{at} {k}: the second run differs"
            earlier[step.name] = host
            for k, (r, S, kd) in refs.items():
                if step.name in first and step.exact:
                    assert torch.equal(host[k], first[step.name][k]), \
                        f"{at} {k}: differs from budget {full} (must not depend on the budget)"
                    continue
                fn = R.assert_bf16 if kd == "bf16" else R.assert_fp32
                got = fn(host[k].float(), (r, S), f"{at} {k}")
                key = f"{step.name}.{k}"
                worst[key] = max(worst.get(key, 0.0), got)
                if step.name in first:
                    R.assert_fp32(host[k].double(), (first[step.name][k].double(), 2 * S), f"{at} {k} vs budget {full}")
            first.setdefault(step.name, host)
    print(f"\nREF64 staged [{label}] worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f" ({time.time() - t0:.1f} s)", flush=True)


def conv_step(L, ops, name, bracket, kclass, dt, s, srcs, offs, wp, cout, dst_shapes, split, acc, refs, old=None):
    """unet_conv3x3 on guarded destinations.  dst_shapes: [(c, h, w, oy, ox)]; old: fp32 CPU tensors the destinations
    hold before the call (read back from the device in the compute dtype: the accumulate reference adds them)"""
    n, h, w = s["n"], s["h"], s["w"]
    names = ["d0", "d1"][:len(dst_shapes)]

    def alloc(G, bv):
        o = {}
        for i, (nm, (c, dh, dw, _, _)) in enumerate(zip(names, dst_shapes)):
            o[nm] = G.nhwc(n, c, dh, dw, nm, fill=None if old is None else old[i].to(dev()), dtype=dt)
            if old is not None:
                o["old_" + nm] = o[nm].double().cpu()
        return o

    def call(o):
        dst = views(L, [(o[nm], sh[3], sh[4]) for nm, sh in zip(names, dst_shapes)] + [None] * (2 - len(names)))
        src = views(L, [(srcs[0], 0, 0), (srcs[1], offs[0], offs[1]) if len(srcs) > 1 else None])
        L.check(L.lib().unet_conv3x3(ops._DT[dt], n, h, w, src, p(wp), cout, dst, split, acc, kclass, st()), name)

    def get_refs(o):
        out = {}
        for i, nm in enumerate(names):
            r, S = refs[i]
            if acc & (1 << i):
                r, S = r + o["old_" + nm], S + o["old_" + nm].abs()
            out[nm] = (r, S, kind(dt))
        return out
    cls = {L.KCLASS_NAMES[kclass]: 1}
    return Step(name, bracket, cls, alloc, call, get_refs)


def sources(s, dt, tag):
    """(CPU fp32 sources, their concatenation in the frame, device NHWC sources, (oy, ox) of the second)"""
    n, h, w = s["n"], s["h"], s["w"]
    x0 = inp(tag + "x0", (n, s["c0"], h, w))
    x1 = inp(tag + "x1", (n, s["c1"], s.get("h1", h), s.get("w1", w))) if s["c1"] else None
    cpu = [x0] + ([x1] if x1 is not None else [])
    return cpu, cat_sources(s, x0, x1), [to_nhwc(t, dt) for t in cpu], (s.get("oy", 0), s.get("ox", 0))


# ------------------------------------------------------------------ the families
def steps_conv3(L, ops, case):
    """conv / two / kg1 / igemm9 / stats"""
    fam, dt, s, want = case
    n, c0, c1, co, h, w = s["n"], s["c0"], s["c1"], s["co"], s["h"], s["w"]
    ctot = c0 + c1
    tag = case_id(case)
    cpu, xs, xd, offs = sources(s, dt, tag)
    wt = inp(tag + "w", (co, ctot, 3, 3), 1 / (3 * ctot ** 0.5))
    wd = wt.to(dev())
    wp = ops.pack_weight(wd, L.PACK_CONV_FWD, co, ctot, dt)
    fwd_b = want[0] if isinstance(want, tuple) else want
    yref = R.conv3x3(xs, wt, dtype=dt)
    full = [(co, h, w, 0, 0)]
    steps = [conv_step(L, ops, "fwd", fwd_b, L.K_CONV_FWD, dt, s, xd, offs, wp, co, full, co, 0, [yref])]
    if fam == "kg1":
        old = [inp(tag + "old", (n, co, h, w))]
        steps.append(conv_step(L, ops, "fwd_acc1", fwd_b, L.K_CONV_FWD, dt, s, xd, offs, wp, co, full, co, 1, [yref], old))
    if fam == "stats":
        steps.append(stats_step(L, ops, fwd_b, dt, s, xd, offs, wp, yref))
    if fam in ("conv", "two"):
        gy = inp(tag + "gy", (n, co, h, w))
        gd = [to_nhwc(gy, dt)]
        wpd = ops.pack_weight(wd, L.PACK_CONV_DGRAD, ctot, co, dt)
        r, S = R.conv3x3_dgrad(gy, wt, dtype=dt)
        if fam == "conv":
            steps.append(conv_step(L, ops, "dgrad", want[1], L.K_CONV_DGRAD, dt, s, gd, (0, 0), wpd, ctot,
                                   [(ctot, h, w, 0, 0)], ctot, 0, [(r, S)]))
        else:
            oy, ox, h1, w1 = s["oy"], s["ox"], s["h1"], s["w1"]
            refs = [(r[:, :c0], S[:, :c0]), (r[:, c0:, oy:oy + h1, ox:ox + w1], S[:, c0:, oy:oy + h1, ox:ox + w1])]
            old = [inp(tag + "old0", (n, c0, h, w)), inp(tag + "old1", (n, c1, h1, w1))]
            for acc in (0, 1, 2, 3):
                steps.append(conv_step(L, ops, f"dgrad_acc{acc}", want[1], L.K_CONV_DGRAD, dt, s, gd, (0, 0), wpd, ctot,
                                       [(c0, h, w, 0, 0), (c1, h1, w1, oy, ox)], c0, acc, refs, old))
    return steps


def stats_step(L, ops, bracket, dt, s, xd, offs, wp, yref):
    n, co, h, w = s["n"], s["co"], s["h"], s["w"]
    lib = L.lib()
    cap = lib.unet_conv3x3_stats_max_parts(n, h, w)
    fused = bracket == M16
    row = 2 * co

    def alloc(G, bv):
        return {"y": G.nhwc(n, co, h, w, "y", dtype=dt), "partials": G.alloc(cap * row, torch.float32, "partials")}

    def call(o):
        nparts = C.c_int32(-1)
        src = views(L, [(xd[0], 0, 0), (xd[1], offs[0], offs[1]) if len(xd) > 1 else None])
        L.check(lib.unet_conv3x3_stats(ops._DT[dt], n, h, w, src, p(wp), co, p(o["y"]), p(o["partials"]), C.byref(nparts),
                                       st()), "stats")
        o["n_parts"] = nparts.value

    def after(o, earlier, at):
        np_ = o["n_parts"]
        assert 0 < np_ <= cap, f"{at}: n_parts {np_} outside (0, {cap}]"
        if fused:
            assert np_ == n * cdiv(h, 8) * cdiv(w, 16), f"{at}: n_parts {np_} is not N tilesY tilesX"
        assert torch.equal(o["y"].cpu(), earlier["fwd"]["d0"]), f"{at}: y differs from the plain call's"
        return [("partials", np_ * row, (cap - np_) * row)]

    def refs(o):
        """y as the plain call; the partial rows summed in float64 = sum y, sum y^2 of the STORED y (frame pixels only)"""
        o["sums"] = o["partials"][:o["n_parts"] * row].view(-1, 2, co).double().sum(0)
        yd = o["y"].double().cpu()
        s0, s1 = R.sums_over_pixels(yd), R.sums_over_pixels(yd * yd)
        return {"y": yref + (kind(dt),), "sums": (torch.stack([s0[0], s1[0]]), torch.stack([s0[1], s1[1]]), "fp32")}

    step = Step("stats", bracket, {"conv3x3_fwd": 1} if fused else {"conv3x3_fwd": 1, "bn": 1}, alloc, call, refs, after)
    return step


def steps_convt(L, ops, case):
    fam, dt, s, want = case
    n, ci, co, h, w = s["n"], s["c0"], s["co"], s["h"], s["w"]
    tag = case_id(case)
    lib = L.lib()
    x, wt, b = inp(tag + "x", (n, ci, h, w)), inp(tag + "w", (ci, co, 2, 2), 0.1), inp(tag + "b", (co,), 0.5)
    gy = inp(tag + "gy", (n, co, 2 * h, 2 * w))
    xd, gd, wd, bd = to_nhwc(x, dt), to_nhwc(gy, dt), wt.to(dev()), b.to(dev()).contiguous()
    wpf = ops.pack_weight(wd, L.PACK_CONVT_FWD, co, ci, dt)
    wpd = ops.pack_weight(wd, L.PACK_CONVT_DGRAD, ci, co, dt)
    yref, dref = R.convt2x2(x, wt, b, dtype=dt), R.convt2x2_dgrad(gy, wt, dtype=dt)

    def call_f(o):
        L.check(lib.unet_convt2x2_fwd(ops._DT[dt], n, h, w, p(xd), ci, p(wpf), p(bd), p(o["y"]), co, st()), "convt fwd")

    def call_d(o):
        L.check(lib.unet_convt2x2_dgrad(ops._DT[dt], n, h, w, p(gd), co, p(wpd), p(o["dx"]), ci, st()), "convt dgrad")
    return [Step("fwd", want[0], {"convt_fwd": 1}, lambda G, bv: {"y": G.nhwc(n, co, 2 * h, 2 * w, "y", dtype=dt)}, call_f,
                 lambda o: {"y": yref + (kind(dt),)}),
            Step("dgrad", want[1], {"convt_dgrad": 1}, lambda G, bv: {"dx": G.nhwc(n, ci, h, w, "dx", dtype=dt)}, call_d,
                 lambda o: {"dx": dref + (kind(dt),)})]


def steps_wgrad(L, ops, case):
    fam, dt, s, want = case
    n, c0, c1, co, h, w = s["n"], s["c0"], s["c1"], s["co"], s["h"], s["w"]
    ctot, cpar = c0 + c1, s.get("cparam", c0 + c1)
    tag = case_id(case)
    lib = L.lib()
    if "cparam" in s:        # the image layer: 3 channels, zero-padded to 64 by unet_nchw_to_nhwc
        img = inp(tag + "x0", (n, cpar, h, w))
        xd0 = torch.empty((n, c0, h, w), dtype=dt, device=dev()).contiguous(memory_format=torch.channels_last)
        imgd = img.to(dev()).contiguous()
        L.check(lib.unet_nchw_to_nhwc(p(imgd), p(xd0), n, cpar, h, w, c0, ops._DT[dt], st()), "pack image")
        xs, xd, offs = img, [xd0], (0, 0)
        back = xd0.float().cpu()
        assert torch.equal(back[:, :cpar], img) and float(back[:, cpar:].abs().max()) == 0.0
    else:
        _, xs, xd, offs = sources(s, dt, tag)
    gy = inp(tag + "gy", (n, co, h, w))
    gd = to_nhwc(gy, dt)
    ref = R.conv3x3_wgrad(xs, gy, dtype=dt)
    ref = (ref[0][:, :cpar], ref[1][:, :cpar])
    need = {}

    def alloc(G, bv):
        need[0] = lib.unet_conv3x3_wgrad_workspace(n, h, w, ctot, co)
        return {"dw": G.alloc(co * cpar * 9, torch.float32, "dw").view(co, cpar, 3, 3),
                "workspace": G.alloc(need[0], torch.uint8, "workspace"), "bv": bv}

    def call(o):
        src = views(L, [(xd[0], 0, 0), (xd[1], offs[0], offs[1]) if len(xd) > 1 else None])
        L.check(lib.unet_conv3x3_wgrad(ops._DT[dt], n, h, w, src, p(gd), co, p(o["dw"]), cpar, p(o["workspace"]), need[0],
                                       st()), "wgrad")

    def after(o, earlier, at):
        used = wgrad_plan(9, n, h, w, co, ctot, o["bv"])["bytes"]
        assert used <= need[0], f"{at}: the launch needs {used} bytes of slabs, the query returned {need[0]}"
        return [("workspace", used, need[0] - used)]
    return [Step("wgrad", want, {"conv3x3_wgrad": 1}, alloc, call, lambda o: {"dw": ref + ("fp32",)}, after, exact=False)]


def steps_convt_wgrad(L, ops, case):
    fam, dt, s, want = case
    n, ci, co, h, w = s["n"], s["c0"], s["co"], s["h"], s["w"]
    tag = case_id(case)
    lib = L.lib()
    x, gy = inp(tag + "x", (n, ci, h, w)), inp(tag + "gy", (n, co, 2 * h, 2 * w))
    xd, gd = to_nhwc(x, dt), to_nhwc(gy, dt)
    rw, rb = R.convt2x2_wgrad(x, gy, dtype=dt)
    need = {}

    def alloc(G, bv):
        need[0] = lib.unet_convt2x2_wgrad_workspace(n, h, w, ci, co)
        return {"dw": G.alloc(ci * co * 4, torch.float32, "dw").view(ci, co, 2, 2), "db": G.alloc(co, torch.float32, "db"),
                "workspace": G.alloc(need[0], torch.uint8, "workspace"), "bv": bv}

    def call(o):
        L.check(lib.unet_convt2x2_wgrad(ops._DT[dt], n, h, w, p(xd), ci, p(gd), co, p(o["dw"]), p(o["db"]),
                                        p(o["workspace"]), need[0], st()), "convt wgrad")

    def after(o, earlier, at):
        # the query has no dtype: it is the larger of make_plan<4> and the bf16 streaming kernel's slabs.  The split-K
        # slabs of this launch (and the column sums of the bias gradient, which reuse their first bytes) end at `used`
        used = wgrad_plan(4, n, h, w, ci, co, o["bv"])["bytes"]
        assert used <= need[0], f"{at}: the launch needs {used} bytes of slabs, the query returned {need[0]}"
        return [("workspace", used, need[0] - used)]
    return [Step("wgrad", want, {"convt_wgrad": 1}, alloc, call, lambda o: {"dw": rw + ("fp32",), "db": rb + ("fp32",)},
                 after, exact=False)]


BUILD = {"conv": steps_conv3, "two": steps_conv3, "kg1": steps_conv3, "igemm9": steps_conv3, "stats": steps_conv3,
         "convt": steps_convt, "wgrad": steps_wgrad, "convt_wgrad": steps_convt_wgrad}


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_staged_kernel_training_forms(hip, budget, case):
    L, ops = hip
    steps = BUILD[case[0]](L, ops, case)
    torch.cuda.synchronize()
    drive(hip, budget, steps, case_id(case))
