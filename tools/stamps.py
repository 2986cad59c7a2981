#!/usr/bin/env python3
"""Diagnostic: where do the cycles of a stamped kernel go?  Needs the stamps build of the library:

    make -C tiaozhanbei_unet_amd/csrc stamps      (-> libunet_hip_stamps.so, s_memtime stamps: csrc/stamps.h)
    UNET_HIP_LIB=tiaozhanbei_unet_amd/libunet_hip_stamps.so python tools/stamps.py pdma 32 512 512 32 32
    UNET_HIP_LIB=...                                 python tools/stamps.py ws16 32 64 64 256 256 [--stats]
    UNET_HIP_LIB=...                                 python tools/stamps.py wgrad 32 256 256 64 64

pdma: conv3_pdma*_kernel / conv3_pp*_kernel (forward 3x3 convolution, N CIN COUT H W); ws16: conv3_ws16_kernel, with
--stats the form that also writes BatchNorm partial sums; wgrad: wgrad_dma_kernel, or wgrad16_kernel where COUT is a
multiple of 128.  Prints, per wave class, the mean cycles per tap (pdma) or per tile spent in each phase, its share of
their total, and the in-kernel clock.  (Stamps cost ~10 % themselves: read shares, not absolutes.)

A record is eight uint64 per wave: laps [0..5], count [6] (taps or tiles), clock [7] = the shader clock in units of
100 MHz, x 2^20.  decode() turns records into rows and needs neither torch nor a GPU."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

# kind -> (what a count is, lap names by lap index (None: not a phase of the loop), wave classes,
#          extras: name -> (lap, per count?) printed beside the phases)
HALVES = (("waves 0-3", slice(0, 4)), ("waves 4-7", slice(4, 8)))
WGRAD_LAPS = ("vmcnt(0) wait", "barrier", "dma issue", "fragment reads + mfma", None, None)
KINDS = {
    "pdma": ("tap", ("vmcnt wait", "barrier", "dma issue", "reads+mfma", None, None), HALVES,
             {"epilogue/launch": (4, False)}),
    "pdma_pp": ("tap", ("reads+dma issue", "vmcnt+lgkm wait", "barrier(L)", "mfma", None, "barrier(C)"), HALVES,
                {"of which fragment-read issue/tap": (4, True)}),
    "ws16": ("tile", ("vmcnt wait", "barrier", "top: dma / deferred stores / geometry", "mfma loop", "late dma",
                      "epilogue + stores"), HALVES, {}),
    "wgrad_dma": ("tile", WGRAD_LAPS, (("all waves", slice(None)),), {}),
    "wgrad16": ("tile", WGRAD_LAPS, (("dY waves (DMA mid-tile)", slice(0, 4)), ("X waves (DMA at tile start)", slice(4, 8))),
                {"partial-slab stores (drained)": (4, False), "kernel body": (5, False)}),
}


def decode(kind, records):
    """records: [blocks, waves, 8] -> one row per wave class: {"waves": its label, "records": how many were used,
    "count": mean taps or tiles per wave, "clock_ghz": median in-kernel clock, "laps": {name: mean cycles per count},
    "extras": {name: cycles}}.  Records whose count is 0 (a block that never ran or lay beyond the buffer) are left out;
    a class without any record gives no row."""
    _, names, classes, extras = KINDS[kind]
    records = np.asarray(records).astype(np.float64)
    rows = []
    for label, sl in classes:
        r = records[:, sl, :].reshape(-1, 8)
        r = r[r[:, 6] > 0]
        if not len(r):
            continue
        rows.append({
            "waves": label, "records": len(r), "count": float(r[:, 6].mean()),
            "clock_ghz": float(np.median(r[:, 7])) / 2 ** 20 * 0.1,
            "laps": {nm: float((r[:, i] / r[:, 6]).mean()) for i, nm in enumerate(names) if nm},
            "extras": {nm: float((r[:, i] / (r[:, 6] if per else 1.0)).mean()) for nm, (i, per) in extras.items()},
        })
    return rows


def report(kind, rows):
    """the printed lines of rows"""
    unit = KINDS[kind][0]
    lines = []
    for row in rows:
        total = sum(row["laps"].values())
        lines.append(f"  {row['waves']}: " +
                     "  ".join(f"{nm} {v:7.0f} ({100 * v / total:4.1f}%)" for nm, v in row["laps"].items()) +
                     f"   total/{unit} {total:.0f} cyc" +
                     "".join(f";  {nm} {v:.0f} cyc" for nm, v in row["extras"].items()))
    return lines


def bind_setter(handle):
    """unet_debug_set_buffer of a ctypes handle of the library; it exists in the stamps build only"""
    try:
        setter = handle.unet_debug_set_buffer
    except AttributeError:
        raise SystemExit("stamps.py: this library has no unet_debug_set_buffer: build the stamps library (make stamps "
                         "in tiaozhanbei_unet_amd/csrc) and point UNET_HIP_LIB at libunet_hip_stamps.so") from None
    setter.argtypes, setter.restype = [C.c_void_p, C.c_int64], None
    return setter


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("kernel", choices=["pdma", "ws16", "wgrad"])
    ap.add_argument("dims", type=int, nargs=5, metavar="N CIN COUT H W".split())
    ap.add_argument("--stats", action="store_true", help="ws16: the form that writes BatchNorm partial sums")
    ap.add_argument("--records", type=int, default=1024, help="room in the stamp buffer, in blocks (default 1024)")
    args = ap.parse_args(argv)
    n, ci, co, h, w = args.dims

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tiaozhanbei_unet_amd import _lib as L, ops

    dev, dt = torch.device("cuda:0"), torch.bfloat16
    lib = L.lib()
    setter = bind_setter(C.CDLL(L.LIB_PATH))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.randn(n, ci, h, w, device=dev).to(dt).contiguous(memory_format=torch.channels_last)
    xv = ops._views([(x, 0, 0), None])
    # per kernel family: the launch, the record kind, waves per block, the headline
    if args.kernel == "wgrad":
        gy = torch.randn(n, co, h, w, device=dev).to(dt).contiguous(memory_format=torch.channels_last)
        dw = torch.empty(co, ci, 3, 3, device=dev)
        need = lib.unet_conv3x3_wgrad_workspace(n, h, w, ci, co)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        run = lambda: L.check(lib.unet_conv3x3_wgrad(L.UNET_BF16, n, h, w, xv, p(gy), co, p(dw), ci, p(ws), need, st), "wgrad")
        kind = "wgrad16" if co % 128 == 0 else "wgrad_dma"      # the dispatcher's choice: wgrad16_kernel for 128-row forms
        what, timed = f"wgrad n={n} {ci}->{co} {h}x{w} ({kind}_kernel)", "incl. reduce (stamped)"
    else:
        wt = torch.randn(co, ci, 3, 3, device=dev) * 0.05
        y = ops._nhwc_empty(n, co, h, w, dt, dev)
        wp = ops.pack_weight(wt, L.PACK_CONV_FWD, co, ci, dt)
        if args.kernel == "ws16" and args.stats:
            part = torch.empty(lib.unet_conv3x3_stats_max_parts(n, h, w) * 2 * co, device=dev)
            nparts = C.c_int32(0)
            run = lambda: L.check(lib.unet_conv3x3_stats(L.UNET_BF16, n, h, w, xv, p(wp), co, p(y), p(part),
                                                         C.byref(nparts), st), "fwd+stats")
        else:
            yv = ops._views([(y, 0, 0), None])
            run = lambda: L.check(lib.unet_conv3x3(L.UNET_BF16, n, h, w, xv, p(wp), co, yv, co, 0, 0, st), "fwd")
        if args.kernel == "ws16":
            kind, what = "ws16", f"conv {'fwd+stats' if args.stats else 'fwd'} n={n} {ci}->{co} {h}x{w} ws16"
        else:
            pp = co % 128 == 0 and ci >= 512          # the dispatcher's choice: ping-pong for 128-channel tiles from 512 inputs
            kind, what = "pdma_pp" if pp else "pdma", f"conv fwd n={n} {ci}->{co} {h}x{w} {'ping-pong' if pp else 'lock-step'}"
        timed = "(stamped)"
    waves = 4 if kind == "wgrad_dma" else 8

    dbg = torch.zeros(args.records * waves * 8, dtype=torch.int64, device=dev)
    setter(dbg.data_ptr(), args.records * waves)
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        run()
    e1.record()
    torch.cuda.synchronize()
    setter(None, 0)
    us = e0.elapsed_time(e1) * 100
    records = dbg.view(args.records, waves, 8).cpu().numpy()

    rows = decode(kind, records)
    used = records[records[:, :, 6].max(axis=1) > 0]
    if not len(used):
        raise SystemExit(f"stamps.py: {what}: no stamp record was written (the launch did not reach a stamped kernel)")
    unit = KINDS[kind][0]
    print(f"{what}: {us:.1f} us/launch {timed}, blocks {len(used)}, {unit}s/wave {used[:, :, 6].mean():.1f}, "
          f"in-kernel clock {float(np.median(used[:, :, 7])) / 2 ** 20 * 0.1:.2f} GHz")
    print("\n".join(report(kind, rows)))


if __name__ == "__main__":
    main()
