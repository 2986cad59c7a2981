"""tools/stamps.py without a GPU: decode() on hand-written stamp records of every kernel family, the torch-free import,
and the one-line error against a library without the setter.

A record is eight uint64 per wave: laps [0..5], count [6], clock [7] (csrc/stamps.h).  Every case is 3 blocks x the
family's wave count: block 1 is left all-zero (a block that never ran or lay beyond the buffer), and the second wave
class (where the family has two) carries laps twice as large as the first."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import stamps  # noqa: E402

COUNT = 90
LAPS = np.array([100.0, 250.0, 400.0, 1300.0, 70.0, 33.0]) * COUNT     # per wave, summed over COUNT taps or tiles
CLOCK = 2 ** 20 * 24                                                    # 24 x 100 MHz


def records(waves):
    r = np.zeros((3, waves, 8), dtype=np.uint64)
    for b in (0, 2):
        for wv in range(waves):
            r[b, wv, :6] = (LAPS * (2 if wv >= 4 else 1)).astype(np.uint64)
            r[b, wv, 6] = COUNT
            r[b, wv, 7] = CLOCK
    return r


PER = LAPS / COUNT
CASES = {
    # kind: (waves, wave classes, lap names in order with their lap index, extras: name -> (lap, per count))
    "pdma": (8, ["waves 0-3", "waves 4-7"],
             [("vmcnt wait", 0), ("barrier", 1), ("dma issue", 2), ("reads+mfma", 3)], {"epilogue/launch": (4, False)}),
    "pdma_pp": (8, ["waves 0-3", "waves 4-7"],
                [("reads+dma issue", 0), ("vmcnt+lgkm wait", 1), ("barrier(L)", 2), ("mfma", 3), ("barrier(C)", 5)],
                {"of which fragment-read issue/tap": (4, True)}),
    "ws16": (8, ["waves 0-3", "waves 4-7"],
             [("vmcnt wait", 0), ("barrier", 1), ("top: dma / deferred stores / geometry", 2), ("mfma loop", 3),
              ("late dma", 4), ("epilogue + stores", 5)], {}),
    "wgrad_dma": (4, ["all waves"],
                  [("vmcnt(0) wait", 0), ("barrier", 1), ("dma issue", 2), ("fragment reads + mfma", 3)], {}),
    "wgrad16": (8, ["dY waves (DMA mid-tile)", "X waves (DMA at tile start)"],
                [("vmcnt(0) wait", 0), ("barrier", 1), ("dma issue", 2), ("fragment reads + mfma", 3)],
                {"partial-slab stores (drained)": (4, False), "kernel body": (5, False)}),
}


@pytest.mark.parametrize("kind", sorted(CASES))
def test_decode(kind):
    waves, classes, laps, extras = CASES[kind]
    rows = stamps.decode(kind, records(waves))
    assert [r["waves"] for r in rows] == classes
    for k, row in enumerate(rows):
        scale = 2.0 if k == 1 else 1.0                        # the second wave class: laps twice as large
        assert list(row["laps"]) == [nm for nm, _ in laps]    # the names, in order
        for nm, i in laps:
            assert row["laps"][nm] == pytest.approx(scale * PER[i], rel=1e-9)
        assert list(row["extras"]) == list(extras)
        for nm, (i, per) in extras.items():
            assert row["extras"][nm] == pytest.approx(scale * (PER[i] if per else LAPS[i]), rel=1e-9)
        # the all-zero block is ignored: two blocks' waves, and means that a zero record would have halved or broken
        assert row["records"] == 2 * (waves if len(classes) == 1 else waves // 2)
        assert row["count"] == pytest.approx(COUNT, rel=1e-9)
        assert f"{row['clock_ghz']:.2f}" == "2.40"
        assert row["clock_ghz"] == pytest.approx(2.4, rel=1e-9)
    assert len(stamps.report(kind, rows)) == len(rows)


def test_decode_leaves_out_every_empty_record():
    assert stamps.decode("ws16", np.zeros((3, 8, 8), dtype=np.uint64)) == []


def test_import_needs_no_torch():
    code = "import sys; import tools.stamps; assert 'torch' not in sys.modules, 'torch imported'"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_without_the_setter_gives_one_line():
    with pytest.raises(SystemExit) as e:
        stamps.bind_setter(ctypes.CDLL(None))                 # the process itself: no unet_debug_set_buffer
    msg = str(e.value)
    assert "\n" not in msg and "make stamps" in msg and "unet_debug_set_buffer" in msg
