#!/usr/bin/env python3
"""What the streamed bioclim sink saves with coarse array forcing: one process, one box.

    python tools/bioclim_array_rate.py [--small 1024 --large 4096 --crows 8 --ccols 8 --out profiles/bioclim_array_rate.txt]

runbioclim2Cpp_coarse on a synthetic `small`^2 raster under a crows x ccols climate grid, 624 steps (fourteen days and four
three-day quarters): the whole-series sink (MCF_BIOCLIM_WHOLE=1: 2 x 8 B x cells x steps of solver output, then k_bioclim)
against the streamed sink (day chunks into the ring, k_bioclim_acc, k_bioclim_fin<true>), where both fit; then the streamed
sink alone at `large`^2, where the whole-series output would not.  The default ring budget (MCF_BIOCLIM_RING_GB) holds the
small raster's whole series in one chunk: set it smaller to see the small raster in the chunks the large one gets.  Each
configuration: one warm-up call, then one call timed between two HIP events on the null stream — the call is synchronous and
includes the plan's set-up and the upload of the rasters, which both routes share.  Peak device memory: the smallest free
figure hipMemGetInfo gives while the timed call runs (polled from a second thread every few milliseconds), against the figure
before it.  The two routes must agree bit for bit.  There is no pass threshold: the file is where the measured values go.
Needs an MI355X.
"""
import argparse
import ctypes as C
import os
import platform
import sys
import threading
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np                                   # noqa: E402

from microclimf_amd import _abi, api, synthetic      # noqa: E402

T = 336 + 4 * 72


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown device"


class Hip:
    def __init__(self):
        h = self.h = C.CDLL(_abi._needed_hip_soname(_abi.LIB_PATH) or "libamdhip64.so")
        h.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        h.hipEventSynchronize.argtypes = [C.c_void_p]
        h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            if h.hipEventCreate(C.byref(e)) != 0:
                raise SystemExit("hipEventCreate failed")

    def free_bytes(self):
        f, t = C.c_size_t(), C.c_size_t()
        if self.h.hipMemGetInfo(C.byref(f), C.byref(t)) != 0:
            raise SystemExit("hipMemGetInfo failed")
        return f.value

    def timed(self, fn):
        """(result, milliseconds between the two events, peak bytes in use above the level before the call)"""
        before = self.free_bytes()
        low = [before]
        stop = threading.Event()

        def poll():
            while not stop.is_set():
                low[0] = min(low[0], self.free_bytes())
                time.sleep(0.004)
        th = threading.Thread(target=poll)
        th.start()
        try:
            self.h.hipEventRecord(self.e0, None)
            res = fn()
            self.h.hipEventRecord(self.e1, None)
            self.h.hipEventSynchronize(self.e1)
        finally:
            stop.set()
            th.join()
        ms = C.c_float()
        self.h.hipEventElapsedTime(C.byref(ms), self.e0, self.e1)
        return res, float(ms.value), before - low[0]


def workload(n, crows, ccols):
    a, rp, cp = synthetic.coarse_workload(n, n, T, crows, ccols, reqhgt=0.05, variety=True, na_frac=0.02, start_doy=150)
    for k in ("complete", "out"):
        a.pop(k)
    a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
    q = [np.arange(336 + 72 * i, 336 + 72 * (i + 1)) for i in range(4)]
    return dict(a, out=[1] * 19, wetq=q[0], dryq=q[1], hotq=q[2], colq=q[3], air=True, rowpos=rp, colpos=cp)


def measure(hip, kw, whole):
    if whole:
        os.environ["MCF_BIOCLIM_WHOLE"] = "1"
    else:
        os.environ.pop("MCF_BIOCLIM_WHOLE", None)
    api.runbioclim2Cpp_coarse(**kw)                                        # warm-up
    res, ms, peak = hip.timed(lambda: api.runbioclim2Cpp_coarse(**kw))
    chunks = api.bioclim_last_chunks()
    os.environ.pop("MCF_BIOCLIM_WHOLE", None)
    return res, ms, peak, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=1024)
    ap.add_argument("--large", type=int, default=4096, help="0: skip the large raster")
    ap.add_argument("--crows", type=int, default=8)
    ap.add_argument("--ccols", type=int, default=8)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "bioclim_array_rate.txt"))
    o = ap.parse_args()
    hip = Hip()
    lines = [f"array-weather runbioclim on coarse arrays on {device_name()} (host {platform.node()}): {T} steps, "
             f"{o.crows} x {o.ccols} climate grid, all nineteen variables, 1 warm-up + 1 timed call each, "
             f"MCF_BIOCLIM_RING_GB={os.environ.get('MCF_BIOCLIM_RING_GB', 'default (14)')}"]
    kw = workload(o.small, o.crows, o.ccols)
    cells = o.small * o.small
    w_res, w_ms, w_peak, w_chunks = measure(hip, kw, True)
    s_res, s_ms, s_peak, s_chunks = measure(hip, kw, False)
    same = all(np.array_equal(w_res[k], s_res[k], equal_nan=True) for k in w_res)
    lines += [
        f"-- {o.small} x {o.small} ({cells * T:.3e} cell-steps; whole-series output {2 * 8 * cells * T / 1e9:.1f} GB)",
        f"   whole-series : {w_ms:10.1f} ms  peak device memory {w_peak / 1e9:7.2f} GB  chunks {w_chunks}",
        f"   streamed     : {s_ms:10.1f} ms  peak device memory {s_peak / 1e9:7.2f} GB  chunks {s_chunks}",
        f"   ratio streamed / whole-series: time {s_ms / w_ms:.3f}, memory {s_peak / max(w_peak, 1):.3f}; same bits: {same}",
    ]
    del w_res, s_res, kw
    if o.large:
        kw = workload(o.large, o.crows, o.ccols)
        cells = o.large * o.large
        _, ms, peak, chunks = measure(hip, kw, False)
        lines += [
            f"-- {o.large} x {o.large} ({cells * T:.3e} cell-steps; the whole-series output would be {2 * 8 * cells * T / 1e9:.0f} GB)",
            f"   streamed     : {ms:10.1f} ms  peak device memory {peak / 1e9:7.2f} GB  chunks {chunks}  "
            f"({cells * T / (ms * 1e-3):.3e} cell-steps/s, call included)",
        ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text(text)
    if not same:
        raise SystemExit("the streamed and the whole-series matrices differ")


if __name__ == "__main__":
    main()
