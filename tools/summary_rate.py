#!/usr/bin/env python3
"""What the period-summary sink costs and how fast it reads the ring: one process, one box.

    python tools/summary_rate.py [--rows 1024 --cols 1024 --hours 240 --chunk 5 --reps 5 --out profiles/summary_rate.txt]

Vector forcing, all ten outputs solved; the summary keeps all six statistics of `Tz` alone or of all ten outputs, over monthly
periods or one all-run period (four configurations, one plan each).  Per configuration, after one warm-up pass, `reps` passes of
  plain   the run_days loop over the series in chunks of `chunk` days (kernels this sink does not touch)
  sink    the same loop with summary_accumulate behind every chunk
  acc     summary_accumulate alone on a filled slot (summary_reset before each, outside the timer)
  copy    a device-to-device copy of exactly the bytes the accumulate reads from that slot: the selected variables' blocks
          (all ten: the slot as one run; Tz alone: its 4 KiB block out of every tile-day, a strided 2-D copy)
timed with HIP events on the plan's stream (copy: host clock around a synchronised hipMemcpy, milliseconds long).  Medians.
Reported: ring bytes read per second by acc and by copy (a copy also WRITES as many bytes), acc / copy, and sink / plain.
There is no pass threshold: the file is where the measured values go.  Needs an MI355X.
"""
import argparse
import ctypes as C
import platform
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np                                   # noqa: E402

from microclimf_amd import _abi, frontend, synthetic  # noqa: E402
from microclimf_amd.api import Plan                  # noqa: E402


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown device"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--hours", type=int, default=240)
    ap.add_argument("--chunk", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "summary_rate.txt"))
    o = ap.parse_args()
    nd = o.hours // 24
    if nd % o.chunk:
        raise SystemExit("--chunk must divide the days: the copy yardstick takes a full slot")
    name = device_name()
    a = synthetic.workload(o.rows, o.cols, o.hours, reqhgt=0.05, variety=True, start_doy=176)      # 25 June on: two months
    hip = C.CDLL(_abi._needed_hip_soname(_abi.LIB_PATH) or "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    D2D = 3
    lines = [f"period-summary sink on {name} (host {platform.node()}): {o.rows} x {o.cols} cells x {nd * 24} h, vector forcing, all ten "
             f"outputs solved, chunks of {o.chunk} days, 1 warm-up + {o.reps} timed passes, medians"]
    for sel_name, sel in (("Tz alone", ("Tz",)), ("all ten", _abi.OUT_NAMES)):
        for by in ("month", "all"):
            tab, labels = frontend.summary_periods(a["obstime"], by)
            with Plan(**a, ring_days=o.chunk) as p:
                p.summary_enable(tab, sel, _abi.STAT_NAMES, 15.0, nperiods=len(labels))
                lay = p.ring_layout()
                ntiles = (lay["cells"] + lay["cells_per_tile"] - 1) // lay["cells_per_tile"]
                blk = lay["block_doubles"] * 8
                read_bytes = len(sel) * ntiles * blk * o.chunk                        # what one accumulate of a full slot reads
                q = C.c_void_p()
                _abi.check(p._lib.mcf_plan_slot_ptr(p._p, 0, 0, C.byref(q)))           # Tz is the slot's first slab
                dst = C.c_void_p()
                if hip.hipMalloc(C.byref(dst), read_bytes) != 0:
                    raise SystemExit("hipMalloc of the copy target failed")
                t = {"plain": [], "sink": [], "acc": [], "copy": []}
                for rep in range(o.reps + 1):
                    p.timer_start()
                    for d0 in range(0, nd, o.chunk):
                        p.run_days(d0, o.chunk, 0)
                    plain = p.timer_stop()
                    p.summary_reset()
                    p.timer_start()
                    for d0 in range(0, nd, o.chunk):
                        p.run_days(d0, o.chunk, 0)
                        p.summary_accumulate(0, 0, d0, o.chunk)
                    sink = p.timer_stop()
                    p.summary_reset()
                    p.sync()
                    p.timer_start()
                    p.summary_accumulate(0, 0, nd - o.chunk, o.chunk)                  # the slot holds the last chunk
                    acc = p.timer_stop()
                    p.sync()
                    t0 = time.perf_counter()
                    if len(sel) == 10:
                        rc = hip.hipMemcpy(dst, q, read_bytes, D2D)
                    else:
                        rc = hip.hipMemcpy2D(dst, blk, q, lay["day_stride"] * 8, blk, ntiles * o.chunk, D2D)
                    hip.hipDeviceSynchronize()
                    cp = (time.perf_counter() - t0) * 1e3
                    if rc != 0:
                        raise SystemExit(f"the yardstick copy failed ({rc})")
                    if rep:
                        for k, v in (("plain", plain), ("sink", sink), ("acc", acc), ("copy", cp)):
                            t[k].append(v)
                hip.hipFree(dst)
                state = p.device_bytes
                valid = p.valid_cells
            m = {k: statistics.median(v) for k, v in t.items()}
            rate = lambda ms: read_bytes / (ms * 1e-3) / 1e12                          # noqa: E731
            lines += [
                f"-- {sel_name}, periods by {by} ({len(labels)}): six statistics, {read_bytes / 2**30:.2f} GiB read per {o.chunk}-day slot, plan holds {state / 2**30:.2f} GiB",
                f"   plain loop : {m['plain']:9.3f} ms  ({valid * nd * 24 / (m['plain'] * 1e-3):.3e} cell-steps/s)  runs {[round(x, 2) for x in t['plain']]}",
                f"   with sink  : {m['sink']:9.3f} ms  ratio sink / plain {m['sink'] / m['plain']:.3f}  runs {[round(x, 2) for x in t['sink']]}",
                f"   accumulate : {m['acc']:9.3f} ms per slot  reads {rate(m['acc']):.2f} TB/s  runs {[round(x, 3) for x in t['acc']]}",
                f"   d2d copy   : {m['copy']:9.3f} ms per slot  reads {rate(m['copy']):.2f} TB/s (and writes as much)  runs {[round(x, 3) for x in t['copy']]}",
                f"   ratio accumulate / copy (read rate): {m['copy'] / m['acc']:.3f}",
                f"   a 4096^2 year at this rate: {m['acc'] * 1e-3 * (4096 * 4096 / (o.rows * o.cols)) * (365 / o.chunk) / len(sel):.3f} s per variable",
            ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text(text)


if __name__ == "__main__":
    main()
