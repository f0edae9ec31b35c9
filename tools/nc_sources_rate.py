#!/usr/bin/env python3
"""What the netCDF file costs behind the runs that could reach it only through host arrays: one process, one box.

    python tools/nc_sources_rate.py [--rows 1024 --cols 1024 --days 40 --depth-days 10 --reps 3 --dir DIR --out profiles/nc_sources_rate.txt]

A synthetic site with data.frame weather from 1 January on, `Tz` the file's only variable.  After a short warm-up, `reps`
times each, alternated, both routes writing into --dir (default: the system's temporary directory):
  (a) arrays   the array call (snow.runmicrosnow1 / api.runmicro_depths), then ncsink.writetonc of its arrays — the only route
               there was: 8 B per value over PCIe into a [rows, cols, steps] host array, packed again on one host core
  (b) one call snow.runmicrosnow_nc / api.runmicro_depths_nc: every chunk packed on the device, 4 B per value over PCIe, no
               host array
for the snow run over --days days and for five depths below ground over --depth-days days (five [rows, cols, steps] arrays
on the host for route (a): the default keeps them at 9.4 GiB).  Host clock around each route, inputs marshalled inside it;
medians with min .. max, and the host array bytes each route allocates.  Then k_pack_nc_planes alone: one 5-day chunk of one
series through mcf_nc_write_planes, the kernel's device time from its events (`kernel_ms`), beside a device-to-device
hipMemcpy of as many bytes as the kernel reads.  There is no pass threshold: the file is where the measured values go.
Needs an MI355X.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np                                   # noqa: E402

from microclimf_amd import _abi, api, ncsink, synthetic  # noqa: E402
from microclimf_amd import snow as S                 # noqa: E402

MAT = 7.5
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
DEPTHS = (-0.05, -0.1, -0.2, -0.5, -1.0)


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        return "unknown device"


def head(d, n):
    return {k: (np.asarray(v)[:n] if np.ndim(v) == 1 else v) for k, v in d.items()}


def stat(v):
    return f"{statistics.median(v):8.3f} s ({min(v):.3f} .. {max(v):.3f})"


def alternate(reps, route_a, route_b, files):
    ta, tb = [], []
    for rep in range(reps):
        for t, route, name in ((ta, route_a, "(a)"), (tb, route_b, "(b)")):
            t0 = time.perf_counter()
            route()
            t.append(time.perf_counter() - t0)
            print(f"rep {rep} {name}: {t[-1]:.3f} s", flush=True)
            for f in files:
                if os.path.exists(f):
                    os.remove(f)
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--days", type=int, default=40)
    ap.add_argument("--depth-days", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "nc_sources_rate.txt"))
    o = ap.parse_args()
    R, Cc, N = o.rows, o.cols, o.rows * o.cols
    T = o.days * 24
    grid = dict(xmin=0.0, xmax=float(Cc), ymin=0.0, ymax=float(R), res=1.0)
    fa, fb = os.path.join(o.dir, "mcf_nc_sources_a.nc"), os.path.join(o.dir, "mcf_nc_sources_b.nc")
    out = [1] + [0] * 9
    sw = synthetic.snow_workload(R, Cc, T, cold=0.0, zref=3.5, start_doy=1)
    g = synthetic.workload(R, Cc, T, reqhgt=0.05, zref=3.5, hgt_range=(0.05, 3.0), start_doy=1, variety=True, out=out)
    _, _, dtm = synthetic.rasters(R, Cc)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    # warm-up: ten days of the same site through both routes
    g10 = dict(g, obstime=head(g["obstime"], 240), climdata=head(g["climdata"], 240), pointm=head(g["pointm"], 240))
    s10 = dict(snow, obstime=head(sw["obstime"], 240), climdata=head(sw["climdata"], 240), pointm=head(sw["pointm"], 240))
    m10 = dict(micro, obstime=head(sw["obstime"], 240), climdata=head(sw["climdata"], 240))
    S.runmicrosnow1(g10, s10, m10, MAT)
    S.runmicrosnow_nc(g10, s10, m10, MAT, fileout=fb, nc_grid=grid, vars=("Tz",))
    os.remove(fb)
    print(f"inputs made ({o.days} days), library warm", flush=True)

    def snow_a():
        arrays = S.runmicrosnow1(g, snow, micro, MAT)
        ncsink.writetonc(dict(arrays, tme=sw["obstime"]), fa, grid, 0.05, ("Tz",))

    def snow_b():
        S.runmicrosnow_nc(g, snow, micro, MAT, fileout=fb, nc_grid=grid, vars=("Tz",))

    sa, sb = alternate(o.reps, snow_a, snow_b, (fa, fb))
    lines = [f"netCDF file behind the snow run and the depth run on {device_name()}: {R} x {Cc} cells, data.frame "
             f"weather from 1 January, Tz the file's only variable, classic container, both routes writing into one directory; 1 warm-up + {o.reps} alternated "
             f"runs per route, host clock, median (min .. max)",
             f"command: python tools/nc_sources_rate.py --rows {R} --cols {Cc} --days {o.days} --depth-days {o.depth_days} --reps {o.reps}",
             f"-- snow run, {o.days} days ({T} h), 5-day chunks, one block; the file is {N * T * 4 / 2**30:.2f} GiB",
             f"   (a) runmicrosnow1 + writetonc : {stat(sa)}  host arrays {N * T * 8 / 2**30:.2f} GiB",
             f"   (b) runmicrosnow_nc           : {stat(sb)}  host arrays 0 GiB",
             f"   (b) / (a) = {statistics.median(sb) / statistics.median(sa):.3f}"]
    del sw, g, snow, micro
    # ---- five depths from one solve
    Td = o.depth_days * 24
    a = synthetic.workload(R, Cc, Td, reqhgt=DEPTHS[0], variety=True, start_doy=150, complete=True, out=[1, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    b = {k: a[k] for k in ARGS}
    files_a = [os.path.join(o.dir, f"mcf_nc_sources_a{d}.nc") for d in range(5)]
    files_b = [os.path.join(o.dir, f"mcf_nc_sources_b{d}.nc") for d in range(5)]

    def depths_a():
        full = api.runmicro_depths(**b, depths=DEPTHS, soilm=False)
        for d in range(5):
            ncsink.writetonc(dict(Tz=full["Tz"][d], tme=a["obstime"]), files_a[d], grid, DEPTHS[d], ("Tz",))

    def depths_b():
        api.runmicro_depths_nc(**b, depths=DEPTHS, files=files_b, grid=grid, soilm=False)

    da, db = alternate(o.reps, depths_a, depths_b, files_a + files_b)
    lines += [f"-- five depths {DEPTHS} from one streamed solve, complete = 1, {o.depth_days} days ({Td} h); five files of {N * Td * 4 / 2**30:.2f} GiB",
              f"   (a) runmicro_depths + 5 x writetonc : {stat(da)}  host arrays {5 * N * Td * 8 / 2**30:.2f} GiB",
              f"   (b) runmicro_depths_nc              : {stat(db)}  host arrays 0 GiB",
              f"   (b) / (a) = {statistics.median(db) / statistics.median(da):.3f}"]
    del a, b
    # ---- k_pack_nc_planes alone, beside a copy of as many bytes
    hip = C.CDLL(_abi._needed_hip_soname(_abi.LIB_PATH) or "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    steps = 120
    rng = np.random.default_rng(1)
    x = np.asfortranarray(np.round(rng.normal(size=(R, Cc, steps)) * 30, 3))
    x[rng.random((R, Cc)) < 0.02] = np.nan
    read_bytes = steps * N * 8
    pa, pb = C.c_void_p(), C.c_void_p()
    if hip.hipMalloc(C.byref(pa), read_bytes) != 0 or hip.hipMalloc(C.byref(pb), read_bytes) != 0:
        raise SystemExit("hipMalloc of the copy buffers failed")
    kms, cms = [], []
    hours, east, north = 400000.0 + np.arange(steps), np.arange(Cc) + 0.5, np.arange(R) + 0.5
    for rep in range(o.reps + 3):
        with ncsink.SnowpackNcWriter(fb, R, Cc, hours, east, north, vars=("totalSWE",)) as w:
            ms = w.write_planes(0, 0, {"totalSWE": x}, timing=True)
        os.remove(fb)
        hip.hipDeviceSynchronize()
        t1 = time.perf_counter()
        rc = hip.hipMemcpy(pb, pa, read_bytes, 3)
        hip.hipDeviceSynchronize()
        t2 = time.perf_counter()
        if rc != 0:
            raise SystemExit(f"the yardstick copy failed ({rc})")
        if rep:
            kms.append(ms)
            cms.append((t2 - t1) * 1e3)
    hip.hipFree(pa)
    hip.hipFree(pb)
    mk, mc = statistics.median(kms), statistics.median(cms)
    rate = lambda ms: read_bytes / (ms * 1e-3) / 1e12      # noqa: E731
    lines += [f"-- k_pack_nc_planes, one series x {steps} steps: {read_bytes / 2**30:.2f} GiB read, half as much written",
              f"   kernel (its events, summed over the pieces of a call) : {mk:9.3f} ms  reads {rate(mk):.2f} TB/s  runs {[round(v, 3) for v in kms]}",
              f"   d2d copy (host clock around a synchronised call)      : {mc:9.3f} ms  reads {rate(mc):.2f} TB/s (and writes as much)  runs {[round(v, 3) for v in cms]}",
              f"   ratio kernel / copy (read rate): {mc / mk:.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text(text)


if __name__ == "__main__":
    main()
