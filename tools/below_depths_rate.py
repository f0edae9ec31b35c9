"""Below ground at several depths from one solve: what D depths cost beside one.  One process, 512 x 512
cells x 8760 h, vector forcing, complete = 0 and 1:

  1. api.runmicro_depths_summary (Tz by month: mean, min, max) at D = 1, 3 and 5, the three alternating after a warm-up of
     each: medians of five with min .. max, t(5) / t(1) and t(5) / (5 t(1));
  2. k_below_chunk alone, one launch between two events on the stream it runs on, on state of a year's shape (a 16-day chunk
     in the middle of the series, damping depths of 5 .. 30 cm): this library at D = 1 and D = 5 and the PARENT commit's
     library at D = 1, the three alternating.  The launcher is called directly with a hand-built argument block — the
     parent's block is the first part of this library's, so both read the same one.  With complete = 1 a launch is
     k_below_chunk and k_below_carry, in both libraries;
  3. the device bytes per cell of a streamed plan with its depth slabs and summary state (16 ring days) at D = 1 and 5.

The parent's library is built to a second path from `git archive` when it is not there yet.
Usage: python tools/below_depths_rate.py [--n 512] [--parent-rev HEAD~1] [--parent-lib build/parent/libmcfhip.so]
                                         [--out profiles/below_depths_rate.txt]"""
import argparse
import ctypes as C
import shutil
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from microclimf_amd import _abi, api, frontend, synthetic          # noqa: E402

OUT = [1, 0, 0, 1, 0, 0, 0, 0, 0, 0]
DEPTHS = {1: (-0.05,), 3: (-0.05, -0.2, -1.0), 5: (-0.05, -0.1, -0.2, -0.5, -1.0)}
T, ND, WIN = 8760, 365, 47
LAUNCH = "_ZN3mcf18launch_below_chunkERKNS_15BelowStreamArgsEP12ihipStream_t"
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return f"{statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})"


def parent_library(path: Path, rev: str) -> Path:
    if path.exists():
        return path
    src = path.parent / "src"
    src.mkdir(parents=True, exist_ok=True)
    tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, "microclimf_amd/csrc", "include"], check=True,
                         capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", str(src)], input=tar, check=True)
    subprocess.run(["make", "-C", str(src / "microclimf_amd" / "csrc"), "-j16"], check=True, capture_output=True)
    shutil.copy(src / "microclimf_amd" / "csrc" / "libmcfhip.so", path)
    return path


def tbp_rows(a, depths):
    base = np.asarray(a["pointm"]["Tbp"], dtype=np.float64)
    k = np.arange(base.size)
    return np.stack([base + 0.2 * d + np.cos(2 * np.pi * k / 24 + d) for d in depths])


# ---- 1. the one call -----------------------------------------------------------------------------------------------------------
def one_call(n, complete):
    a = synthetic.workload(n, n, T, reqhgt=-0.05, start_doy=1, out=OUT, complete=bool(complete))
    b = {k: v for k, v in a.items() if k not in ("reqhgt", "out")}
    tab, labels = frontend.summary_periods(a["obstime"], "month")

    def run(D):
        t0 = time.perf_counter()
        api.runmicro_depths_summary(**b, depths=DEPTHS[D], tbp=None if complete else tbp_rows(a, DEPTHS[D]), periods=tab,
                                    nperiods=len(labels), vars=("Tz",), stats=("mean", "min", "max"))
        return time.perf_counter() - t0
    for D in (1, 3, 5):
        run(D)
    t = {1: [], 3: [], 5: []}
    for _ in range(5):
        for D in (1, 3, 5):
            t[D].append(run(D))
    say(f"runmicro_depths_summary, {n} x {n} x {T}, complete = {complete}, Tz by month (mean, min, max), seconds, median of 5 (min .. max)")
    for D in (1, 3, 5):
        say(f"  D = {D}: {spread(t[D])}")
    m1, m5 = statistics.median(t[1]), statistics.median(t[5])
    say(f"  t(5) / t(1) = {m5 / m1:.3f}   t(5) / (5 t(1)) = {m5 / (5 * m1):.3f}   per extra depth {(m5 - m1) / 4 * 1e3:.1f} ms "
        f"(the spread of t(1): {(max(t[1]) - min(t[1])) * 1e3:.1f} ms)")


# ---- 2. the kernel alone ---------------------------------------------------------------------------------------------------------
class RingView(C.Structure):
    _fields_ = [("base", C.c_void_p), ("N", C.c_int64), ("tile_stride", C.c_int64), ("day_stride", C.c_int64), ("cpb", C.c_int32)]


class BelowStreamArgs(C.Structure):      # microclimf_amd/csrc/mcf_kernels.h; the parent's block ends behind cal0
    _fields_ = [("N", C.c_int64), ("tsteps", C.c_int32), ("ndays", C.c_int32), ("complete", C.c_int32), ("hiy", C.c_int32),
                ("reqhgt", C.c_double), ("mat", C.c_double), ("hgt", C.c_void_p), ("tg", RingView), ("tz", RingView),
                ("day0", C.c_int32), ("ndays_chunk", C.c_int32), ("tail", C.c_int32), ("ddsum", C.c_void_p), ("hsum", C.c_void_p),
                ("dmean", C.c_void_p), ("ybuf", C.c_void_p), ("wrap", C.c_void_p), ("prev", C.c_void_p), ("Tgp", C.c_void_p),
                ("Tbp", C.c_void_p), ("per_cell_pointm", C.c_int32), ("days", C.c_void_p), ("cal0", C.c_int32),
                ("ndepths", C.c_int32), ("depth", C.c_double * 8), ("tzx", RingView), ("tzx_stride", C.c_int64),
                ("ybufx", C.c_void_p), ("tbp_stride", C.c_int64)]


def kernel_alone(n, complete, parent_path):
    import torch
    dev = torch.device("cuda:0")
    N, cpb, blk, chunk = n * n, 21, 512, 16
    ntiles = (N + cpb - 1) // cpb
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, device=dev, generator=g) * 5 + 10
    slab = ntiles * chunk * blk
    tg, tz, tzx = rnd(slab), torch.empty(slab, dtype=torch.float64, device=dev), torch.empty(4 * slab, dtype=torch.float64, device=dev)
    hgt = torch.full((N,), 0.5, dtype=torch.float64, device=dev)
    hgt[::97] = float("nan")
    meanD = 0.05 + 0.25 * torch.rand(N, dtype=torch.float64, device=dev, generator=g)
    ddsum, hsum = meanD * T, rnd(N) * T
    dmean, ybuf, ybufx = rnd(ND * N), rnd(ND * N), rnd(4 * ND * N)
    wrap, prev = rnd(WIN * N), rnd(WIN * N)
    tgp, tbp = rnd(T), rnd(5 * T)
    md = meanD.cpu().numpy()
    for depth in DEPTHS[5]:
        nn = np.round(-118.35 * depth / md)
        say(f"    depth {depth:5.2f}: n <= 48 {np.mean(nn <= 48):5.1%}, 48 < n < tsteps {np.mean((nn > 48) & (nn < T)):5.1%}, "
            f"n >= tsteps {np.mean(nn >= T):5.1%}" + ("" if complete else f"; nb <= 24 {np.mean(nn <= 24):5.1%}"))

    def view(t):
        return RingView(t.data_ptr(), N, chunk * blk, blk, cpb)

    def block(depths):
        a = BelowStreamArgs()
        a.N, a.tsteps, a.ndays, a.complete, a.hiy = N, T, ND, complete, 8760
        a.reqhgt, a.mat, a.hgt = depths[0], 10.0, hgt.data_ptr()
        a.tg, a.tz, a.tzx = view(tg), view(tz), view(tzx)
        a.day0, a.ndays_chunk, a.tail = 160, chunk, 0
        a.ddsum, a.hsum, a.dmean, a.ybuf, a.wrap, a.prev = (t.data_ptr() for t in (ddsum, hsum, dmean, ybuf, wrap, prev))
        a.Tgp, a.Tbp, a.per_cell_pointm, a.days, a.cal0 = tgp.data_ptr(), tbp.data_ptr(), 0, None, 160
        a.ndepths = len(depths)
        for d, v in enumerate(depths):
            a.depth[d] = v
        a.tzx_stride, a.ybufx, a.tbp_stride = slab, ybufx.data_ptr(), T
        return a

    here, parent = _abi.load(), C.CDLL(str(parent_path))
    cases = [("this library, D = 1", here, block(DEPTHS[1])), ("this library, D = 5", here, block(DEPTHS[5])),
             ("parent's library, D = 1", parent, block(DEPTHS[1]))]
    fns = []
    for _, lib, _a in cases:
        fn = getattr(lib, LAUNCH)
        fn.restype, fn.argtypes = None, [C.POINTER(BelowStreamArgs), C.c_void_p]
        fns.append(fn)

    def launch(i):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fns[i](C.byref(cases[i][2]), None)          # the null stream: the stream the events are recorded on
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    for i in range(3):
        launch(i), launch(i)
    ms = [[], [], []]
    for _ in range(15):
        for i in range(3):
            ms[i].append(launch(i))
    # the D = 1 slab of the two libraries from the same state: the same bits
    fns[0](C.byref(cases[0][2]), None)
    torch.cuda.synchronize()
    mine = tz.clone()
    fns[2](C.byref(cases[2][2]), None)
    torch.cuda.synchronize()
    same = bool((mine.view(torch.int64) == tz.view(torch.int64)).all())
    say(f"  k_below_chunk{' + k_below_carry' if complete else ''}, one launch of {chunk} days x {N} cells, ms, median of 15 (min .. max); "
        f"D = 1 slab equal to the parent's bit for bit: {same}")
    for (name, _, _a), v in zip(cases, ms):
        say(f"    {name:24s} {spread(v)}   {statistics.median(v) * 1e6 / (N * chunk):.3f} ns per cell-day")
    m = [statistics.median(v) for v in ms]
    say(f"    D = 5 / D = 1 = {m[1] / m[0]:.2f}   this D = 1 / parent's D = 1 = {m[0] / m[2]:.2f}")


# ---- 3. device bytes ---------------------------------------------------------------------------------------------------------------
def device_bytes(n, complete):
    a = synthetic.workload(n, n, T, reqhgt=-0.05, start_doy=1, out=OUT, complete=bool(complete))
    tab, _labels = frontend.summary_periods(a["obstime"], "month")
    for D in (1, 5):
        with api.Plan(**a, ring_days=16, stream_below=True) as p:
            b0 = p.device_bytes
            p.below_set_depths(DEPTHS[D], None if complete else tbp_rows(a, DEPTHS[D]))
            b1 = p.device_bytes
            p.summary_enable_below(tab, ("Tz",), ("mean", "min", "max"))
            b2 = p.device_bytes
        say(f"  complete = {complete}, D = {D}: {b2 / (n * n):9.0f} B per cell for the year (plan {b0 / (n * n):.0f}, depth slabs and rows "
            f"{(b1 - b0) / (n * n):.0f}, summary state {(b2 - b1) / (n * n):.0f}); a [steps] series of one variable: {T * 8} B per cell")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--parent-rev", default="HEAD~1")
    ap.add_argument("--parent-lib", default=str(ROOT / "build" / "parent" / "libmcfhip.so"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "below_depths_rate.txt"))
    o = ap.parse_args()
    parent = parent_library(Path(o.parent_lib), o.parent_rev)
    say(f"tools/below_depths_rate.py: depths D = 1 {DEPTHS[1]}, D = 3 {DEPTHS[3]}, D = 5 {DEPTHS[5]}")
    for complete in (0, 1):
        one_call(o.n, complete)
    for complete in (0, 1):
        say(f"k_below_chunk alone, complete = {complete}; regimes of the cells at each depth:")
        kernel_alone(o.n, complete, parent)
    say("device bytes of a streamed plan, 16 ring days, Tz + soilm requested, Tz summarised by month (3 statistics):")
    for complete in (0, 1):
        device_bytes(o.n, complete)
    Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    Path(o.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
