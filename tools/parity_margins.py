#!/usr/bin/env python3
"""Margins of the GPU-against-oracle parity bars (tests/parity_bars.py), case by case.

For every workload of tests/parity_cases.py (the hand-written cases and the 96 random draws) and tests/snow_cases.py (snow
model; snow microclimate at MICRO_HEIGHTS), and with --sets snowfast1,snowfast2 of tests/snowfast_cases.py (the oracle chains of
the fast snow method's one-call entries), one line, or with --per-variable one line per variable:

    N        spread of the oracle's noise variants (fma, ulp, ulpfma): how far apart two correct evaluations lie
    bar      min(1e-6, max(2^-40, 16 N)): what the GPU tests assert
    S_*      distance of each slip variant (one libm family through float; exp at 46 bits) from the oracle
             ("pattern": the slip changes the NaN / inf pattern, which the comparator refuses outright)
    d, d/bar with --gpu: distance of the HIP kernels from the oracle on the same inputs

The per-case line gives the variable with the largest bar (N, bar), each slip's S / bar in the variable where that is
largest (what the power condition of tests/test_parity_bars_cpu.py is about; "-": the slip does not touch the case), and
with --gpu the variable with the largest d / bar.

The snowfast sets run on terrain_oracle's terrain without --gpu.  With --gpu the oracle chain is handed the device's terrain
(terrain.snow_terrain; no variant models numpy terrain: DESIGN section 2, "Tolerance"), so N, bar and S are those of that
terrain, and each case gives two lines: `caseN` the one device-resident call, `caseN/days` the host day loop.

    python tools/parity_margins.py > profiles/parity_bars_cpu.txt             (no GPU needed)
    python tools/parity_margins.py --gpu > profiles/parity_margins_gpu.txt
    python tools/parity_margins.py --sets snowfast1,snowfast2 [--gpu] [--per-variable]       (appended to the same files)
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import parity_bars as PB  # noqa: E402
from oracle import oracle as O  # noqa: E402


def hip(inp):
    if inp["kind"] == "grid":
        from microclimf_amd.api import runmicro1Cpp, runmicro2Cpp
        a = dict(inp["a"])
        if inp["af"]:
            a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
            return runmicro2Cpp(**a, **inp["extra"])
        return runmicro1Cpp(**a, **inp["extra"])
    from microclimf_amd import snow as S
    if inp["kind"] in ("snowfast1", "snowfast2"):
        c, days = inp["case"], "_days" if inp.get("days") else ""
        if inp["kind"] == "snowfast1":
            return getattr(S, "snowmodelq1" + days)(*c["args"])
        return getattr(S, "snowmodelq2" + days)(*c["args"], **c["pos"])
    if inp["kind"] == "snowmodel":
        sw = inp["sw"]
        return (S.gridmodelsnow2 if inp["af"] else S.gridmodelsnow1)(sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"],
                                                                      sw["other"], sw["snowenv"])
    return (S.gridmicrosnow2 if inp["af"] else S.gridmicrosnow1)(*inp["args"])


def workloads(sets, gpu):
    """PB.case_sets; with --gpu a snowfast case runs on the device's terrain and yields the one call and the day loop"""
    for kind, label, run, inp in PB.case_sets(O, sets):
        if gpu and kind in ("snowfast1", "snowfast2"):
            import snowfast_cases as FC
            from microclimf_amd.terrain import snow_terrain
            z, res, zref, _ = FC.oracle_terrain(inp["case"])
            run = FC.run(O, inp["case"], terrain=snow_terrain(z, res, zref, device=0))
            yield kind, label, run, inp
            yield kind, label + "/days", run, dict(inp, days=True)
        else:
            yield kind, label, run, inp


def fmt(x):
    return "pattern" if x == float("inf") else f"{x:.2e}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gpu", action="store_true", help="also solve every workload on the device and print d, d / bar")
    ap.add_argument("--per-variable", action="store_true", help="one line per (case, variable) instead of one per case")
    ap.add_argument("--sets", default="cases,random,snowmodel,microsnow")
    args = ap.parse_args()
    slips = O.SLIP_VARIANTS
    print(f"# K = {PB.K:g}, FLOOR = 2^-40 = {PB.FLOOR:.3e}, CAP = {PB.CAP:g}; noise variants {', '.join(O.NOISE_VARIANTS)}")
    if args.per_variable:
        print("# set case variable N bar " + " ".join(f"S_{s}" for s in slips) + (" d d/bar" if args.gpu else ""))
    else:
        print("# set case variables largest-bar-variable N bar " + " ".join(f"S_{s}/bar" for s in slips)
              + (" largest-d/bar-variable d bar d/bar" if args.gpu else ""))
    summary = {}
    slipped = {}
    for kind, label, run, inp in workloads(tuple(args.sets.split(",")), args.gpu):
        want, bars, noise = PB.bars_for(O, run, (kind, label.split("/")[0]))
        if (kind, label.split("/")[0]) not in slipped:
            slipped.clear()                                    # the day loop's line shares the call's variant runs
            slipped[kind, label.split("/")[0]] = PB.slips_for(O, run, want)
        S = slipped[kind, label.split("/")[0]]
        got = hip(inp) if args.gpu else None
        s = summary.setdefault(kind, dict(cases=0, pairs=0, floor=0, cap=0, maxbar=0.0, maxbar_at="", minpower=float("inf"),
                                          minpower_at="", maxratio=0.0, maxratio_at="", over=0, exp46=[float("inf"), 0.0]))
        s["cases"] += 1
        dist = {}
        for k in want:
            line = f"{kind} {label} {k} {noise[k]:.2e} {bars[k]:.2e} " + " ".join(fmt(S[v][k]) for v in slips)
            s["pairs"] += 1
            s["floor"] += bars[k] == PB.FLOOR
            s["cap"] += bars[k] >= PB.CAP
            if bars[k] > s["maxbar"]:
                s["maxbar"], s["maxbar_at"] = bars[k], f"{label}:{k}"
            if got is not None:
                d = dist[k] = PB.distance(got[k], want[k]) if PB.same_pattern(got[k], want[k]) else float("inf")
                line += f" {fmt(d)} {d / bars[k]:.3f}"
                s["over"] += d > bars[k]
                if d / bars[k] > s["maxratio"]:
                    s["maxratio"], s["maxratio_at"] = d / bars[k], f"{label}:{k}"
            if args.per_variable:
                print(line)
        power = {}
        for v in slips:                                        # power: best variable of each slip that touches the case
            touched = [S[v][k] / bars[k] for k in want if S[v][k] > 0]
            power[v] = "-" if not touched else "pattern" if max(touched) == float("inf") else f"{max(touched):.3g}"
            if not touched:
                continue
            if v == "exp46":
                s["exp46"] = [min(s["exp46"][0], max(touched)), max(s["exp46"][1], max(touched))]
            elif max(touched) < s["minpower"]:
                s["minpower"], s["minpower_at"] = max(touched), f"{label}:{v}"
        if not args.per_variable:
            kb = max(want, key=lambda k: bars[k])
            line = f"{kind} {label} {len(want)} {kb} {noise[kb]:.2e} {bars[kb]:.2e} " + " ".join(power[v] for v in slips)
            if got is not None:
                kd = max(want, key=lambda k: dist[k] / bars[k])
                line += f" {kd} {fmt(dist[kd])} {bars[kd]:.2e} {dist[kd] / bars[kd]:.3f}"
            print(line)
        sys.stdout.flush()
    print("#\n# summary")
    for kind, s in summary.items():
        print(f"# {kind}: {s['cases']} cases, {s['pairs']} (case, variable) pairs, {s['floor']} at the floor, {s['cap']} at the cap; "
              f"largest bar {s['maxbar']:.2e} ({s['maxbar_at']}); smallest S/bar of a *32 slip that touches a case (best "
              f"variable) {s['minpower']:.3g} ({s['minpower_at']}); exp46 S/bar (best variable) {s['exp46'][0]:.3g} .. {s['exp46'][1]:.3g}"
              + (f"; largest d/bar {s['maxratio']:.3f} ({s['maxratio_at']}), {s['over']} pairs over their bar" if args.gpu else ""))


if __name__ == "__main__":
    main()
