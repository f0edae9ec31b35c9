#!/usr/bin/env python3
"""How far the compiled path's radGsw / radGlw lie from the published maps of the staged section (vignettes/images/image3.png,
digitised into tests/golden/vignette_stage_maps.json), cell by cell, in colour classes — written to
profiles/diag_image3_distances.txt.

    python tools/stage_map_distances.py            # CPU only

The values are the yardstick's (tests/stages_ref.c: the oracle's own twostream on the bundled site, monthly-tmax subset, entry
131; terrain planes from oracle/terrain_oracle.py), which the device's diagnostics follow to their parity bar (<= 1e-6 relative):
the distances below are hundreds of thousands of bars, so they are the device's too.  The sibling figure of the same run and hour
(image3b, downward short wave) is measured beside them as the control."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import stages_ref as SR                 # noqa: E402
import vignette_fixture as V            # noqa: E402
from bundled import load                # noqa: E402
from microclimf_amd import frontend as F    # noqa: E402
from oracle import terrain_oracle as TO     # noqa: E402


def stage_panel(k):
    p = json.loads((ROOT / "tests" / "golden" / "vignette_stage_maps.json").read_text())["maps"]["image3"]["panels"][k]
    cls, idx = np.array(p["classes"], float), np.array(p["cells"])
    lo = np.where(idx >= 0, cls[np.maximum(idx, 0), 0], np.nan)
    hi = np.where(idx >= 0, cls[np.maximum(idx, 0), 1], np.nan)
    return {"lo": lo, "hi": hi, "class_width": float(np.median(cls[:, 1] - cls[:, 0])), "legend": p["legend"], "what": p["what"]}


def per_cell(m, raster):
    with np.errstate(invalid="ignore"):
        return np.maximum(np.maximum(m["lo"] - raster, raster - m["hi"]), 0.0) / m["class_width"]


def main():
    weather, vegp, soilc, dtm = load()
    mx = F.subsetpointmodel(F.runpointmodel(weather, 0.05, dtm, vegp, soilc), what="tmax")
    t = TO.terrain(np.asarray(dtm["z"], float), float(dtm["res"]), float(mx["zref"]))
    a = F.prepare_grid_inputs(mx, 0.05, vegp, soilc, dtm, slr=t["slope"], apr=t["aspect"], hor=t["hor"], svf=t["svfa"], wsa=t["wsa"])
    r = SR.run(a)
    sw, lw = stage_panel(0), stage_panel(1)
    bar = 2.0 * V.map_panel("image3b", 0)["class_width"] / sw["class_width"]
    with np.errstate(invalid="ignore"):
        down = (r["Rbdown"] + r["Rddown"])[:, :, 130]
    lines = ["image3 (running-microclimf.Rmd:340-352, twostream(micro): radGsw[,,131], radGlw[,,131]) against the compiled path's values",
             f"bar of the map test the issue asked for: 2.0 x class_width(image3b panel 0) / class_width(image3 panel 0) = {bar:.3f} classes "
             f"of {sw['class_width']:.3f} W/m2 = {bar * sw['class_width']:.2f} W/m2", ""]
    for name, m, ras in (("image3 radGsw", sw, r["radGsw"][:, :, 130]), ("image3 radGlw", lw, r["radGlw"][:, :, 130]),
                         ("image3b downward short wave (control)", V.map_panel("image3b", 0), down)):
        d = per_cell(m, ras)
        ok = np.isfinite(d)
        q = np.percentile(d[ok], [50, 90, 99, 100])
        mid = 0.5 * (m["lo"] + m["hi"])
        with np.errstate(invalid="ignore"):
            bias = np.nanmedian(ras - mid)
        lines.append(f"{name}: {int(ok.sum())} cells, class width {m['class_width']:.3f} W/m2; distance in classes: median {q[0]:.2f}, p90 {q[1]:.2f}, "
                     f"p99 {q[2]:.2f}, max {q[3]:.2f}; within 1 class {np.mean(d[ok] <= 1):.3f}, within {bar:.0f} {np.mean(d[ok] <= bar):.3f}; "
                     f"median (model - published class centre) {bias:+.2f} W/m2")
        hist, edges = np.histogram(d[ok], bins=[0, 1, 2, 4, 8, 16, 32, 64])
        lines.append("    cells by distance (classes) " + ", ".join(f"[{int(a)},{int(b)}): {int(n)}" for a, b, n in zip(edges[:-1], edges[1:], hist)))
        worst = np.argsort(np.where(ok, d, -1).ravel())[::-1][:8]
        lines.append("    farthest cells (row, col from the north-west, 0-based: model / published class) " +
                     "; ".join(f"({i // 50},{i % 50}): {ras.ravel()[i]:.1f} / [{m['lo'].ravel()[i]:.1f}, {m['hi'].ravel()[i]:.1f}]" for i in worst))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    (ROOT / "profiles" / "diag_image3_distances.txt").write_text(text)


if __name__ == "__main__":
    main()
