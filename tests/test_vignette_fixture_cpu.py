"""tests/golden/vignette_points.json — the reference's published result figures, digitised by tools/digitize_vignette.py.
Here (no GPU): the fixture is self-consistent, the digitiser recovers a curve from a figure drawn in base R's style, and the
one published series that needs no GPU — the host-side point model of image1b — meets it.  The grid
solver's and the snow branch's curves — and the ten published raster maps, cell by cell — are compared in
tests/test_frontend_gpu.py::test_vignette_*."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

import vignette_fixture as V
from bundled import load
from microclimf_amd import frontend as F

ROOT = Path(__file__).resolve().parent.parent


def test_fixture_is_self_consistent():
    fx = json.loads(V.FIXTURE.read_text())["figures"]
    assert set(fx) == {"image1b", "image7", "image8", "image9", "image14a", "image14p", "image14b"}
    for name, f in fx.items():
        for p in f["panels"]:
            for ax in ("x", "y"):
                a = p[ax]
                assert a["fit_resid_px"] <= 0.75, (name, ax)            # printed labels sit on the detected ticks
                back = (np.array(a["tick_labels"]) - a["at_px0"]) / a["per_px"]
                assert np.abs(back - np.array(a["tick_px"])).max() <= 0.75
            fr = p["frame_px"]
            for c in p["curves"].values():
                assert c["columns"], name
                for x, flat in c["columns"]:
                    assert fr["left"] < x < fr["right"] and len(flat) % 2 == 0
                    assert all(fr["top"] < r < fr["bottom"] for r in flat)
    # the digitisation error per figure: one pixel in data units
    assert abs(fx["image9"]["panels"][0]["px"]["y"] - 0.0503) < 1e-3          # degC
    assert abs(fx["image14a"]["panels"][0]["px"]["y"] - 1.30) < 0.01          # mm of snow water equivalent


def test_map_fixtures_are_self_consistent():
    """the digitised raster maps: 50 x 50 cells each, the bundled site's 128 no-data cells white, the printed legend labels
    on the detected tick strokes, colour classes that tile the legend without gaps, every cell matched to a legend colour"""
    _, _, _, dtm = load()
    na = np.isnan(np.asarray(dtm["z"], dtype=float))
    mp = json.loads(V.FIXTURE.read_text())["maps"]
    assert set(mp) == {"image1a", "image2", "image3b", "image4", "image5", "image6", "image10", "image11"}
    assert sum(len(f["panels"]) for f in mp.values()) == 10
    for name, f in mp.items():
        for k, p in enumerate(f["panels"]):
            idx = np.array(p["cells"])
            assert idx.shape == (50, 50) and np.array_equal(idx < 0, na), (name, k)
            cls = np.array(p["classes"])
            assert idx.max() < len(cls) and (cls[:, 1] > cls[:, 0]).all()
            order = np.argsort(cls[:, 0])
            assert np.abs(cls[order][1:, 0] - cls[order][:-1, 1]).max() < 1e-5, (name, k)      # classes tile the legend
            for a in (p["x"], p["y"], p["legend"]):
                assert a["fit_resid_px"] <= 0.75, (name, k)
            assert p["worst_colour_distance"] <= 16
            m = V.map_panel(name, k)
            assert np.nanmin(m["lo"]) >= p["legend"]["min"] - 1e-6 and np.nanmax(m["hi"]) <= p["legend"]["max"] + 1e-6
    # the resolution this buys, in data units: one colour class
    assert abs(V.map_panel("image6")["class_width"] - 0.097) < 0.002          # degC
    assert abs(V.map_panel("image4")["class_width"] - 0.0100) < 0.0005        # m/s


def test_digitiser_recovers_a_drawn_figure(tmp_path, monkeypatch):
    """tools/digitize_vignette.py on a figure drawn here as base R draws a line plot — a 1 px black frame, 7 px tick strokes
    outside it, a red curve of known values: the frame, the ticks and the axis calibration are found exactly and the curve
    comes back to within the half pixel the drawing rounded it to"""
    sys.path.insert(0, str(ROOT / "tools"))
    import digitize_vignette as D
    from PIL import Image
    top, bot, left, right = 40, 240, 60, 360
    img = np.full((300, 400, 3), 255, np.uint8)
    img[[top, bot], left:right + 1] = 0
    img[top:bot + 1, [left, right]] = 0
    yt, xt = [220, 180, 140, 100, 60], [80, 140, 200, 260, 320]        # y = 0 at row 220, 10 per 40 rows; x = 0 at column 80, 100 per 60
    for r in yt:
        img[r, left - 7:left] = 0
    for c in xt:
        img[bot + 1:bot + 8, c] = 0
    cols = np.arange(left + 1, right)
    x = (cols - 80) * 100.0 / 60
    y = 20 + 15 * np.sin(x / 80)
    img[np.rint(220 - 4 * y).astype(int), cols] = (220, 30, 30)
    Image.fromarray(img).save(tmp_path / "drawn.png")
    monkeypatch.setattr(D, "IMAGES", tmp_path)
    spec = dict(rmd="-", what="a drawn figure", panels=[dict(xticks=[0, 100, 200, 300, 400], yticks=[0, 10, 20, 30, 40], x_is="index1",
                                                             y_is="degC", curves={"c": "red"})])
    p = D.digitize("drawn", spec)["panels"][0]
    assert p["frame_px"] == {"top": top, "bottom": bot, "left": left, "right": right}
    assert p["x"]["tick_px"] == xt and p["y"]["tick_px"] == yt                  # bottom label first
    assert abs(p["x"]["per_px"] - 100 / 60) < 1e-12 and abs(p["y"]["per_px"] + 0.25) < 1e-12
    assert p["x"]["fit_resid_px"] < 1e-9 and p["y"]["fit_resid_px"] < 1e-9
    got = p["curves"]["c"]["columns"]
    assert [c for c, _ in got] == list(cols) and all(len(flat) == 2 for _, flat in got)
    xr = np.array([c for c, _ in got]) * p["x"]["per_px"] + p["x"]["at_px0"]
    yr = np.array([flat[0] for _, flat in got]) * p["y"]["per_px"] + p["y"]["at_px0"]
    assert np.abs(xr - x).max() < 1e-9
    assert np.abs(yr - y).max() <= 0.5 * p["px"]["y"] + 1e-9


def test_point_model_series_meet_the_published_figure():
    """vignettes/images/image1b.png (running-microclimf.Rmd:283-292): ground and canopy temperature of `runpointmodel` over
    2017 — host code, so this pin needs no GPU.  1 px = 18.2 h x 0.115 degC; both directions within 2 px."""
    weather, vegp, soilc, dtm = load()
    dfo = F.runpointmodel(weather, 0.05, dtm, vegp, soilc)["dfo"]
    hours = np.arange(len(dfo["Tg"]), dtype=float)
    d = V.distances(V.panel("image1b"), "all", np.concatenate([hours, [np.nan], hours]),
                    np.concatenate([dfo["Tg"], [np.nan], dfo["Tc"]]))
    assert d["fig_to_model_max"] < 2.0 and d["model_to_fig_max"] < 2.0, (d["fig_to_model_max"], d["model_to_fig_max"])
