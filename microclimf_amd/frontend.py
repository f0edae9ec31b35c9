"""Host-side mirror of the reference's user-level calls for data.frame weather — `runpointmodel()`
(R/Cppwrappers.R:59-139) and `runmicro()` → `.runmicronosnow` → `.runmodel1Cpp` / `.runmodel3Cpp`
(R/Cppwrappers.R:376-397, R/internal.R:3290-3349, 1065-1169, 1345-1459) — for hosts without R.

In an R session these R functions keep running unchanged above the C ABI.  Here every step they take
between the user's rasters and the solver call is restated with numpy on top of libmcfhip's own producers:

    step of the reference                          here
    ---------------------------------------------  -----------------------------------------------------
    soilmCpp, BigLeafCpp, pointmprocess, manCpp     libmcfhip, host C++ (pointmodel.py)
    terra::terrain, .horizon, .windsheltera         mcf_precompute_terrain (device kernels, terrain.py)
    .topidx / flowaccCpp                            mcf_topidx (host C++)
    leafrfromalb, find_lref, find_gref, fill_naCpp  mcf_leafrfromalb_device (device kernels, vegprep.py)
    runmicro1Cpp / runmicro3Cpp                     mcf_runmicro1 / mcf_runmicro3 (the hot path)
    a loop of runmicro over reqhgt (the vignette)   mcf_runmicro_heights: one plan, .foliageden per height on the device (k_foliage)
    .sortvegp, .soilinit, .foliageden, .satvap ...  numpy, below, citing the R lines they follow

Rasters are numpy arrays `[rows, cols]` (or `[rows, cols, layers]`), row 0 = northern edge as in terra; what a
SpatRaster carries besides values is passed as `dtm = {"z": array, "res": xres | (xres, yres), "lat": ., "long": .}`
(the reference gets lat / long from the CRS through sf/PROJ, `.latlongfromraster`, R/internal.R:61-69).
`checkinputs()` (R/dataprep.R) is not mirrored: inputs are taken as checked (`runchecks = FALSE`).
"""
from __future__ import annotations

import warnings
from types import SimpleNamespace
from typing import Mapping, Sequence

import numpy as np

from . import api, ncsink, pointmodel, terrain
from .vegprep import fill_na, find_gref, find_lref, leafrfromalb      # noqa: F401  (leafrfromalb(), R/dataprep.R:1000-1050)
from .soil_tables import SOILPARAMETERS, SOILPARAMSP
from .rformulas import dewpoint_R as _dewpoint, satvap_R as _satvap   # .satvap / .dewpoint, R/internal.R:501-521

WEATHER = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "winddir", "precip")


# ---- small R helpers --------------------------------------------------------------------------------------------
def getmode(v):
    """`.getmode` (R/internal.R:107-111): most frequent non-NA value, the first seen on ties."""
    v = np.asarray(v, dtype=np.float64).ravel(order="F")
    v = v[~np.isnan(v)]
    if v.size == 0:
        return np.nan
    u, first, counts = np.unique(v, return_index=True, return_counts=True)
    order = np.argsort(first)                      # unique() in R keeps first-appearance order
    return float(u[order][np.argmax(counts[order])])


def r_round(x):
    """R's round(x, 0): half to even"""
    return np.rint(x)


def layer_index(nr: int, n: int):
    """`s <- round(seq(0.50001, nr + 0.5, length.out = n), 0)` clipped to 1..nr (R/internal.R:188-191); 1-based"""
    s = r_round(np.linspace(0.50001, nr + 0.5, n)) if n > 1 else r_round(np.array([0.50001]))
    return np.clip(s, 1, nr).astype(int)


def as3d(a):
    a = np.asarray(a, dtype=np.float64)
    return a[:, :, None] if a.ndim == 2 else a


def intr(a, n: int, subs):
    """`.intr` (R/internal.R:187-195): pick, for each of `n` time steps, the nearest of the raster's layers"""
    a = as3d(a)
    s = layer_index(a.shape[2], n)[np.asarray(subs) - 1]
    return a[:, :, s - 1]


def spline_fmm(y, n: int):
    """`stats::spline(y, n = n)$y` for x = 1..length(y): the cubic spline of Forsythe, Malcolm & Moler (1977), whose
    end conditions fit cubics through the first and the last four points, evaluated at `n` equally spaced abscissae
    (R's default `method = "fmm"`, `xmin = min(x)`, `xmax = max(x)`)."""
    y = np.asarray(y, dtype=np.float64)
    m = len(y)
    x = np.arange(1.0, m + 1.0)
    xo = np.linspace(1.0, float(m), n)
    if m < 2:
        return np.full(n, y[0] if m else np.nan)
    b, c, d = np.zeros(m), np.zeros(m), np.zeros(m)
    if m < 3:
        b[:] = (y[1] - y[0]) / (x[1] - x[0])
    else:
        d[0] = x[1] - x[0]
        c[1] = (y[1] - y[0]) / d[0]
        for i in range(1, m - 1):
            d[i] = x[i + 1] - x[i]
            b[i] = 2.0 * (d[i - 1] + d[i])
            c[i + 1] = (y[i + 1] - y[i]) / d[i]
            c[i] = c[i + 1] - c[i]
        b[0], b[m - 1] = -d[0], -d[m - 2]
        c[0] = c[m - 1] = 0.0
        if m > 3:
            c[0] = c[2] / (x[3] - x[1]) - c[1] / (x[2] - x[0])
            c[m - 1] = c[m - 2] / (x[m - 1] - x[m - 3]) - c[m - 3] / (x[m - 2] - x[m - 4])
            c[0] = c[0] * d[0] * d[0] / (x[3] - x[0])
            c[m - 1] = -c[m - 1] * d[m - 2] * d[m - 2] / (x[m - 1] - x[m - 4])
        for i in range(1, m):                       # Gaussian elimination
            t = d[i - 1] / b[i - 1]
            b[i] = b[i] - t * d[i - 1]
            c[i] = c[i] - t * c[i - 1]
        c[m - 1] = c[m - 1] / b[m - 1]              # back substitution
        for i in range(m - 2, -1, -1):
            c[i] = (c[i] - d[i] * c[i + 1]) / b[i]
        b[m - 1] = (y[m - 1] - y[m - 2]) / d[m - 2] + d[m - 2] * (c[m - 2] + 2.0 * c[m - 1])
        for i in range(m - 1):
            b[i] = (y[i + 1] - y[i]) / d[i] - d[i] * (c[i + 1] + 2.0 * c[i])
            d[i] = (c[i + 1] - c[i]) / d[i]
            c[i] = 3.0 * c[i]
        c[m - 1] = 3.0 * c[m - 1]
        d[m - 1] = d[m - 2]
    i = np.clip(np.searchsorted(x, xo, side="right") - 1, 0, m - 1)
    dx = xo - x[i]
    return y[i] + dx * (b[i] + dx * (c[i] + dx * d[i]))


# ---- vegetation -------------------------------------------------------------------------------------------------
VEG_KEYS = ("hgt", "pai", "x", "gsmax", "leafr", "clump", "leafd", "leaft")


def vegpdmx(vegp) -> int:
    """`.vegpdmx` (R/internal.R:197-208)"""
    return max(as3d(vegp[k]).shape[2] for k in VEG_KEYS)


def sortvegp_point(vegp) -> np.ndarray:
    """`.sortvegp(vegp, method = "P")` (R/internal.R:229-239): the point model's vegetation vector"""
    m = {k: float(np.nanmean(np.asarray(vegp[k], dtype=np.float64))) for k in VEG_KEYS}
    return np.array([m["hgt"], m["pai"], m["x"], m["clump"], m["leafr"], m["leaft"], m["leafd"], 0.97, m["gsmax"], 100.0])


def sortvegp_grid(vegp, n: int, subs):
    """`.sortvegp(vegp, method = "C", n, subs)` (R/internal.R:249-273): every variable expanded to the layers of the
    variable with most layers, and `lsubs`, the layer of each time step with whole days never split"""
    subs = np.asarray(subs)
    dmx = vegpdmx(vegp)
    s = layer_index(dmx, n)
    first = []
    for v in s[subs - 1]:                              # unique(s[subs]) keeps first-appearance order
        if v not in first:
            first.append(int(v))
    out = {k: intr(vegp[k], dmx, np.array(first)) for k in VEG_KEYS}
    ss = s[subs - 1]
    if len(ss) % 24:
        raise ValueError("the grid model needs whole days (matrix(s, ncol = 24) in .sortvegp)")
    sdd = np.array([getmode(row) for row in ss.reshape(-1, 24)]).astype(int)
    out["lsubs"] = np.repeat(sdd, 24)
    return out


def foliageden(z, hgt, pai, paia=None, shape: float = 1.5, rate: float | None = None):
    """`.foliageden` (R/internal.R:937-946): gamma-shaped foliage profile -> leaf density at z and plant area above z"""
    from scipy.stats import gamma
    rate = shape / 7 if rate is None else rate
    g = gamma(a=shape, scale=1.0 / rate)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = ((hgt - z) / hgt) * 10
        td = g.cdf(10)
        rfd = g.pdf(x) / td
        tdf = (pai / hgt) * rfd * 10
        if paia is None:
            paia = g.cdf(x) * (pai / td)
    return tdf, paia


def cleanvars(vegp, soilc, dtm_z):
    """`.cleanvars` (R/internal.R:1020-1063): one NA mask for everything; zero pai where pai or hgt is zero or a
    vegetation parameter is missing.  (`.cleanr(vegp$hgt, 0)` there sets cell 0 — nothing — so hgt keeps its values.)"""
    veg = {k: as3d(vegp[k]).copy() for k in VEG_KEYS}
    soil = {k: np.asarray(v, dtype=np.float64).copy() for k, v in soilc.items()}
    z = np.asarray(dtm_z, dtype=np.float64).copy()
    na = (np.isnan(veg["pai"][:, :, 0]) | np.isnan(veg["hgt"][:, :, 0]) | np.isnan(soil["soiltype"])
          | np.isnan(soil["groundr"]) | np.isnan(z))
    for k in VEG_KEYS:
        veg[k][na] = np.nan
    for k in ("soiltype", "groundr"):
        soil[k][na] = np.nan
    z[na] = np.nan
    with np.errstate(invalid="ignore"):
        zero = (veg["pai"][:, :, 0] == 0) | (veg["hgt"][:, :, 0] == 0)
    for k in ("gsmax", "leafr", "clump", "leafd", "leaft"):
        zero |= np.isnan(veg[k][:, :, 0])
    veg["pai"][zero] = 0.0
    veg["pai"][na] = np.nan                              # mask(vegp$pai, dtm)
    veg["hgt"][na] = np.nan
    return veg, soil, z


# ---- soil -------------------------------------------------------------------------------------------------------
def soilinit(soilc) -> dict:
    """`.soilinit` (R/internal.R:304-336): per-cell soil constants from the soil type unless given explicitly"""
    st = np.asarray(soilc["soiltype"], dtype=np.float64)
    num = np.array(SOILPARAMETERS["Number"])
    out = {}
    for name, col in (("rho", "rho"), ("Vm", "Vm"), ("Vq", "Vq"), ("Mc", "Mc"), ("psi_e", "psi_e"), ("soilb", "b"),
                      ("Smax", "Smax"), ("Smin", "Smin")):
        if col in soilc:
            out[name] = np.asarray(soilc[col], dtype=np.float64)
            continue
        a = np.full(st.shape, np.nan)
        tab = np.array(SOILPARAMETERS[col])
        for u in np.unique(st[~np.isnan(st)]):
            a[st == u] = tab[num == u][0]
        out[name] = a
    return out


def sortsoilc_point(soilc) -> np.ndarray:
    """`.sortsoilc(soilc, "P")` (R/internal.R:338-357): the point model's ground vector (BigLeafCpp reads 12 entries)"""
    sl = soilinit(soilc)
    sn = int(getmode(soilc["soiltype"]))
    return np.array([getmode(soilc["groundr"]), 0.0, 180.0, 0.97, getmode(sl["rho"]), getmode(sl["Vm"]), getmode(sl["Vq"]),
                     getmode(sl["Mc"]), getmode(sl["soilb"]), getmode(sl["psi_e"]), getmode(sl["Smax"]), getmode(sl["Smin"]),
                     SOILPARAMSP["alpha"][sn - 1], SOILPARAMSP["n"][sn - 1], SOILPARAMSP["Ksat"][sn - 1]])


# ---- runpointmodel ----------------------------------------------------------------------------------------------
def soilbelowT(dfo: Mapping, reqhgt: float) -> np.ndarray:
    """`.soilbelowT` (R/internal.R:169-185)"""
    n = -118.35 * reqhgt / dfo["DDp"]
    nmn, nmx = int(np.floor(n.min())), int(np.ceil(n.max()))
    # manCpp's circular mean reads outside its array when the window exceeds the series (the reference then returns
    # whatever lies there); windows are capped at the whole days available
    cap = max(24 * (len(n) // 24), 1) if len(n) >= 48 else len(n)
    nmn, nmx = max(1, min(nmn, cap)), max(1, min(nmx, cap))
    Tnmn, Tnmx = pointmodel.manCpp(dfo["Tg"], nmn), pointmodel.manCpp(dfo["Tg"], nmx)
    if nmx == nmn:                                  # capped windows: one mean serves both
        Tb = Tnmn
    else:
        wgt = np.clip((n - nmn) / (nmx - nmn), 0.0, 1.0)
        Tb = wgt * Tnmx + (1 - wgt) * Tnmn
    wgt2 = 0.041596 * (reqhgt / np.mean(dfo["DDp"])) + 0.87142
    return wgt2 * Tb + (1 - wgt2) * np.mean(dfo["Tg"])


def runpointmodel(weather: Mapping, reqhgt: float, dtm: Mapping, vegp: Mapping, soilc: Mapping, *, zref: float = 2.0,
                  windhgt: float | None = None, soilm=None, matemp: float | None = None, dTmx: float = 25.0,
                  maxiter: int = 20, yearG: bool = True, lat: float | None = None, long: float | None = None,
                  vegp_p=None, groundp_p=None, soiltype: int | None = None, mxhgt: float | None = None) -> dict:
    """`runpointmodel(weather, reqhgt, dtm, vegp, soilc, ...)` (R/Cppwrappers.R:59-139).  `weather`: the columns of the
    reference's `climdata` plus `obstime = {year, month, day, hour}` in place of the POSIX `obs_time`."""
    w = {k: np.array(weather[k], dtype=np.float64, copy=True) for k in WEATHER if k in weather}
    obstime = {k: np.asarray(weather["obstime"][k]) for k in ("year", "month", "day", "hour")}
    n = len(w["temp"])
    windhgt = zref if windhgt is None else windhgt
    if matemp is None:
        matemp = float(np.mean(w["temp"]))
    if zref != windhgt:
        w["windspeed"] = w["windspeed"] * np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    if n < 8760:
        yearG = False
    vegp_p = sortvegp_point(vegp) if vegp_p is None else np.asarray(vegp_p, dtype=np.float64)
    groundp_p = sortsoilc_point(soilc) if groundp_p is None else np.asarray(groundp_p, dtype=np.float64)
    if mxhgt is None:
        mxhgt = float(np.nanmax(np.asarray(vegp["hgt"], dtype=np.float64)))
    zout = mxhgt if mxhgt > 2 else 2.0
    lat = dtm["lat"] if lat is None else lat
    long = dtm["long"] if long is None else long
    if zout > zref:
        w2 = pointmodel.weatherhgtCpp(obstime, w, zref, zout, zout, lat, long)
        if not np.isnan(np.mean(w2["temp"])):
            w = w2
        zref = zout
    w["windspeed"] = np.maximum(w["windspeed"], 0.5)
    if soilm is None:
        ii = (int(getmode(soilc["soiltype"])) if soiltype is None else int(soiltype)) - 1
        p = SOILPARAMSP
        sd = pointmodel.soilmCpp(w, p["rmu"][ii], p["mult"][ii], p["pwr"][ii], p["Smax"][ii], p["Smin"][ii], p["Ksat"][ii],
                                 p["a"][ii])
        soilm = spline_fmm(sd, n)
    soilm = np.asarray(soilm, dtype=np.float64)
    bl = pointmodel.BigLeafCpp(obstime, w, vegp_p, groundp_p, soilm, lat, long, dTmx, zref, maxiter, 0.5, 0.5, 0.1, yearG)
    pp = pointmodel.pointmprocess({"windspeed": w["windspeed"], "tc": w["temp"], "rh": w["relhum"], "pk": w["pres"],
                                   "uf": bl["uf"], "soilm": soilm, "RabsG": bl["RabsG"]},
                                  zref, vegp_p[0], vegp_p[1], groundp_p[4], groundp_p[5], groundp_p[6], groundp_p[7])
    dfo = dict(pp)
    dfo.update(G=bl["G"], soilm=soilm, Tg=bl["Tg"], Tc=bl["Tc"])
    Tbz = soilbelowT(dfo, reqhgt) if reqhgt < 0 else None
    return {"weather": w, "obstime": obstime, "dfo": dfo, "Tbz": Tbz, "lat": lat, "long": long, "zref": zref,
            "subs": np.arange(1, n + 1), "ntme": n, "matemp": matemp, "bigleaf_err": bl["err"]}


# ---- runmicro ---------------------------------------------------------------------------------------------------
def _dfsel(lsubs) -> dict:
    """`.runmodel3Cpp`'s layer table (R/internal.R:1391-1399) from the layer of every step of the series it solves: the layers in
    use renumbered 1, 2, ... in their order, each with the whole days its steps span (0-based steps st .. ed)"""
    lyr = []
    for v in lsubs:
        if v not in lyr:
            lyr.append(int(v))
    st, ed = [], []
    for v in lyr:
        s = np.nonzero(lsubs == v)[0] + 1                                # 1-based positions
        st.append(int(np.floor(s[0] / 24) * 24))
        ed.append(int(np.floor(s[-1] / 24) * 24 - 1))
    return {"lyr": np.arange(1, len(lyr) + 1), "st": np.array(st), "ed": np.array(ed)}


def subset_day_layers(micropoint: Mapping, vegp: Mapping, soilc: Mapping, dtm: Mapping, days) -> np.ndarray | None:
    """The vegetation layer (0-based row of the layered arrays) `.runmodel3Cpp` / `.runmodel4Cpp` solve each of the 1-based
    `days` of a complete micropoint with when they are handed the day SUBSET, as `.runmicronosnow` does: one entry per day of the
    whole series, -1 for the days that are not in the subset; None when the vegetation has a single layer.
    Two things make this differ from the whole-series table.  `.sortvegp` cuts the layered arrays to `unique(s[subs])`, the
    layers some STEP of the subset has, in their order; the layer table has one row per layer that is some DAY's mode
    (`_dfsel`), and the solver walks the cut arrays by ROW of that table.  Row r therefore reads the r-th layer of
    `unique(s[subs])`, which is the table's own layer only as long as the two lists agree: a layer that keeps a few steps of
    the subset without being a day's mode puts every later row one layer early, a layer that loses all its steps does not.
    The entries returned are rows of the WHOLE series' arrays (`unique(s)` of every step)."""
    veg = cleanvars(vegp, soilc, dtm["z"])[0]
    if as3d(veg["pai"]).shape[2] <= 1:
        return None
    sub = subsetpointmodel(micropoint, days=days)
    n, subs = sub["ntme"], np.asarray(sub["subs"])
    s = layer_index(vegpdmx(veg), n)

    def unique(v):                                                        # first-appearance order, as sortvegp_grid
        out = []
        for x in v:
            if x not in out:
                out.append(int(x))
        return out
    first_sub, first_whole = unique(s[subs - 1]), unique(s)
    t = _dfsel(sortvegp_grid(veg, n, subs)["lsubs"])
    days = np.asarray(days, dtype=np.int64)
    lod_sub = np.full(days.size, -1, dtype=np.int32)
    for row, (st, ed) in enumerate(zip(t["st"], t["ed"])):
        d0, nd = st // 24, (ed - st + 1) // 24
        lod_sub[d0:min(d0 + nd, days.size)] = first_whole.index(first_sub[row])      # (the solver's day -> layer map: later rows win)
    lod = np.full(micropoint["ntme"] // 24, -1, dtype=np.int32)
    lod[days - 1] = lod_sub
    return lod


def prepare_grid_inputs(micropoint: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, pai_a=None,
                        out: Sequence = (1,) * 10, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None,
                        device: int = 0, from_dtm: bool = False, foliage: bool = True) -> dict:
    """Everything `.runmodel1Cpp` / `.runmodel3Cpp` do before calling the solver (R/internal.R:1067-1166 / 1347-1456):
    returns the keyword arguments of runmicro1Cpp, plus `dfsel` when the vegetation varies in time.  `from_dtm`: those of
    slr, apr, hor, twi, wsa, svf that are not given are left out of `soilc` and `dtm` = {z, res} is returned with the
    arguments instead: the solver's plan derives them on the device (api.runmicro1Cpp, `dtm`).  `foliage=False` leaves
    vegp$leafden and vegp$paia out (no `.foliageden` on the host): the height-profile entries derive them on the device."""
    res = dtm["res"]
    xres, yres = (res, res) if np.isscalar(res) else res
    if xres != yres:
        raise ValueError("the horizon / wind-shelter pre-compute works on z / res with one resolution, as the reference's "
                         ".horizon does (R/internal.R:909-925): square cells only")
    veg, soil, z = cleanvars(vegp, soilc, dtm["z"])
    w = micropoint["weather"]
    clim = {k: np.asarray(w[k], dtype=np.float64) for k in ("temp", "pres", "swdown", "difrad", "lwdown", "windspeed", "winddir")}
    clim["es"] = _satvap(clim["temp"])
    clim["ea"] = clim["es"] * np.asarray(w["relhum"], dtype=np.float64) / 100
    clim["tdew"] = _dewpoint(clim["ea"], clim["temp"])
    dfo = micropoint["dfo"]
    nt = len(clim["temp"])
    pointm = {k: np.asarray(dfo[k], dtype=np.float64) for k in ("soilm", "Tg", "T0p", "G", "DDp", "umu", "kp", "muGp", "dtrp")}
    pointm["Tbp"] = np.asarray(micropoint["Tbz"], dtype=np.float64) if reqhgt < 0 else np.zeros(nt)
    n, subs = micropoint["ntme"], micropoint["subs"]
    sv = sortvegp_grid(veg, n, subs)
    lsubs = sv.pop("lsubs")
    with np.errstate(invalid="ignore"):
        sv["hgt"][sv["pai"] == 0] = 0.0
        sv["pai"][sv["hgt"] == 0] = 0.0
    if pai_a is not None:
        pai_a = intr(pai_a, n, subs)
    if foliage:
        sv["leafden"], sv["paia"] = foliageden(reqhgt, sv["hgt"], sv["pai"], pai_a)
    layers = sv["pai"].shape[2]
    dfsel = None
    if layers > 1:                                                       # R/internal.R:1391-1399
        dfsel = _dfsel(lsubs)
    else:
        sv = {k: v[:, :, 0] for k, v in sv.items()}
    sl = soilinit(soil)
    sc = {"gref": soil["groundr"], "Smin": sl["Smin"], "Smax": sl["Smax"], "soilb": sl["soilb"], "Psie": sl["psi_e"],
          "Vq": sl["Vq"], "Vm": sl["Vm"], "Mc": sl["Mc"], "rho": sl["rho"]}
    na = np.isnan(z)
    need = [k for k, v in (("slope", slr), ("aspect", apr), ("hor", hor), ("svfa", svf), ("wsa", wsa)) if v is None]
    ter = terrain.precompute_terrain(z, xres, micropoint["zref"], what=tuple(need), device=device) if need and not from_dtm else {}
    for k, given in (("slope", slr), ("aspect", apr)):
        if given is None and from_dtm:
            continue
        a = np.array(ter[k] if given is None else given, dtype=np.float64, copy=True)
        a[np.isnan(a)] = 0.0
        a[na] = np.nan
        sc[k] = a
    if not (twi is None and from_dtm):
        t = np.array(terrain.topidx(z, (xres, yres)) if twi is None else twi, dtype=np.float64, copy=True)
        t[np.isnan(t)] = 1.0
        t[na] = np.nan
        sc["twi"] = t
    for k, given in (("hor", hor), ("svfa", svf), ("wsa", wsa)):
        if not (given is None and from_dtm):
            sc[k] = ter[k] if given is None else np.asarray(given, dtype=np.float64)
    out = [int(bool(v)) for v in out]
    if reqhgt == 0:
        out = [a * b for a, b in zip((1, 0, 0, 1, 0, 1, 1, 1, 1, 1), out)]
    if reqhgt < 0:
        out = [a * b for a, b in zip((1, 0, 0, 1, 0, 0, 0, 0, 0, 0), out)]
    args = dict(obstime=micropoint["obstime"], climdata=clim, pointm=pointm, vegp=sv, soilc=sc, reqhgt=float(reqhgt),
                zref=float(micropoint["zref"]), lat=float(micropoint["lat"]), lon=float(micropoint["long"]),
                Sminp=getmode(sc["Smin"]), Smaxp=getmode(sc["Smax"]), tfact=1.5, complete=len(subs) == n,
                mat=float(micropoint["matemp"]), out=out)
    if dfsel is not None:
        args["dfsel"] = dfsel
    if from_dtm:
        args["dtm"] = {"z": z, "res": (xres, yres)}
    return args


def runmicro(micropoint: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, pai_a=None,
             tfact: float = 1.5, out: Sequence = (1,) * 10, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None,
             device: int = 0, from_dtm: bool = False) -> dict:
    """`runmicro(micropoint, reqhgt, vegp, soilc, dtm, ...)` for data.frame weather without snow: time-invariant
    vegetation goes to runmicro1Cpp, layered vegetation to runmicro3Cpp (R/internal.R:3332-3346).  `from_dtm`: every one of
    slr, apr, hor, twi, wsa, svf that is not given is derived on the device inside the solver's plan instead of on the host
    first (opt-in: the wetness index then differs from the host's in the last bits of atan / tan)."""
    a = prepare_grid_inputs(micropoint, reqhgt, vegp, soilc, dtm, pai_a=pai_a, out=out, slr=slr, apr=apr, hor=hor, twi=twi,
                            wsa=wsa, svf=svf, device=device, from_dtm=from_dtm)
    a["tfact"] = float(tfact)
    dfsel = a.pop("dfsel", None)
    if dfsel is None:
        return api.runmicro1Cpp(**a, device=device)
    return api.runmicro3Cpp(dfsel, **a, device=device)


def nc_extent(dtm: Mapping, rows: int, cols: int, r0: int = 0, c0: int = 0) -> dict:
    """The mapping ncsink.writetonc takes as `dtm` for rows [r0, r0 + rows) x columns [c0, c0 + cols) of the raster `dtm`
    ("xmin", "ymax", "res"[, "crs"]; row 0 is the northern edge)"""
    res = dtm["res"] if np.isscalar(dtm["res"]) else dtm["res"][0]
    return {"xmin": dtm["xmin"] + c0 * res, "xmax": dtm["xmin"] + (c0 + cols) * res, "ymin": dtm["ymax"] - (r0 + rows) * res,
            "ymax": dtm["ymax"] - r0 * res, "res": res, "crs": dtm.get("crs", "")}


def runmicro_nc(micropoint: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, fileout: str, *, vars=None,
                format: str = "classic", deflate_level: int = 0, pai_a=None, tfact: float = 1.5, slr=None, apr=None, hor=None, twi=None,
                wsa=None, svf=None, device: int = 0, devices=None, n_blocks: int = 0, days_per_chunk: int = 0, extent: Mapping | None = None):
    """`runmicro()` followed by `writetonc()` without the arrays in between (include/mcf.h mcf_runmicro_nc): data.frame weather,
    any reqhgt — below ground the streamed plan — every chunk packed on the device and written while the next is solved.  `vars`:
    writetonc's default for the height.  `dtm` needs "xmin", "ymax" besides "z" / "res" for the file's coordinates (`extent`: the
    mapping itself, for a tile of a larger raster).  `devices` / `n_blocks`: row blocks, each writing its strips (classic
    container).  -> the file's variable names; the classic file is byte for byte ncsink.writetonc(runmicro(...))."""
    names = tuple(ncsink.default_vars(reqhgt) if vars is None else vars)
    out = [1 if n in names else 0 for n in api._abi.OUT_NAMES]
    a = prepare_grid_inputs(micropoint, reqhgt, vegp, soilc, dtm, pai_a=pai_a, out=out, slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa,
                            svf=svf, device=device)
    a["tfact"] = float(tfact)
    a.pop("out")
    rows, cols = np.shape(as3d(a["vegp"]["hgt"])[:, :, 0])
    return api.runmicro_nc(**a, fileout=fileout, grid=nc_extent(dtm, rows, cols) if extent is None else extent, vars=names, format=format,
                           deflate_level=deflate_level, device=device, devices=devices, n_blocks=n_blocks, days_per_chunk=days_per_chunk)


def runmicro_depths_nc(micropoint: Mapping, depths, vegp: Mapping, soilc: Mapping, dtm: Mapping, files, *, soilm: bool = True,
                       format: str = "classic", deflate_level: int = 0, pai_a=None, tfact: float = 1.5, slr=None, apr=None, hor=None,
                       twi=None, wsa=None, svf=None, device: int = 0, days_per_chunk: int = 0) -> None:
    """runmicro_depths into one `writetonc` file per depth (include/mcf.h mcf_runmicro_depths_nc): files[d] holds Tz at depths[d]
    under that depth's long name and, with soilm, the soil moisture.  `dtm` as for runmicro_nc."""
    a, depths, tbp = _depth_inputs(micropoint, depths, vegp, soilc, dtm, pai_a, tfact, dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf), device)
    rows, cols = np.shape(as3d(a["vegp"]["hgt"])[:, :, 0])
    api.runmicro_depths_nc(**a, depths=depths, tbp=tbp, files=files, grid=nc_extent(dtm, rows, cols), soilm=soilm, format=format,
                           deflate_level=deflate_level, device=device, days_per_chunk=days_per_chunk)


# ---- period summaries: monthly (yearly, daily, ...) maps straight from the device ------------------------------------------------
def summary_periods(obstime: Mapping, by="month"):
    """The period of every whole day of an hourly `obstime` (taken from the first of the day's 24 rows) for
    include/mcf.h's period summaries -> (int32 table [days], labels [nperiods]).  `by`: "all" (one period), "year", "month"
    (year-month, in order of appearance), "monthofyear" (all Januaries together, ...: the months present, ascending), "day",
    or an explicit array with one integer per day (-1: not counted)."""
    year, month, day = (np.asarray(obstime[k]).astype(np.int64) for k in ("year", "month", "day"))
    nd = len(year) // 24
    y, m, d = year[:nd * 24:24], month[:nd * 24:24], day[:nd * 24:24]
    if not isinstance(by, str):
        tab = np.asarray(by).astype(np.int32).ravel()
        if tab.size != nd:
            raise ValueError(f"periods: one entry per whole day ({nd}), got {tab.size}")
        if tab.size and tab.min() < -1:
            raise ValueError("periods: entries are period indices >= 0, or -1 for a day that is not counted")
        return tab, list(range(int(tab.max()) + 1 if tab.size and tab.max() >= 0 else 1))
    if by == "all":
        return np.zeros(nd, dtype=np.int32), ["all"]
    if by == "monthofyear":
        months = sorted(set(m.tolist()))
        return np.array([months.index(v) for v in m.tolist()], dtype=np.int32), months
    keys = {"year": lambda i: (int(y[i]),), "month": lambda i: (int(y[i]), int(m[i])),
            "day": lambda i: (int(y[i]), int(m[i]), int(d[i]))}
    if by not in keys:
        raise ValueError('periods: "all", "year", "month", "monthofyear", "day" or one integer per day')
    seen, tab = {}, np.empty(nd, dtype=np.int32)
    for i in range(nd):
        tab[i] = seen.setdefault(keys[by](i), len(seen))
    fmt = {"year": "{:04d}", "month": "{:04d}-{:02d}", "day": "{:04d}-{:02d}-{:02d}"}[by]
    return tab, ([k[0] for k in seen] if by == "year" else [fmt.format(*k) for k in seen])


def _out_mask(vars, allow_none: bool = True):
    """-> (the names, the solver's ten `out` flags) for output names (one name or several); a name that is no output is refused,
    and with `allow_none` False an empty selection too"""
    names = (vars,) if isinstance(vars, str) else tuple(vars)
    out = [1 if n in names else 0 for n in api._abi.OUT_NAMES]
    if sum(out) != len(set(names)) or not (names or allow_none):
        raise ValueError(f"vars: names of {api._abi.OUT_NAMES}")
    return names, out


def runmicro_summary(micropoint, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, periods="month",
                     vars: Sequence = ("Tz",), stats: Sequence = ("mean", "min", "max"), thresholds=None, pai_a=None,
                     tfact: float = 1.5, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0,
                     from_dtm: bool = False, crows: int | None = None, ccols: int | None = None, lats=None, lons=None,
                     altcorrect: int = 0, dtmc=None, chunk_days: int = 0, devices=None, n_blocks: int = 0) -> dict:
    """`runmicro()` reduced over time on the device: per-cell statistics (`stats`, names of api._abi.STAT_NAMES) of the outputs
    `vars` over `periods` (see summary_periods) instead of the [rows, cols, steps] arrays — what apply(mout$Tz, c(1, 2), mean)
    and monthly mean / minimum / maximum maps need, without cells x steps values ever leaving the solver's ring.  A micropoint
    (data.frame weather) or, with `crows`, `ccols`, `lats`, `lons`, the list of micropoints of runpointmodela (array weather,
    as runmicro_array).  reqhgt == 0 masks the variables as runmicro does; reqhgt < 0 is not available.
    -> {variable: {statistic: [rows, cols, nperiods]}, "periods": labels, "days": counted days per period}"""
    if reqhgt < 0:
        raise ValueError("period summaries need reqhgt >= 0 (below ground: runmicro_depths_summary)")
    names, out = _out_mask(vars)
    ter = dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf)
    array = not isinstance(micropoint, Mapping)
    if array:
        if crows is None or ccols is None or lats is None or lons is None:
            raise ValueError("a list of micropoints (array weather) needs crows, ccols, lats and lons")
        if from_dtm:
            raise ValueError("from_dtm is not available with array weather")
        a = prepare_grid_inputs_array(micropoint, crows, ccols, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons, pai_a=pai_a, out=out,
                                      device=device, **ter)
        coarse = api._coarse_spec(a["vegp"], a["climdata"], None, None, altcorrect, dtmc,
                                  cleanvars(vegp, soilc, dtm["z"])[2] if altcorrect else None, refuse_missing=False)
        extra = dict(array_forcing=True, coarse=coarse)
    else:
        a = prepare_grid_inputs(micropoint, reqhgt, vegp, soilc, dtm, pai_a=pai_a, out=out, device=device, from_dtm=from_dtm, **ter)
        extra = dict(devices=devices, n_blocks=n_blocks)
        if from_dtm:
            extra["dtm"] = a.pop("dtm")
    a["tfact"] = float(tfact)
    kept = [n for n, o in zip(api._abi.OUT_NAMES, a.pop("out")) if o]      # (reqhgt == 0: tleaf, relhum and windspeed are masked)
    if not kept:
        raise ValueError("none of the selected variables exists at this reqhgt")
    tab, labels = summary_periods(a["obstime"], periods)
    res = api.runmicro_summary(**a, periods=tab, nperiods=len(labels), vars=kept, stats=stats, thresholds=thresholds,
                               chunk_days=chunk_days, device=device, **extra)
    res["periods"] = labels
    return res


# ---- series at logger sites and per-step zonal statistics, straight from the device -------------------------------------------------
def series_cells(dtm: Mapping, rows: int, cols: int, points=None, xy=None) -> np.ndarray:
    """0-based cell indices row + rows * col of `points` ((row, col) pairs) followed by those of `xy` (map coordinates (x, y),
    placed with dtm["xmin"], dtm["ymax"] and dtm["res"] as runmicro_big lays out its files: row 0 is the northern edge).  A
    point or coordinate outside the raster is a ValueError."""
    cells = []
    if points is not None:
        for r, c in np.asarray(points, dtype=np.int64).reshape(-1, 2):
            if not (0 <= r < rows and 0 <= c < cols):
                raise ValueError(f"points: ({r}, {c}) is outside the {rows} x {cols} raster")
            cells.append(int(r) + rows * int(c))
    if xy is not None:
        res = dtm["res"]
        xres, yres = (res, res) if np.isscalar(res) else res
        for x, y in np.asarray(xy, dtype=np.float64).reshape(-1, 2):
            c, r = int(np.floor((x - dtm["xmin"]) / xres)), int(np.floor((dtm["ymax"] - y) / yres))
            if not (0 <= r < rows and 0 <= c < cols):
                raise ValueError(f"xy: ({x}, {y}) is outside the raster")
            cells.append(int(r) + rows * int(c))
    return np.asarray(cells, dtype=np.int64)


def runmicro_series(micropoint, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, points=None, xy=None, zones=None,
                    vars: Sequence = ("Tz",), stats: Sequence = ("mean", "min", "max"), pai_a=None, tfact: float = 1.5, slr=None,
                    apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0, from_dtm: bool = False,
                    crows: int | None = None, ccols: int | None = None, lats=None, lons=None, altcorrect: int = 0, dtmc=None,
                    chunk_days: int = 0) -> dict:
    """`runmicro()` reduced over space on the device: the hourly series of `vars` at logger sites — `points` ((row, col) pairs)
    and / or `xy` (map coordinates, see series_cells) — and their per-step statistics `stats` (names of api._abi.ZSTAT_NAMES)
    over `zones`, a [rows, cols] integer array of labels 0 .. 63 (negative or masked: in no zone) — what terra::zonal or
    global(..., na.rm = TRUE) over mout$Tz give layer by layer, without cells x steps values ever leaving the solver's ring.
    The other arguments as for runmicro_summary.  reqhgt == 0 masks the variables as runmicro does; reqhgt < 0 is not available.
    -> {"points": {variable: [tsteps, npoints]}, "zones": {variable: {statistic: [tsteps, nzones]}}, "cells": the points' cell
    indices row + rows * col}"""
    if reqhgt < 0:
        raise ValueError("the series sink needs reqhgt >= 0")
    names, out = _out_mask(vars)
    if any(s not in api._abi.ZSTAT_NAMES for s in ((stats,) if isinstance(stats, str) else stats)):
        raise ValueError(f"stats: names of {api._abi.ZSTAT_NAMES}")
    rows, cols = np.asarray(dtm["z"]).shape[:2]
    cells = series_cells(dtm, rows, cols, points, xy)
    ter = dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf)
    array = not isinstance(micropoint, Mapping)
    plan_kw = {}
    if array:
        if crows is None or ccols is None or lats is None or lons is None:
            raise ValueError("a list of micropoints (array weather) needs crows, ccols, lats and lons")
        if from_dtm:
            raise ValueError("from_dtm is not available with array weather")
        a = prepare_grid_inputs_array(micropoint, crows, ccols, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons, pai_a=pai_a, out=out,
                                      device=device, **ter)
        coarse = api._coarse_spec(a["vegp"], a["climdata"], None, None, altcorrect, dtmc,
                                  cleanvars(vegp, soilc, dtm["z"])[2] if altcorrect else None, refuse_missing=False)
        extra = dict(array_forcing=True, coarse=coarse)
    else:
        a = prepare_grid_inputs(micropoint, reqhgt, vegp, soilc, dtm, pai_a=pai_a, out=out, device=device, from_dtm=from_dtm, **ter)
        extra = {}
        if from_dtm:
            plan_kw["dtm"] = a.pop("dtm")
    a["tfact"] = float(tfact)
    kept = [n for n, o in zip(api._abi.OUT_NAMES, a.pop("out")) if o]      # (reqhgt == 0: tleaf, relhum and windspeed are masked)
    if not kept:
        raise ValueError("none of the selected variables exists at this reqhgt")
    sel = dict(points=cells if cells.size else None, zones=zones, vars=kept, stats=stats)
    if plan_kw:      # missing terrain planes derived on the device: the plan API from here, as runmicro_summary's dtm route
        nd = len(np.asarray(a["obstime"]["year"])) // 24
        ring = max(1, min(nd, int(chunk_days) if chunk_days else 8))
        with api.Plan(**a, out=[n in kept for n in api._abi.OUT_NAMES], ring_days=ring, device=device, **plan_kw) as p:
            vs, ss = p.series_enable(**sel)
            for d0 in range(0, nd, ring):
                p.run_days(d0, min(ring, nd - d0), 0)
                p.series_accumulate(0, 0, d0, min(ring, nd - d0))
            res = {"points": {v: p.fetch_point_series(v) for v in vs} if cells.size else {},
                   "zones": {v: {s: p.fetch_zone_series(v, s) for s in ss} for v in vs} if zones is not None else {}}
    else:
        res = api.runmicro_series(**a, **sel, chunk_days=chunk_days, device=device, **extra)
    res["cells"] = cells
    return res


# ---- below ground at several depths from one solve ---------------------------------------------------------------------------------
def _depth_inputs(micropoint, depths, vegp, soilc, dtm, pai_a, tfact, ter, device):
    """runmicro1Cpp's arguments at depths[0] with `depths` in place of reqhgt, and the point model's soil temperature at every
    depth: below ground the solver's work does not depend on the depth, only the tail of Tbelowgroundv does"""
    depths = [float(d) for d in np.atleast_1d(np.asarray(depths, dtype=np.float64))]
    if not depths or not all(d < 0 for d in depths):
        raise ValueError("depths: one or more heights below ground (each < 0)")
    tbp = np.stack([soilbelowT(micropoint["dfo"], d) for d in depths])
    a = prepare_grid_inputs(dict(micropoint, Tbz=tbp[0]), depths[0], vegp, soilc, dtm, pai_a=pai_a, out=(1, 0, 0, 1, 0, 0, 0, 0, 0, 0),
                            device=device, **ter)
    a["tfact"] = float(tfact)
    a.pop("out")
    a.pop("reqhgt")
    return a, depths, tbp


def runmicro_depths(micropoint: Mapping, depths, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, pai_a=None, tfact: float = 1.5,
                    slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0, days_per_chunk: int = 0) -> dict:
    """`runmicro()` at several depths below ground from ONE run of the solver (include/mcf.h mcf_runmicro_depths): a soil
    temperature profile costs one run, not one per depth.  `depths`: each < 0, any order, at most api._abi.MAX_DEPTHS.  The
    point model's soil temperature at each depth comes from `.soilbelowT` on the micropoint.
    -> {"Tz": [one [rows, cols, steps] array per depth], "soilm": [rows, cols, steps], "depths": depths}, each array with
    the bits of runmicro(micropoint, depth, ...) on a micropoint of that depth."""
    a, depths, tbp = _depth_inputs(micropoint, depths, vegp, soilc, dtm, pai_a, tfact, dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf), device)
    return api.runmicro_depths(**a, depths=depths, tbp=tbp, device=device, days_per_chunk=days_per_chunk)


def runmicro_depths_summary(micropoint: Mapping, depths, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, periods="month",
                            vars: Sequence = ("Tz",), stats: Sequence = ("mean", "min", "max"), thresholds=None, pai_a=None,
                            tfact: float = 1.5, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0,
                            chunk_days: int = 0) -> dict:
    """runmicro_depths reduced over time on the device, as runmicro_summary reduces runmicro: monthly (...) soil-temperature
    maps at several depths without a cells x steps array anywhere.  `vars` among "Tz" and "soilm".
    -> {"Tz": [per depth {statistic: [rows, cols, nperiods]}], "soilm": {statistic: ...} (if selected), "periods", "days",
    "depths"}"""
    names = (vars,) if isinstance(vars, str) else tuple(vars)
    if not names or any(n not in ("Tz", "soilm") for n in names):
        raise ValueError('vars: below ground "Tz" and "soilm" can be summarised')
    a, depths, tbp = _depth_inputs(micropoint, depths, vegp, soilc, dtm, pai_a, tfact, dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf), device)
    tab, labels = summary_periods(a["obstime"], periods)
    res = api.runmicro_depths_summary(**a, depths=depths, tbp=tbp, periods=tab, nperiods=len(labels), vars=names, stats=stats,
                                      thresholds=thresholds, chunk_days=chunk_days, device=device)
    res["periods"] = labels
    return res


def runmicro_depths_series(micropoint: Mapping, depths, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, points=None, xy=None,
                           zones=None, vars: Sequence = ("Tz",), stats: Sequence = ("mean", "min", "max"), pai_a=None,
                           tfact: float = 1.5, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0,
                           chunk_days: int = 0) -> dict:
    """runmicro_depths reduced over space on the device, as runmicro_series reduces runmicro: the hourly soil temperature at
    logger sites (`points`, `xy`: see series_cells) and per-step statistics over `zones` at several depths, without a
    cells x steps array anywhere.  `vars` among "Tz" and "soilm".
    -> {"Tz": [per depth {"points": [tsteps, npoints], "zones": {statistic: [tsteps, nzones]}}], "soilm": {...} (if selected),
    "depths", "cells"}"""
    names = (vars,) if isinstance(vars, str) else tuple(vars)
    if not names or any(n not in ("Tz", "soilm") for n in names):
        raise ValueError('vars: below ground "Tz" and "soilm" have a series')
    if any(s not in api._abi.ZSTAT_NAMES for s in ((stats,) if isinstance(stats, str) else stats)):
        raise ValueError(f"stats: names of {api._abi.ZSTAT_NAMES}")
    rows, cols = np.asarray(dtm["z"]).shape[:2]
    cells = series_cells(dtm, rows, cols, points, xy)
    a, depths, tbp = _depth_inputs(micropoint, depths, vegp, soilc, dtm, pai_a, tfact, dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf), device)
    res = api.runmicro_depths_series(**a, depths=depths, tbp=tbp, points=cells if cells.size else None, zones=zones, vars=names,
                                     stats=stats, chunk_days=chunk_days, device=device)
    res["cells"] = cells
    return res


# ---- height profiles from one plan ----------------------------------------------------------------------------------------------
def _height_inputs(micropoint, heights, vegp, soilc, dtm, pai_a, tfact, ter, device, out=(1,) * 10):
    """runmicro1Cpp's (runmicro3Cpp's) arguments without reqhgt and without the two foliage planes, the heights, and `pai_a` per
    height dealt to the time steps as prepare_grid_inputs deals runmicro's"""
    heights = [float(h) for h in np.atleast_1d(np.asarray(heights, dtype=np.float64))]
    if not heights or not all(h > 0 for h in heights):
        raise ValueError("heights: one or more heights above ground (each > 0; the ground surface: runmicro, below ground: "
                         "runmicro_depths)")
    if pai_a is not None and len(pai_a) != len(heights):
        raise ValueError(f"pai_a: one entry per height ({len(heights)}), each None or the plant area above that height")
    a = prepare_grid_inputs(micropoint, heights[0], vegp, soilc, dtm, out=out, device=device, foliage=False, **ter)
    a["tfact"] = float(tfact)
    a.pop("reqhgt")
    if pai_a is not None:
        n, subs = micropoint["ntme"], micropoint["subs"]
        pai_a = [None if p is None else intr(p, n, subs) for p in pai_a]
    return a, heights, pai_a


def runmicro_heights(micropoint: Mapping, heights, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, pai_a=None, tfact: float = 1.5,
                     out: Sequence = (1,) * 10, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0,
                     days_per_chunk: int = 0) -> dict:
    """`runmicro()` at several heights above ground from ONE plan (include/mcf.h mcf_runmicro_heights): the vignette's loop over
    `reqhgt` without repeating the terrain pre-compute, the wetness index, the uploads, the plan and the ring per height.  A
    height is still a full solve (the canopy's own absorbed radiation depends on the foliage above the height); what only
    depends on the height — vegp$paia and vegp$leafden — is derived on the device.  `heights`: each > 0; `pai_a`: None, or one
    entry per height, each None or the plant area above that height.
    -> {"heights": heights, "Tz": [one [rows, cols, steps] array per height], ...: likewise for every requested variable}"""
    a, heights, pai_a = _height_inputs(micropoint, heights, vegp, soilc, dtm, pai_a, tfact,
                                       dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf), device, out)
    return api.runmicro_heights(**a, heights=heights, pai_a=pai_a, device=device, days_per_chunk=days_per_chunk)


def runmicro_heights_summary(micropoint: Mapping, heights, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, periods="month",
                             vars: Sequence = ("Tz",), stats: Sequence = ("mean", "min", "max"), thresholds=None, pai_a=None,
                             tfact: float = 1.5, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0,
                             chunk_days: int = 0) -> dict:
    """runmicro_heights reduced over time on the device, as runmicro_summary reduces runmicro: one plan with period summaries,
    per height set_height, summary_reset, the accumulate loop and the fetches.
    -> {"heights": heights, variable: [per height {statistic: [rows, cols, nperiods]}], "periods": labels, "days": counted days}"""
    names, out = _out_mask(vars, allow_none=False)
    a, heights, pai_a = _height_inputs(micropoint, heights, vegp, soilc, dtm, pai_a, tfact,
                                       dict(slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf), device, out)
    tab, labels = summary_periods(a["obstime"], periods)
    # (a plan is created with both foliage planes in place: zeros, which set_height replaces before the first run)
    a["vegp"] = dict(a["vegp"], paia=np.zeros_like(a["vegp"]["pai"]), leafden=np.zeros_like(a["vegp"]["pai"]))
    nd = len(tab)
    ring = max(1, min(nd, int(chunk_days) if chunk_days else 8))
    res = {"heights": np.array(heights), "periods": labels}
    with api.Plan(**a, reqhgt=heights[0], ring_days=ring, device=device) as p:
        vi, si = p.summary_enable(tab, names, stats, thresholds, nperiods=len(labels))
        for h, hgt in enumerate(heights):
            p.set_height(hgt, None if pai_a is None else pai_a[h])
            p.summary_reset()
            p.summarise_days(ring)
            for v in vi:
                res.setdefault(v, []).append({s: p.fetch_summary(v, s) for s in si})
            res["days"] = p.summary_days()
    return res


# ---- the staged workflow: modelin -> soilmdistribute -> twostream -> wind -> soiltemp -> aboveground / belowground ------------
# The reference's R-mode stages (R/Rimplementation.R:70-342) let a user look inside a run.  Here every stage reads the
# COMPILED path's own intermediates — the solver's diagnostics ring (include/mcf.h mcf_diag): the values that produce the ten
# outputs of the same run, with one solar position per time step and runmicro1Cpp's soil-moisture clamp, not the R mode's
# per-cell solar position and its clamp.  One diagnostics solve per (reqhgt, pai_a, tfact) serves all stages; it is made when
# the first stage needs device values and kept in `micro`.
STAGE_FIELDS = {1: ("soilm",),
                2: ("radGsw", "radGlw", "radCsw", "radClw", "radLsw", "radLpar", "lwout", "Rbdown", "Rddown", "Rdup", "si"),
                3: ("uf", "uz", "gHa"),
                4: ("Tg", "T0", "G", "kDDg")}
_STAGE_OUTPUT = {"soilm": "soilm", "Rbdown": "Rdirdown", "Rddown": "Rdifdown", "Rdup": "Rswup", "uz": "windspeed"}   # from the ten outputs


def modelin(micropoint, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, slr=None, apr=None, hor=None, twi=None, wsa=None,
            svf=None, device: int = 0) -> dict:
    """`modelin(micropoint, vegp, soilc, dtm)` for data.frame weather (R/Rimplementation.R:70-77): the prepared grid inputs
    (prepare_grid_inputs: cleaned vegetation and soil, the terrain planes, the wetness index), `progress = 0` and `tme`."""
    if not isinstance(micropoint, Mapping):
        raise NotImplementedError("modelin: a list of micropoints (array weather) needs the climate grid's shape and the "
                                  "raster's lats / lons — see modelina")
    inputs = prepare_grid_inputs(micropoint, 0.05, vegp, soilc, dtm, slr=slr, apr=apr, hor=hor, twi=twi, wsa=wsa, svf=svf,
                                 device=device)
    return {"inputs": inputs, "progress": 0, "tme": micropoint["obstime"], "device": device,
            "_src": (micropoint, vegp, soilc, dtm), "_runs": {}}


def modelina(micropointa: Sequence, crows: int, ccols: int, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, lats, lons, dtmc=None,
             altcorrect: int = 0, slr=None, apr=None, hor=None, twi=None, wsa=None, svf=None, device: int = 0) -> dict:
    """`modelin(micropoint, vegp, soilc, dtm, dtmc, altcorrect)` for a list of micropoints from `runpointmodela` (array weather:
    `.modelina`, R/internal.R:645): the prepared grid inputs with the climate and point-model variables left on the coarse grid
    (prepare_grid_inputs_array), `progress = 0` and `tme`.  The stage functions work on the result as on modelin's; `altcorrect`
    1 / 2 with `dtmc` [crows, ccols] as in runmicro_array.  Below ground is refused as runmicro_array refuses it."""
    if isinstance(micropointa, Mapping):
        raise ValueError("modelina takes the list of micropoints of runpointmodela: see modelin for data.frame weather")
    if altcorrect and dtmc is None:
        raise ValueError("altcorrect needs dtmc, the elevations of the climate cells")
    inputs = prepare_grid_inputs_array(micropointa, crows, ccols, 0.05, vegp, soilc, dtm, lats=lats, lons=lons, slr=slr, apr=apr,
                                       hor=hor, twi=twi, wsa=wsa, svf=svf, device=device)
    return {"inputs": inputs, "progress": 0, "tme": micropointa[0]["obstime"], "device": device,
            "_src": (micropointa, vegp, soilc, dtm), "_runs": {},
            "_array": {"crows": int(crows), "ccols": int(ccols), "lats": lats, "lons": lons, "dtmc": dtmc, "altcorrect": int(altcorrect)}}


def _stage_key(reqhgt, pai_a, tfact):
    return (max(float(reqhgt), 0.0), None if pai_a is None else np.asarray(pai_a, dtype=np.float64).tobytes(), float(tfact))


def _stage_run(micro: dict, reqhgt, pai_a, tfact) -> dict:
    """the diagnostics solve of (reqhgt, pai_a, tfact): the ten outputs and, under "diag", the thirteen diagnostics.  The ground
    sees neither reqhgt nor the foliage above it, so a below-ground height is served by the solve at reqhgt = 0."""
    key = _stage_key(reqhgt, pai_a, tfact)
    if key not in micro["_runs"]:
        micropoint, vegp, soilc, dtm = micro["_src"]
        sc = micro["inputs"]["soilc"]      # the terrain planes made by modelin are handed back: nothing is derived twice
        terrain = dict(slr=sc["slope"], apr=sc["aspect"], hor=sc["hor"], twi=sc["twi"], wsa=sc["wsa"], svf=sc["svfa"])
        if "_array" in micro:              # modelina: the coarse one-shot with the diagnostics beside the outputs
            res = _run_array(micropoint, reqhgt=key[0], vegp=vegp, soilc=soilc, dtm=dtm, tfact=tfact, pai_a=pai_a, **terrain,
                             device=micro["device"], diag="all", **micro["_array"])
        else:
            a = prepare_grid_inputs(micropoint, key[0], vegp, soilc, dtm, pai_a=pai_a, **terrain, device=micro["device"])
            a["tfact"] = float(tfact)
            dfsel = a.pop("dfsel", None)
            if dfsel is None:
                res = api.runmicro1Cpp(**a, device=micro["device"], diag="all")
            else:
                res = api.runmicro3Cpp(dfsel, **a, device=micro["device"], diag="all")
        micro["_runs"][key] = res
    micro["_last"] = key
    return micro["_runs"][key]


def _stage(micro: dict, level: int, reqhgt, pai_a, tfact) -> dict:
    res = _stage_run(micro, reqhgt, pai_a, tfact)
    for lv in range(1, level + 1):
        for name in STAGE_FIELDS[lv]:
            if name in _STAGE_OUTPUT:
                if _STAGE_OUTPUT[name] in res:       # (windspeed is not an output at reqhgt = 0, as in the reference)
                    micro[name] = res[_STAGE_OUTPUT[name]]
            else:
                micro[name] = res["diag"]["T0" if name == "Tg" else name]
    micro["progress"] = max(micro["progress"], level)
    return micro


def soilmdistribute(micro: dict, reqhgt: float = 0.05, pai_a=None, tfact: float = 1.5) -> dict:
    """adds `soilm`, the soil moisture spread by the wetness index (R/Rimplementation.R:97-118); progress 1"""
    return _stage(micro, 1, reqhgt, pai_a, tfact)


def twostream(micro: dict, reqhgt: float = 0.05, pai_a=None, tfact: float = 1.5) -> dict:
    """adds radGsw, radGlw, radCsw, radClw, radLsw, radLpar, lwout, Rbdown, Rddown, Rdup and si (R/Rimplementation.R:136-176,
    twostreamgrid); progress 2.  Runs soilmdistribute if it has not run."""
    return _stage(micro, 2, reqhgt, pai_a, tfact)


def wind(micro: dict, reqhgt: float = 0.05, pai_a=None, tfact: float = 1.5) -> dict:
    """adds uf, gHa and (reqhgt > 0) uz (R/Rimplementation.R:202-218, windgrid); progress 3"""
    return _stage(micro, 3, reqhgt, pai_a, tfact)


def soiltemp(micro: dict, reqhgt: float = 0.05, pai_a=None, tfact: float = 1.5) -> dict:
    """adds the ground surface temperature (`Tg`, under the reference's list name `T0` too), the ground heat flux `G` and the
    damping depth `kDDg` (R/Rimplementation.R:242-256, soiltempgrid); progress 4"""
    return _stage(micro, 4, reqhgt, pai_a, tfact)


def aboveground(micro: dict, reqhgt: float = 0.05, pai_a=None, tfact: float = 1.5) -> dict:
    """the reference's eleven arrays (R/Rimplementation.R:291-303, abovegrid): runmicro's ten — those the height has — plus `T0`,
    all from the one diagnostics solve of (reqhgt, pai_a, tfact)"""
    if reqhgt < 0:
        raise ValueError("aboveground needs reqhgt >= 0: see belowground")
    if micro["progress"] < 4 or micro.get("_last") != _stage_key(reqhgt, pai_a, tfact):
        soiltemp(micro, reqhgt, pai_a, tfact)
    res = _stage_run(micro, reqhgt, pai_a, tfact)
    out = {k: v for k, v in res.items() if k != "diag"}
    out["T0"] = res["diag"]["T0"]
    return out


def belowground(micro: dict, reqhgt: float = -0.05, pai_a=None, tfact: float = 1.5) -> dict:
    """Tz, T0 and soilm (R/Rimplementation.R:331-342, belowgrid): Tz and soilm from the below-ground solve of runmicro, T0 from
    the kept diagnostics solve (the ground's temperature does not depend on reqhgt)"""
    if reqhgt >= 0:
        raise ValueError("belowground needs reqhgt < 0: see aboveground")
    if "_array" in micro:
        raise ValueError(_ARRAY_BELOW)
    if micro["progress"] < 4 or micro.get("_last") != _stage_key(reqhgt, pai_a, tfact):
        soiltemp(micro, reqhgt, pai_a, tfact)
    micropoint, vegp, soilc, dtm = micro["_src"]
    sc = micro["inputs"]["soilc"]
    below = runmicro(micropoint, reqhgt, vegp, soilc, dtm, pai_a=pai_a, tfact=tfact, out=(1, 0, 0, 1, 0, 0, 0, 0, 0, 0),
                     slr=sc["slope"], apr=sc["aspect"], hor=sc["hor"], twi=sc["twi"], wsa=sc["wsa"], svf=sc["svfa"],
                     device=micro["device"])
    return {"Tz": below["Tz"], "T0": _stage_run(micro, reqhgt, pai_a, tfact)["diag"]["T0"], "soilm": below["soilm"]}


# ---- array weather: runpointmodela() and runmicro() -> .runmodel2Cpp / .runmodel4Cpp ------------------------------
def block_reduce(a, crows: int, ccols: int, how: str = "mean"):
    """A fine raster [rows, cols(, layers)] summarised per coarse cell (the fine cells whose centres fall in it):
    stands for `.resampler(r2, r)` = terra aggregate + resample (R/internal.R:358-380; terra semantics unpinned)."""
    a = as3d(a)
    R, Cc, L = a.shape
    ri = np.minimum((np.arange(R) + 0.5) * crows / R, crows - 1).astype(int)
    ci = np.minimum((np.arange(Cc) + 0.5) * ccols / Cc, ccols - 1).astype(int)
    out = np.full((crows, ccols, L), np.nan)
    for i in range(crows):
        for j in range(ccols):
            blk = a[np.ix_(ri == i, ci == j)].reshape(-1, L)
            for l in range(L):
                v = blk[:, l]
                v = v[~np.isnan(v)]
                if v.size:
                    out[i, j, l] = getmode(v) if how == "mode" else v.mean()
    return out


def runpointmodela(climarray: Mapping, obstime: Mapping, reqhgt: float, dtm: Mapping, vegp: Mapping, soilc: Mapping, *,
                   lats, lons, matemp: float | None = None, zref: float = 2.0, windhgt: float = 2.0, soilm=None,
                   dTmx: float = 25.0, maxiter: int = 20, yearG: bool = True, device: int | None = None) -> list:
    """`runpointmodela(climarrayr, tme, reqhgt, dtm, vegp, soilc, ...)` (R/Cppwrappers.R:208-263): the point model once
    per cell of the coarse climate grid.  `climarray[k]`: [crows, ccols, T]; `lats`, `lons`: [crows, ccols] (the reference
    takes them from the climate raster's CRS).  Returns the row-major list of micropoints (None where the cell has no
    data), as the reference's `pointo`.  `device` = None: one cell at a time on the host, as the reference does; an int:
    the cells with data as ONE batch on that device (weatherhgt_batch, BigLeafBatch, pointmprocess_batch; whole days
    only), with the soil moisture model and `.soilbelowT` per cell on the host as before."""
    cr, cc, T = np.shape(climarray["temp"])
    mxhgt = float(np.nanmax(np.asarray(vegp["hgt"], dtype=np.float64)))
    wdir = np.array([getmode(np.asarray(climarray["winddir"])[:, :, k]) for k in range(T)])
    vc = {k: block_reduce(vegp[k], cr, cc) for k in VEG_KEYS}
    st = block_reduce(soilc["soiltype"], cr, cc, "mode")[:, :, 0]
    soiltype = int(getmode(st))
    gr = float(np.nanmean(np.asarray(soilc["groundr"], dtype=np.float64)))
    P = SOILPARAMETERS
    out = []
    batch = []                                    # device: (list position, weather, vegp_p, groundp_p, soilm, lat, long)
    for i in range(cr):
        for j in range(cc):
            if np.isnan(climarray["temp"][i, j, 0]) or np.isnan(vc["hgt"][i, j, 0]):
                out.append(None)
                continue
            w = {k: np.asarray(climarray[k])[i, j, :] for k in WEATHER if k != "winddir"}
            w["winddir"] = wdir
            w["obstime"] = obstime
            m = {k: float(np.mean(vc[k][i, j, :])) for k in VEG_KEYS}                                   # .tovp
            vegp_p = np.array([m["hgt"], m["pai"], m["x"], m["clump"], m["leafr"], m["leaft"], m["leafd"], 0.97, m["gsmax"], 100.0])
            sn = int(st[i, j]) - 1                                                                       # .togp
            groundp_p = np.array([gr, 0.0, 180.0, 0.97, P["rho"][sn], P["Vm"][sn], P["Vq"][sn], P["Mc"][sn], P["b"][sn],
                                  P["psi_e"][sn], P["Smax"][sn], P["Smin"][sn], P["Smin"][sn], P["Smin"][sn], P["Smin"][sn]])
            if device is not None:
                batch.append((len(out), w, vegp_p, groundp_p, None if soilm is None else np.asarray(soilm)[i, j, :],
                              float(lats[i, j]), float(lons[i, j])))
                out.append(None)
                continue
            out.append(runpointmodel(w, reqhgt, dtm, vegp, soilc, zref=zref, windhgt=windhgt,
                                     soilm=None if soilm is None else np.asarray(soilm)[i, j, :], matemp=matemp, dTmx=dTmx,
                                     maxiter=maxiter, yearG=yearG, lat=float(lats[i, j]), long=float(lons[i, j]),
                                     vegp_p=vegp_p, groundp_p=groundp_p, soiltype=soiltype, mxhgt=mxhgt))
    if batch:
        for (pos, *_), m in zip(batch, _runpointmodel_batch(batch, obstime, reqhgt, zref=zref, windhgt=windhgt,
                                                            matemp=matemp, dTmx=dTmx, maxiter=maxiter, yearG=yearG,
                                                            soiltype=soiltype, mxhgt=mxhgt, device=int(device))):
            out[pos] = m
    return out


def _runpointmodel_batch(batch, obstime, reqhgt, *, zref, windhgt, matemp, dTmx, maxiter, yearG, soiltype, mxhgt,
                         device) -> list:
    """`runpointmodel` for the cells of `runpointmodela` as one batch on the device: the same steps in the same order,
    the three point-model operators through their `_batch` entries."""
    obst = {k: np.asarray(obstime[k]) for k in ("year", "month", "day", "hour")}
    ws = [{k: np.array(b[1][k], dtype=np.float64, copy=True) for k in WEATHER if k in b[1]} for b in batch]
    n = len(ws[0]["temp"])
    lat = np.array([b[5] for b in batch])
    lon = np.array([b[6] for b in batch])
    windhgt = zref if windhgt is None else windhgt
    mat = [float(np.mean(w["temp"])) if matemp is None else matemp for w in ws]
    if zref != windhgt:
        for w in ws:
            w["windspeed"] = w["windspeed"] * np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    if n < 8760:
        yearG = False
    cols = ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed")
    zout = mxhgt if mxhgt > 2 else 2.0
    if zout > zref:
        w2 = pointmodel.weatherhgt_batch(obst, {k: np.stack([w[k] for w in ws]) for k in cols}, zref, zout, zout, lat, lon,
                                         device=device)
        for p, w in enumerate(ws):
            if not np.isnan(np.mean(w2["temp"][p])):
                for k in ("temp", "relhum", "windspeed"):
                    w[k] = w2[k][p].copy()
        zref = zout
    sms = []
    for b, w in zip(batch, ws):
        w["windspeed"] = np.maximum(w["windspeed"], 0.5)
        sm = b[4]
        if sm is None:
            ii = int(soiltype) - 1
            p = SOILPARAMSP
            sd = pointmodel.soilmCpp(w, p["rmu"][ii], p["mult"][ii], p["pwr"][ii], p["Smax"][ii], p["Smin"][ii], p["Ksat"][ii],
                                     p["a"][ii])
            sm = spline_fmm(sd, n)
        sms.append(np.asarray(sm, dtype=np.float64))
    W = {k: np.stack([w[k] for w in ws]) for k in cols}
    SM = np.stack(sms)
    vp = np.stack([b[2] for b in batch])
    gp = np.stack([b[3] for b in batch])
    bl = pointmodel.BigLeafBatch(obst, W, vp, gp, SM, lat, lon, dTmx, zref, maxiter, 0.5, 0.5, yearG, device=device)
    pp = pointmodel.pointmprocess_batch({"windspeed": W["windspeed"], "tc": W["temp"], "rh": W["relhum"], "pk": W["pres"],
                                         "uf": bl["uf"], "soilm": SM, "RabsG": bl["RabsG"]},
                                        zref, vp[:, 0], vp[:, 1], gp[:, 4], gp[:, 5], gp[:, 6], gp[:, 7], device=device)
    res = []
    for p, w in enumerate(ws):
        dfo = {k: pp[k][p].copy() for k in pp}
        dfo.update(G=bl["G"][p].copy(), soilm=sms[p], Tg=bl["Tg"][p].copy(), Tc=bl["Tc"][p].copy())
        Tbz = soilbelowT(dfo, reqhgt) if reqhgt < 0 else None
        res.append({"weather": w, "obstime": obst, "dfo": dfo, "Tbz": Tbz, "lat": float(lat[p]), "long": float(lon[p]),
                    "zref": zref, "subs": np.arange(1, n + 1), "ntme": n, "matemp": mat[p], "bigleaf_err": float(bl["err"][p])})
    return res


def prepare_grid_inputs_array(micropointa: Sequence, crows: int, ccols: int, reqhgt: float, vegp: Mapping, soilc: Mapping,
                              dtm: Mapping, *, lats, lons, pai_a=None, out: Sequence = (1,) * 10, slr=None, apr=None,
                              hor=None, twi=None, wsa=None, svf=None, device: int = 0) -> dict:
    """What `.runmodel2Cpp` / `.runmodel4Cpp` prepare (R/internal.R:1175-1343) with the climate and
    point-model variables left on the coarse grid: the solver interpolates them (array_forcing == 2; the altitude
    correction is applied there too, see runmicro_array).  `lats`, `lons`:
    [rows, cols] of the fine raster (`.latslonsfromr(dtm)`).  Cells of the coarse grid without a micropoint are not
    supported (the reference fills them with NA and lets `resample` look around them)."""
    if any(m is None for m in micropointa):
        raise ValueError("every coarse cell needs a micropoint")
    first = micropointa[0]
    base = prepare_grid_inputs(first, reqhgt, vegp, soilc, dtm, pai_a=pai_a, out=out, slr=slr, apr=apr, hor=hor, twi=twi,
                               wsa=wsa, svf=svf, device=device)
    grid = lambda get: _stack_micropoints(micropointa, crows, ccols, get)                      # noqa: E731
    clim = {k: grid(lambda m, k=k: m["weather"][k]) for k in ("temp", "relhum", "pres", "swdown", "difrad", "lwdown",
                                                                "windspeed", "winddir")}
    pm = {"soilm": "soilm", "Gp": "G", "umu": "umu", "kp": "kp", "muGp": "muGp", "dtrp": "dtrp"}
    pointm = {k: grid(lambda m, v=v: m["dfo"][v]) for k, v in pm.items()}
    base.update(climdata=clim, pointm=pointm, lat=np.asfortranarray(lats, dtype=np.float64),
                lon=np.asfortranarray(lons, dtype=np.float64), zref=float(first["zref"]),
                mat=float(np.mean([m["matemp"] for m in micropointa])))
    return base


def runmicro_array(micropointa: Sequence, crows: int, ccols: int, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping,
                   *, lats, lons, tfact: float = 1.5, altcorrect: int = 0, dtmc=None, device: int = 0, **kw) -> dict:
    """`runmicro()` for a list of micropoints from `runpointmodela` (array weather, no snow).  `altcorrect` 1 / 2 with
    `dtmc` [crows, ccols], the elevations of the climate cells: the lapse-rate correction of R/internal.R:1233-1251."""
    return _run_array(micropointa, crows, ccols, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons, tfact=tfact, altcorrect=altcorrect,
                      dtmc=dtmc, device=device, **kw)


_ARRAY_BELOW = "coarse array forcing below ground needs the per-cell point-model series: not mirrored"


def _run_array(micropointa, crows, ccols, reqhgt, vegp, soilc, dtm, *, lats, lons, tfact=1.5, altcorrect=0, dtmc=None, device=0,
               diag=None, **kw) -> dict:
    """runmicro_array, and — `diag` — the same solve with the staged model's diagnostics under "diag" (modelina's stages)"""
    if reqhgt < 0:
        raise ValueError(_ARRAY_BELOW)
    a = prepare_grid_inputs_array(micropointa, crows, ccols, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons, device=device, **kw)
    a["tfact"] = float(tfact)
    dfsel = a.pop("dfsel", None)
    coarse = api._coarse_spec(a["vegp"], a["climdata"], None, None, altcorrect, dtmc,
                              cleanvars(vegp, soilc, dtm["z"])[2] if altcorrect else None, refuse_missing=False)
    order = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact",
             "complete", "mat", "out")
    fn = "mcf_runmicro2" if dfsel is None else "mcf_runmicro4"
    return api._run(fn, True, *[a[k] for k in order], device, 0, 0, dfsel, coarse, diag=diag)


# ---- snow: runsnowmodel() -> .snowmodel1 --------------------------------------------------------------------------
def cleanvegp(vegp):
    """`.cleanvegp` (R/internal.R:121-139): no plant area on zero-height cells and the other way round, so that the
    snow model does not return NAs"""
    veg = {k: as3d(vegp[k]).copy() for k in VEG_KEYS}
    hm = veg["hgt"][:, :, 0]
    for l in range(veg["pai"].shape[2]):
        pm = veg["pai"][:, :, l]
        with np.errstate(invalid="ignore"):
            hm[(pm == 0) & (hm > 0)] = 0
            pm[(hm == 0) & (pm > 0)] = 0
    return {k: (v[:, :, 0] if np.ndim(vegp[k]) == 2 else v) for k, v in veg.items()}


def sortl(vegp, sdep):
    """`.sortl` (R/internal.R:2388-2419): pai, hgt, leaft, clump averaged over the layers in force while snow lies
    (weights = number of snow-covered steps each layer serves); single-layer variables pass through"""
    sdep = np.asarray(sdep, dtype=np.float64)
    out = {}
    for k in ("pai", "hgt", "leaft", "clump"):
        a = as3d(vegp[k])
        dmx = a.shape[2]
        if dmx == 1:
            out[k] = a[:, :, 0]
            continue
        s = layer_index(dmx, len(sdep))
        sel = np.nonzero(sdep > 0)[0]
        s = s[sel] if len(sel) else s[:1]
        num, fre = np.unique(s, return_counts=True)
        # the reference sums a[,,j] * fre[j] with j = 1..length(num) — the FIRST layers, not layers `num`
        m = np.zeros(a.shape[:2])
        for j in range(len(num)):
            m = m + a[:, :, j] * fre[j]
        out[k] = m / fre.sum()
    return out


def runsnowmodel(weather: Mapping, micropoint: Mapping, vegp: Mapping, soilc: Mapping, dtm: Mapping, *,
                 snowenv: str = "Taiga", method: str = "fast", snowinitd=0.0, snowinita=0.0, zref: float = 2.0,
                 windhgt: float | None = None, stfact: float = 0.01, device: int = 0, inputs_only: bool = False,
                 one_call: bool = False) -> dict:
    """`runsnowmodel(weather, micropoint, vegp, soilc, dtm, ...)` for data.frame weather (R/Cppwrappers.R:717-735);
    `weather` is always the complete hourly series.  A complete micropoint runs `.snowmodel1` (R/internal.R:2498-2619)
    at the point model's reference height: weather height adjustment, the snow point model (host C++), `.sortl`, the
    5-day chunk loop on the device (terrain refresh from dtm + snow, gridmodelsnow1, `.tpicalc` redistribution,
    hand-over).  A subset micropoint runs, at `zref` / `windhgt`, either that and its subset (`method = "slow"`) or
    `.snowmodelq1` (:2627-2776, `method = "fast"`, the reference's default): the point model over every hour, the grid
    model on the selected days only, the pack carried between them by the point model's balance.
    Returns Tc, Tg, groundsnowdepth, totalSWE, snowden, umu.
    `inputs_only` (complete micropoint): everything up to the chunk loop, not the loop — the `snow` mapping of
    snow.SnowRun / snow.runmicrosnow1 plus `umu`, what `runmicro_snow(..., one_call=True)` takes as `snow_inputs`.
    `one_call` (subset micropoint, `method = "fast"`): the day loop of `.snowmodelq1` as one device-resident call
    (snow.snowmodelq1) instead of the host loop over the selected days (snow.snowmodelq1_days)."""
    from . import snow as S
    if method not in ("fast", "slow"):
        raise ValueError('method is "fast" or "slow"')
    if one_call and (method != "fast" or len(micropoint["subs"]) == micropoint["ntme"]):
        raise ValueError('one_call: the device-resident day loop is the fast method of a subset micropoint (method = "fast", '
                         "subsetpointmodel's output)")
    vegp = cleanvegp(vegp)
    w = {k: np.array(weather[k], dtype=np.float64, copy=True) for k in WEATHER if k in weather}
    tme = weather["obstime"]
    obstime = {k: np.asarray(tme[k]) for k in ("year", "month", "day", "hour")}
    subset = len(micropoint["subs"]) != micropoint["ntme"]
    if subset:
        zref = float(zref)
        windhgt = zref if windhgt is None else float(windhgt)
    else:
        zref = windhgt = float(micropoint["zref"])                     # runsnowmodel passes micropoint$zref twice
    if zref != windhgt:                                                # R/internal.R:2505-2507, 2636-2638
        w["windspeed"] = w["windspeed"] * np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    lat, long = float(micropoint["lat"]), float(micropoint["long"])
    z = np.asarray(dtm["z"], dtype=np.float64)
    hmax = float(np.nanmax(np.asarray(vegp["hgt"], dtype=np.float64)))
    if hmax > zref:                                                    # R/internal.R:2509-2526
        w.update({k: v for k, v in pointmodel.weatherhgtCpp(obstime, w, zref, zref, hmax, lat, long).items() if k in w})
        zref = hmax
    vp = sortvegp_point(vegp)                                          # (hgt, pai, x, clump, leafr, leaft, ...)
    vegpp = np.array([vp[1], vp[0], vp[5], vp[3]])                     # c(vegpp[2], vegpp[1], vegpp[6], vegpp[4])
    sdep = z * 0 + snowinitd
    sage = z * 0 + snowinita
    other_p = [0.0, 0.0, lat, long, zref, float(np.nanmean(sdep)), float(np.nanmean(sage))]
    hour_int = {**obstime, "hour": np.floor(np.asarray(obstime["hour"], dtype=np.float64))}   # `hour = tme$hour`
    fast = subset and method == "fast"
    pmod = pointmodel.pointmodelsnow(hour_int, w, vegpp, other_p, snowenv, maxiter=20 if fast else 100)
    n = len(w["temp"])
    pointm = {"Gp": pmod["G"], "Tc": pmod["Tc"], "RswabsG": pmod["RswabsG"], "RlwabsG": pmod["RlwabsG"], "umu": pmod["umu"],
              "tr": pmod["tr"]}
    vg = sortl(vegp, pmod["sdepc"][:n])
    res = dtm["res"]
    xres = res if np.isscalar(res) else res[0]
    clim = {k: w[k] for k in ("temp", "relhum", "pres", "swdown", "difrad", "lwdown", "windspeed", "winddir", "precip")}
    if fast:
        subs = np.asarray(micropoint["subs"], dtype=np.int64)          # 1-based positions, as in the reference
        ai = subs - 1
        vg["leaft"] = np.where(np.isnan(vg["leaft"]), 0.01, vg["leaft"])
        other = {"zref": zref, "lat": lat, "lon": long, "isnowdc": snowinitd * z, "isnowac": sage, "isnowag": sage}
        days = S.snowmodelq1 if one_call else S.snowmodelq1_days
        out = days(_rows(hour_int, ai), _rows(clim, ai), _rows(pointm, ai), pmod, w["temp"],
                   np.where(w["temp"] > 2, 0.0, w["precip"]), subs, vg, other, snowenv, z, xres, stfact, device=device)
        out["umu"] = pmod["umu"][ai]
        return out
    other = {"zref": zref, "lat": lat, "lon": long, "isnowdc": sdep, "isnowac": sage, "isnowdg": sdep * 0.5, "isnowag": sage}
    if inputs_only:
        if subset:
            raise ValueError("inputs_only: the one-call snow run takes a complete micropoint")
        return {"obstime": hour_int, "climdata": clim, "pointm": pointm, "vegp": vg, "other": other, "snowenv": snowenv, "dtm": z,
                "res": xres, "tfact": stfact, "umu": pmod["umu"]}
    out = S.snowmodel1_chunks(hour_int, clim, pointm, vg, other, snowenv, z, xres, stfact, device=device)
    out["umu"] = pmod["umu"]
    if subset:                                                         # method = "slow": the full model, then its subset
        out = subsetsnowmodel(out, micropoint["subs"])
    return out


def runsnowmodela(climarray: Mapping, obstime: Mapping, micropointa: Sequence, vegp: Mapping, soilc: Mapping, dtm: Mapping, *,
                  dtmc, lats_c, lons_c, lats, lons, altcorrect: int = 0, snowenv: str = "Taiga", method: str = "fast",
                  snowinitd: float = 0.0, snowinita: float = 0.0, zref: float = 2.0, windhgt: float | None = None,
                  stfact: float = 0.01, device: int = 0, point_device: int | None = None, one_call: bool = False,
                  device_loop: bool = False, inputs_only: bool = False) -> dict:
    """`runsnowmodel(climarrayr, micropointa, vegp, soilc, dtm, dtmc, tme, altcorrect, ...)` for array weather
    (R/Cppwrappers.R:735-757 -> `.snowmodel2`, R/internal.R:2777-3013): the snow point model once per cell of
    the climate grid (`point_device=None`: host C++, a cell at a time; an int: every cell as one batch on that device,
    whole days only), then `snow.snowmodel2_chunks`.  `climarray[k]`: [crows, ccols, T]; `dtmc`, `lats_c`, `lons_c`:
    [crows, ccols] of the climate grid; `lats`, `lons`: [rows, cols] of the fine raster.  A subset micropoint list with
    `method = "slow"` runs the whole series and subsets it (here `umu` too along time; the reference indexes the array as
    a vector there); `method = "fast"` runs `.snowmodelq2` (R/internal.R:3017-3283) = `snow.snowmodelq2_days`.  As in the reference every climate cell needs
    data, and vegetation taller than `zref` fails (`.snowmodel2` stops at R/internal.R:2838, `climdfr` not found).
    `one_call` (subset micropoints, `method = "fast"`): the day loop as one device-resident call with the coarse arrays left
    coarse (`snow.snowmodelq2`) instead of the host day loop; the default is unchanged.
    `device_loop` (`method = "slow"`, or micropoints of the complete series): the chunk loop as one device-resident call with
    the coarse arrays left coarse (`snow.snowmodel2_coarse`) instead of `snow.snowmodel2_chunks`; the default is unchanged.
    `inputs_only` (the slow method on micropoints of the complete series): everything up to the chunk loop, not the loop — the
    arguments of `snow.snowmodel2_coarse` by name, what `runmicro_snow_array(..., one_call=True)` takes as `snow_inputs`."""
    from . import snow as S
    if any(m is None for m in micropointa):
        raise ValueError("every coarse cell needs a micropoint")
    last = micropointa[-1]                                            # the reference's loop keeps the last one's subs
    subset = len(last["subs"]) != last["ntme"]
    if method not in ("fast", "slow"):
        raise ValueError('method is "fast" or "slow"')
    fast = subset and method == "fast"
    if one_call and not fast:
        raise ValueError('one_call: the device-resident day loop is the fast method of subset micropoints (method = "fast", '
                         "subsetpointmodel's output for every climate cell)")
    if device_loop and fast:
        raise ValueError('device_loop: the device-resident chunk loop is the slow method (method = "slow", or micropoints of the '
                         "complete series); the fast method's device-resident day loop is one_call=True")
    if inputs_only and subset:
        raise ValueError("inputs_only: the one-call snow run takes micropoints of the complete series")
    vegp = cleanvegp(vegp)
    if subset:
        zref = float(zref)
        windhgt = zref if windhgt is None else float(windhgt)
    else:
        zref = windhgt = float(micropointa[0]["zref"])
    cr, cc, T = np.shape(climarray["temp"])
    z = np.asarray(dtm["z"], dtype=np.float64)
    R, Cc = z.shape
    if float(np.nanmax(np.asarray(vegp["hgt"], dtype=np.float64))) > zref:
        raise ValueError("the array snow model needs zref at or above the tallest vegetation (the reference fails there)")
    wdir = np.array([getmode(np.asarray(climarray["winddir"])[:, :, k]) for k in range(T)])
    vc = {k: block_reduce(vegp[k], cr, cc) for k in ("pai", "hgt", "leaft", "clump")}
    if np.isnan(np.asarray(climarray["temp"])[:, :, 0]).any() or np.isnan(vc["hgt"][:, :, 0]).any():
        raise ValueError("every coarse cell needs climate data and vegetation")
    ob = {k: np.asarray(obstime[k]) for k in ("year", "month", "day", "hour")}
    clim_c = {k: np.array(climarray[k], dtype=np.float64, order="F", copy=True) for k in WEATHER if k != "winddir"}
    if zref != windhgt:
        clim_c["windspeed"] *= np.log(67.8 * zref - 5.42) / np.log(67.8 * windhgt - 5.42)
    clim_c["winddir"] = wdir
    pointm_c = snow_pointm_cells(ob, clim_c, vc, lats_c, lons_c, zref, snowinitd, snowinita, snowenv, fast, point_device)
    res = dtm["res"]
    xres = res if np.isscalar(res) else res[0]
    rowpos, colpos = api.coarse_positions(R, cr), api.coarse_positions(Cc, cc)
    if fast:                                                          # R/internal.R:3017-3283
        subs = np.asarray(last["subs"], dtype=np.int64)
        ai = subs - 1
        pm2_c = {k: pointm_c[k] for k in ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng")}
        pm2_c["tc"] = clim_c["temp"]
        pm2_c["snow"] = np.where(clim_c["temp"] > 2, 0.0, clim_c["precip"])
        sel = lambda d: {k: (np.asarray(v)[ai] if np.ndim(v) == 1 else np.asfortranarray(np.asarray(v)[:, :, ai]))   # noqa: E731
                         for k, v in d.items()}
        pm_s = sel({k: pointm_c[k] for k in ("Gp", "Tc", "RswabsG", "RlwabsG", "umu", "tr", "sdepc")})
        vg = sortl(vegp, np.max(pm_s["sdepc"], axis=(0, 1)))
        other = {"zref": zref, "lats": np.asarray(lats, dtype=np.float64), "lons": np.asarray(lons, dtype=np.float64),
                 "isnowdc": z * 0 + snowinitd, "isnowac": z * 0 + snowinita, "isnowag": z * 0 + snowinita}
        days = S.snowmodelq2 if one_call else S.snowmodelq2_days
        return days(sel(ob), sel(clim_c), pm_s, pm2_c, subs, vg, other, snowenv, z, np.asarray(dtmc, dtype=np.float64),
                    xres, stfact, rowpos=rowpos, colpos=colpos, altcorrect=altcorrect, device=device)
    vg = sortl(vegp, np.max(pointm_c["sdepc"], axis=(0, 1)))
    sdep = z * 0 + snowinitd
    sage = z * 0 + snowinita
    other = {"zref": zref, "lats": np.asarray(lats, dtype=np.float64), "lons": np.asarray(lons, dtype=np.float64),
             "isnowdc": sdep, "isnowac": sage, "isnowdg": sdep * 0.5, "isnowag": sage}
    agg = 10 if xres <= 100 and min(cr, cc) >= 10 else 1
    if inputs_only:
        return {"obstime": ob, "clim_c": clim_c, "pointm_c": pointm_c, "vegp": vg, "other": other, "snowenv": snowenv, "dtm": z,
                "dtmc": np.asarray(dtmc, dtype=np.float64), "res": xres, "tfact": stfact, "rowpos": rowpos, "colpos": colpos,
                "altcorrect": int(altcorrect), "agg": agg}
    loop = S.snowmodel2_coarse if device_loop else S.snowmodel2_chunks
    out = loop(ob, clim_c, pointm_c, vg, other, snowenv, z, np.asarray(dtmc, dtype=np.float64), xres, stfact,
               rowpos=rowpos, colpos=colpos, altcorrect=altcorrect,
               agg=agg, device=device)
    if subset:
        i = np.asarray(last["subs"], dtype=np.int64) - 1
        out = {k: v[:, :, i] for k, v in out.items()}
    return out


def snow_pointm_cells(ob: Mapping, clim_c: Mapping, vc: Mapping, lats_c, lons_c, zref: float, snowinitd: float,
                      snowinita: float, snowenv: str, fast: bool, point_device: int | None = None) -> dict:
    """The point stage of `.snowmodel2` / `.snowmodelq2`: pointmodelsnow (maxiter = 10) for every cell of the climate grid
    -> `pointm_c`, [crows, ccols, T] each.  `point_device=None`: the host entry, one cell at a time; an int: all cells as one
    batch on that device (pointmodel.pointmodelsnow_batch).  `fast` adds the melt terms and takes the depth AFTER the step."""
    cr, cc, T = np.shape(clim_c["temp"])
    pn = {"Gp": "G", "Tc": "Tc", "RswabsG": "RswabsG", "RlwabsG": "RlwabsG", "umu": "umu", "tr": "tr", "sdepc": "sdepc"}
    if fast:                                                          # `.snowmodelq2`: depth after the step, the melt terms
        pn.update({k: k for k in ("sublmelt", "tempmelt", "rainmelt", "sstemp", "sdenc", "sdeng")})
    pointm_c = {k: np.empty((cr, cc, T), order="F") for k in pn}
    cells = [(i, j) for i in range(cr) for j in range(cc)]
    vegpp = [[float(np.mean(vc[k][i, j, :])) for k in ("pai", "hgt", "leaft", "clump")] for i, j in cells]           # `.tovp`
    other = [[0.0, 0.0, float(lats_c[i, j]), float(lons_c[i, j]), zref, snowinitd, snowinita] for i, j in cells]
    cols = [k for k in clim_c if k != "winddir"]
    if point_device is None:
        pmods = [pointmodel.pointmodelsnow(ob, {**{k: clim_c[k][i, j, :] for k in cols}, "winddir": clim_c["winddir"]}, vegpp[p],
                                           other[p], snowenv, maxiter=10) for p, (i, j) in enumerate(cells)]
        take = lambda v, p: pmods[p][v]                                                  # noqa: E731
    else:
        batch = pointmodel.pointmodelsnow_batch(ob, {k: np.reshape(clim_c[k], (cr * cc, T)) for k in cols}, vegpp, other,
                                                snowenv, maxiter=10, device=int(point_device))
        take = lambda v, p: batch[v][p]                                                  # noqa: E731
    for p, (i, j) in enumerate(cells):
        for k, v in pn.items():
            pointm_c[k][i, j, :] = take(v, p)[1:T + 1] if fast and k == "sdepc" else take(v, p)[:T]
    return pointm_c


# ---- snow: runmicro(snow = TRUE) -> .runmicrosnow1 ----------------------------------------------------------------
def _rows(d: Mapping, ai):
    return {k: np.asarray(v)[ai] for k, v in d.items()}


def subsetpointmodel(micropoint: Mapping, tstep: str = "month", what: str = "tmax", days=None, Tc=None) -> dict:
    """`subsetpointmodel` (R/dataprep.R:31-103): whole days of the point model — given 1-based `days`, or one day per
    month / year chosen by the point model's canopy temperature (`what` = tmax, tmin, tmedian)."""
    dfo, ob = micropoint["dfo"], micropoint["obstime"]
    if days is not None:
        days = np.asarray(days, dtype=np.int64)
        ai = (np.repeat((days - 1) * 24, 24) + np.tile(np.arange(24), days.size)).astype(np.int64)
    else:
        tc = np.asarray(dfo["Tc"] if Tc is None else Tc, dtype=np.float64)
        yr, mo, dy = (np.asarray(ob[k]).astype(int) for k in ("year", "month", "day"))

        def extract(sel):
            v = tc[sel]
            if what == "tmax":
                s2 = int(np.argmax(v))
            elif what == "tmin":
                s2 = int(np.argmin(v))
            elif what == "tmedian":
                o = np.argsort(v, kind="stable")
                s2 = int(o[len(o) // 2 - 1])                       # o[trunc(length(o) / 2)], 1-based
            else:
                raise ValueError("what must be one of tmax, tmin or tmedian")
            k = sel[s2]
            return np.nonzero((yr == yr[k]) & (mo == mo[k]) & (dy == dy[k]))[0]
        parts = []
        for y in dict.fromkeys(yr.tolist()):
            sely = np.nonzero(yr == y)[0]
            if tstep == "year":
                parts.append(extract(sely))
            elif tstep == "month":
                # `which(tme$mon[sely] == m)` indexes WITHIN the year's rows; the reference then uses those positions
                # on the whole series — the same thing for the first year only
                for m in dict.fromkeys(mo[sely].tolist()):
                    parts.append(extract(np.nonzero(mo[sely] == m)[0]))
            else:
                raise ValueError("tstep must be month or year")
        ai = np.concatenate(parts)
    out = dict(micropoint)
    out["dfo"] = _rows(dfo, ai)
    out["weather"] = _rows(micropoint["weather"], ai)
    out["obstime"] = _rows(ob, ai)
    out["subs"] = np.asarray(micropoint["subs"])[ai]
    if micropoint.get("Tbz") is not None:
        out["Tbz"] = np.asarray(micropoint["Tbz"])[ai]
    return out


def subsetpointmodela(micropointa: Sequence, tstep: str = "month", what: str = "tmax", days=None) -> list:
    """`subsetpointmodela` (R/dataprep.R:105-138): the same days for every cell of the climate grid — chosen, as there,
    from the mean canopy temperature over the cells that have a point model"""
    have = [m for m in micropointa if m is not None]
    if days is None:
        tc = np.mean([np.asarray(m["dfo"]["Tc"], dtype=np.float64) for m in have], axis=0)
        return [None if m is None else subsetpointmodel(m, tstep, what, Tc=tc) for m in micropointa]
    return [None if m is None else subsetpointmodel(m, days=days) for m in micropointa]


def subsetsnowmodel(smod: Mapping, subs) -> dict:
    """`subsetsnowmodel` (R/dataprep.R:148-160); `subs` 1-based.  (The reference tests `snowmods$umu`, which does not
    exist yet, so `umu` is always subset as a vector.)"""
    i = np.asarray(subs, dtype=np.int64) - 1
    out = {k: np.asarray(smod[k])[:, :, i] for k in ("Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden")}
    out["umu"] = np.asarray(smod["umu"])[i]
    return out


def sortl2(vegp, sdep, reqhgt, pai_a=None):
    """`.sortl2` (R/internal.R:2421-2482): as `.sortl` for pai, hgt, leaft, clump, leafd, plus paia and leafden"""
    sdep = np.asarray(sdep, dtype=np.float64)
    out = {}
    for k in ("pai", "hgt", "leaft", "clump", "leafd"):
        a = as3d(vegp[k])
        dmx = a.shape[2]
        if dmx == 1:
            out[k] = a[:, :, 0]
            continue
        s = layer_index(dmx, len(sdep))
        sel = np.nonzero(sdep > 0)[0]
        s = s[sel] if len(sel) else s[:1]
        num, fre = np.unique(s, return_counts=True)
        m = np.zeros(a.shape[:2])
        for j in range(len(num)):
            m = m + a[:, :, j] * fre[j]
        out[k] = m / fre.sum()
    if pai_a is not None and as3d(pai_a).shape[2] > 1:
        pai_a = sortl({"pai": pai_a, "hgt": pai_a, "leaft": pai_a, "clump": pai_a}, sdep)["pai"]
    elif pai_a is not None:
        pai_a = as3d(pai_a)[:, :, 0]
    out["leafden"], out["paia"] = foliageden(reqhgt, out["hgt"], out["pai"], pai_a)
    return out


def _stack_micropoints(mps: Sequence, crows: int, ccols: int, get) -> np.ndarray:
    """get(micropoint) -> [T] of every coarse cell (the micropoints run along the rows of the climate grid) as [crows, ccols, T]"""
    a = np.empty((crows, ccols, len(mps[0]["weather"]["temp"])), order="F")
    for k, m in enumerate(mps):
        a[k // ccols, k % ccols, :] = get(m)
    return a


def _snow_day_other(z, dtm: Mapping, zref, lat, lon, soil: Mapping, device: int, _terrain) -> dict:
    """gridmicrosnow's `other`: the bare-ground terrain of the dtm (`_terrain`: the tests' stand-in), the site(s), Smax"""
    res = dtm["res"]
    xres = res if np.isscalar(res) else res[0]
    ter = terrain.precompute_terrain(z, xres, zref, device=device) if _terrain is None else _terrain(z, xres, zref)
    return {"slope": ter["slope"], "aspect": ter["aspect"], "hor": ter["hor"], "skyview": ter["svfa"], "wsa": ter["wsa"],
            "lat": lat, "lon": lon, "zref": float(zref), "Smax": soilinit(soil)["Smax"]}


def _snow_day_template(moutn: Mapping, snowdays, nosnowdays, rows: int, cols: int) -> dict:
    """the snow days' outputs as gridmicrosnow receives them: the solver's values on the days of both classes, NaN elsewhere"""
    t1 = len(snowdays) * 24
    s1 = np.arange(t1)[np.repeat(np.isin(snowdays, nosnowdays), 24)]
    s2 = np.arange(len(nosnowdays) * 24)[np.repeat(np.isin(nosnowdays, snowdays), 24)]
    micro = {}
    for k, v in moutn.items():
        a = np.full((rows, cols, t1), np.nan, order="F")
        if len(s1):
            a[:, :, s1] = np.asarray(v)[:, :, s2]
        micro[k] = a
    return micro


def _snow_day_outm(out: Sequence, reqhgt: float) -> list:
    """which of the ten outputs gridmicrosnow writes: the caller's selection above ground, a fixed set at and below it"""
    if reqhgt == 0:
        return [1 if i in (0, 3, 5, 6, 7, 8, 9) else 0 for i in range(10)]
    if reqhgt < 0:
        return [1 if i in (0, 3) else 0 for i in range(10)]
    return [int(bool(v)) for v in out]


def _snow_host_route(smod: Mapping, z, reqhgt: float, pai_a, tfact: float, out: Sequence, device: int, solve_days, snow_days) -> dict:
    """What `.runmicrosnow1` and `.runmicrosnow2` share (R/internal.R:3581-3659, 3661-3742): the day classes from the snow
    model's totalSWE (NA -> 0, masked by the dtm `z`), the no-snow days through `solve_days(days, **runmicro's keywords)` (none:
    `.createblanktemplate`, day 1 solved and blanked), the snow days through `snow_days(smod, snowdays, their hour indices, the
    template gridmicrosnow writes over, its output selection)`, and the two merged by day"""
    from . import snow as S
    sm = dict(smod)
    swe = np.array(sm["totalSWE"], dtype=np.float64, copy=True)
    swe[np.isnan(swe)] = 0.0
    swe[np.isnan(z)] = np.nan                                            # mask(totalSWE, dtm)
    sm["totalSWE"] = swe
    sd = S.snowdaysfun(S.applycpp3(swe, "max", device=device), S.applycpp3(swe, "min", device=device))
    alldays = np.arange(1, len(sd["snowdays"]) + 1)
    snowdays, nosnowdays = alldays[sd["snowdays"] == 1], alldays[sd["nosnowdays"] == 1]
    rows, cols = z.shape
    if len(nosnowdays):
        moutn = solve_days(nosnowdays, pai_a=pai_a, tfact=tfact, out=out)
    else:
        moutn = {k: v * np.nan for k, v in solve_days([1], tfact=1.5, out=out).items()}
    if not len(snowdays):
        return moutn
    ai = (np.repeat((snowdays - 1) * 24, 24) + np.tile(np.arange(24), snowdays.size)).astype(np.int64)
    micro = _snow_day_template(moutn, snowdays, nosnowdays, rows, cols)
    mouts = snow_days(sm, snowdays, ai, micro, _snow_day_outm(out, reqhgt))
    return S.merge_snow_outputs(moutn, mouts, snowdays, nosnowdays, rows, cols)


def runmicro_snow(micropoint: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, smod: Mapping | None, *,
                  pai_a=None, tfact: float = 1.5, out: Sequence = (1,) * 10, device: int = 0,
                  _solve=None, _microsnow=None, _terrain=None, one_call: bool = False, snow_inputs: Mapping | None = None) -> dict:
    """`runmicro(..., snow = TRUE, snowmod = smod)` for data.frame weather = `.runmicrosnow1` (R/internal.R:3581-3659):
    days with no snow anywhere go through the ordinary solver, days with snow through gridmicrosnow1 (which keeps the
    ordinary solver's values on snow-free cell-steps of days that have both), and the two are merged by day.
    `_solve` / `_microsnow` / `_terrain` let the tests put their checkers behind the same orchestration.
    `one_call` (default False: the host orchestration below, the comparison leg): the device-resident run instead
    (snow.SnowRun, include/mcf.h mcf_snowrun_*) for reqhgt >= 0 and, through its below-ground entries, reqhgt < 0 alike — the
    snow model's chunk loop runs inside it, so it takes `snow_inputs` = runsnowmodel(..., inputs_only=True) in place of `smod`
    (a complete micropoint)."""
    from . import snow as S
    if one_call:
        return _runmicro_snow_one_call(micropoint, reqhgt, vegp, soilc, dtm, snow_inputs, pai_a, tfact, out, device, _terrain)
    solve = runmicro if _solve is None else _solve
    microsnow = S.gridmicrosnow1 if _microsnow is None else _microsnow
    veg, soil, z = cleanvars(vegp, soilc, dtm["z"])

    def solve_days(days, **kw):
        return solve(subsetpointmodel(micropoint, days=days), reqhgt, vegp, soilc, dtm, device=device, **kw)

    def snow_days(sm, snowdays, ai, micro, outm):
        mps = subsetpointmodel(micropoint, days=snowdays)
        w = dict(mps["weather"])
        w["umu"] = np.asarray(sm["umu"])[ai]
        sdept = np.zeros(micropoint["ntme"])
        sdept[np.asarray(mps["subs"]) - 1] = 1
        vg = sortl2(veg, sdept, reqhgt, pai_a)
        other = _snow_day_other(z, dtm, micropoint["zref"], float(micropoint["lat"]), float(micropoint["long"]), soil, device, _terrain)
        return microsnow(reqhgt, mps["obstime"], w, subsetsnowmodel(sm, ai + 1), micro, vg, other, float(micropoint["matemp"]), outm)
    return _snow_host_route(smod, z, reqhgt, pai_a, tfact, out, device, solve_days, snow_days)


def _runmicro_snow_one_call(micropoint, reqhgt, vegp, soilc, dtm, snow_inputs, pai_a, tfact, out, device, _terrain):
    """runmicro_snow's `one_call` route: the staged snow run — pass 1 gives the day classes that `.sortl2` weights the
    vegetation layers with, pass 2 takes gridmicrosnow1's inputs for the WHOLE series"""
    from . import snow as S
    if snow_inputs is None:
        raise ValueError("one_call: snow_inputs = runsnowmodel(weather, micropoint, vegp, soilc, dtm, inputs_only=True) is needed")
    if len(micropoint["subs"]) != micropoint["ntme"]:
        raise ValueError("one_call: the one-call snow run takes a complete micropoint")
    a = prepare_grid_inputs(micropoint, reqhgt, vegp, soilc, dtm, pai_a=pai_a, out=out, device=device)
    a["tfact"] = float(tfact)
    veg, soil, z = cleanvars(vegp, soilc, dtm["z"])
    snow = {k: v for k, v in snow_inputs.items() if k != "umu"}
    # `complete` matters below ground only (Tbelowgroundv): the reference solves the no-snow SUBSET, an incomplete series unless
    # every day is a no-snow day (prepare_grid_inputs: complete = len(subs) == ntme) — known after pass 1
    for complete in ((False, True) if reqhgt < 0 else (a["complete"],)):
        a["complete"] = complete
        with S.SnowRun(a, snow, device=device, below=reqhgt < 0) as run:
            sd, nd = run.pass1()
            if reqhgt < 0 and not complete and nd.all():
                continue
            return run.pass2(_one_call_micro(micropoint, reqhgt, veg, soil, z, dtm, snow_inputs, sd, pai_a, device, _terrain),
                             float(micropoint["matemp"]))


def _one_call_micro(micropoint, reqhgt, veg, soil, z, dtm, snow_inputs, sd, pai_a, device, _terrain):
    """gridmicrosnow1's inputs for the WHOLE series once pass 1 has given the snow days `sd` (one flag per day): `.sortl2`
    vegetation weighted by them, bare-ground terrain, Smax, the weather with the snow model's umu; None for a year without a
    snow day"""
    snowdays = np.flatnonzero(sd) + 1
    if not snowdays.size:
        return None
    sdept = np.zeros(micropoint["ntme"])
    sdept[np.asarray(subsetpointmodel(micropoint, days=snowdays)["subs"]) - 1] = 1
    vg = sortl2(veg, sdept, reqhgt, pai_a)
    other = _snow_day_other(z, dtm, micropoint["zref"], float(micropoint["lat"]), float(micropoint["long"]), soil, device, _terrain)
    w = dict(micropoint["weather"])
    w["umu"] = np.asarray(snow_inputs["umu"])
    return {"obstime": micropoint["obstime"], "climdata": w, "vegp": vg, "other": other}


def _names(sel, every, what):
    names = (sel,) if isinstance(sel, str) else tuple(sel)
    if any(n not in every for n in names) or len(set(names)) != len(names):
        raise ValueError(f"{what}: distinct names of {tuple(every)}")
    return names


def _pack_table(tab, tsteps: int, chunk_steps: int):
    """the summary table for the snow model's series: the days past the last whole chunk belong to no chunk (NA in the series)"""
    tab = np.array(tab, dtype=np.int32, copy=True)
    tab[max(1, tsteps // chunk_steps) * (chunk_steps // 24):] = -1
    return tab


def _snow_sink_inputs(micropoint, reqhgt, vegp, soilc, dtm, snow_inputs, vars, snow_vars, pai_a, tfact, device, what):
    """What the snow run's sink-only calls share ahead of the run; `what`: the refusal of reqhgt < 0.  -> a namespace with `a`
    (the solver's inputs), `kept` (the selected outputs that exist at this reqhgt), `snames` (the selected snow series), `snow`
    (the snow model's inputs) and what pass 2's microclimate is made from"""
    if reqhgt < 0:
        raise ValueError(what)
    names = _names(vars, api._abi.OUT_NAMES, "vars")
    snames = _names(snow_vars, api._abi.SNOWDRIVER_OUT, "snow_vars")
    if not names and not snames:
        raise ValueError("nothing selected: vars and snow_vars are both empty")
    if snow_inputs is None:
        raise ValueError("snow_inputs = runsnowmodel(weather, micropoint, vegp, soilc, dtm, inputs_only=True) is needed")
    if len(micropoint["subs"]) != micropoint["ntme"]:
        raise ValueError("the one-call snow run takes a complete micropoint")
    out = _out_mask(names)[1]
    a = prepare_grid_inputs(micropoint, reqhgt, vegp, soilc, dtm, pai_a=pai_a, out=out, device=device)
    a["tfact"] = float(tfact)
    kept = [n for n, o in zip(api._abi.OUT_NAMES, a["out"]) if o]      # (reqhgt == 0: tleaf, relhum and windspeed are masked)
    if names and not kept:
        raise ValueError("none of the selected variables exists at this reqhgt")
    if not kept:                                                       # (the snowpack's sink alone: the run still needs an output)
        a["out"] = [1] + [0] * 9
    return SimpleNamespace(a=a, kept=kept, snames=snames, snow={k: v for k, v in snow_inputs.items() if k != "umu"},
                           micro=(micropoint, reqhgt, *cleanvars(vegp, soilc, dtm["z"]), dtm, snow_inputs), pai_a=pai_a, device=device)


def _snow_sink_run(i, devices, n_blocks, _terrain, enable, fetch) -> dict:
    """The run of _snow_sink_inputs' `i` with a sink as its only output: enable(run), pass 1, pass 2 when an output of the solver
    is selected, fetch(run) -> its result with the day classes"""
    from . import snow as S
    with S.SnowRun(i.a, i.snow, device=i.device, devices=devices, n_blocks=n_blocks) as run:
        enable(run)
        sd, nd = run.pass1()
        if i.kept:
            run.pass2(_one_call_micro(*i.micro, sd, i.pai_a, i.device, _terrain), float(i.micro[0]["matemp"]), want_arrays=False)
        res = fetch(run)
    res.update(snowdays=sd, nosnowdays=nd)
    return res


def runmicro_snow_summary(micropoint: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, snow_inputs: Mapping, *,
                          periods="month", vars: Sequence = ("Tz",), stats: Sequence = ("mean", "min", "max"), thresholds=None,
                          snow_vars: Sequence = (), snow_stats: Sequence = ("mean", "max", "hours_above"), snow_thresholds=None,
                          pai_a=None, tfact: float = 1.5, device: int = 0, devices=None, n_blocks: int = 0, _terrain=None) -> dict:
    """`runmicro(..., snow = TRUE)` reduced over time on the device: runmicro_snow(..., one_call=True) with the period summaries
    of include/mcf.h as its only sink — per-cell statistics `stats` of the merged outputs `vars` and, with `snow_vars` (names
    of Tc, Tg, groundsnowdepth, totalSWE, snowden), `snow_stats` of the snow model's series, over `periods` (summary_periods).
    No [rows, cols, steps] array is made on either side.  Days that are neither snow nor no-snow days are never counted (they
    are NA in runmicro_snow's arrays); the snow series' days past the last whole 5-day chunk neither.  `snow_thresholds`
    defaults to 0 (hours_above of totalSWE: the snow-cover duration).  reqhgt == 0 masks the variables as runmicro does;
    reqhgt < 0 is not available.  `devices` / `n_blocks`: row blocks over several devices.
    -> {variable: {statistic: [rows, cols, nperiods]}, "snow": {series: {statistic: ...}, "days"}, "periods": labels, "days":
    counted days per period, "snowdays", "nosnowdays": one flag per day}"""
    i = _snow_sink_inputs(micropoint, reqhgt, vegp, soilc, dtm, snow_inputs, vars, snow_vars, pai_a, tfact, device,
                          "period summaries of the snow run need reqhgt >= 0")
    tab, labels = summary_periods(i.a["obstime"], periods)
    summary = dict(periods=tab, nperiods=len(labels), vars=i.kept, stats=stats, thresholds=thresholds) if i.kept else None
    pack = None
    if i.snames:
        pack = dict(periods=_pack_table(tab, len(i.a["obstime"]["year"]), int(i.snow.get("chunk_steps", 120))), nperiods=len(labels),
                    vars=i.snames, stats=snow_stats, thresholds=0.0 if snow_thresholds is None else snow_thresholds)
    res = _snow_sink_run(i, devices, n_blocks, _terrain, lambda run: run.summary_enable(summary, pack), lambda run: run.fetch_summary())
    res.setdefault("days", None)
    res["periods"] = labels
    return res


def runmicro_snow_series(micropoint: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, snow_inputs: Mapping, *,
                         points=None, xy=None, zones=None, vars: Sequence = ("Tz",), stats: Sequence = ("mean", "min", "max"),
                         snow_vars: Sequence = (), pai_a=None, tfact: float = 1.5, device: int = 0, devices=None, n_blocks: int = 0,
                         _terrain=None) -> dict:
    """`runmicro(..., snow = TRUE)` reduced over space on the device: the snow run with the series sink of include/mcf.h as
    its only sink — the hourly series of the merged outputs `vars` and, with `snow_vars` (names of Tc, Tg, groundsnowdepth,
    totalSWE, snowden), of the snow model's series at logger sites (`points`, `xy`: see series_cells), and their per-step
    statistics `stats` over `zones` ("mean Tz under snow in the heath class, hour by hour").  Days that are neither snow nor
    no-snow days, and the snow series' days past the last whole 5-day chunk, are NA.  reqhgt < 0 is not available.
    -> {variable: {"points": [tsteps, npoints], "zones": {statistic: [tsteps, nzones]}}, "snow": {series: {...}}, "cells",
    "snowdays", "nosnowdays"}"""
    i = _snow_sink_inputs(micropoint, reqhgt, vegp, soilc, dtm, snow_inputs, vars, snow_vars, pai_a, tfact, device,
                          "the series sink of the snow run needs reqhgt >= 0")
    rows, cols = np.asarray(dtm["z"]).shape[:2]
    cells = series_cells(dtm, rows, cols, points, xy)
    sel = dict(points=cells if cells.size else None, zones=zones, stats=stats)
    res = _snow_sink_run(i, devices, n_blocks, _terrain, lambda run: run.series_enable(dict(sel, vars=i.kept) if i.kept else None,
                                                                                     dict(sel, vars=i.snames) if i.snames else None),
                         lambda run: run.fetch_series())
    res["cells"] = cells
    return res


def runsnowmodel_series(weather: Mapping, micropoint: Mapping, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, points=None, xy=None,
                        zones=None, vars: Sequence = ("totalSWE",), stats: Sequence = ("mean", "min", "max"), snowenv: str = "Taiga",
                        snowinitd=0.0, snowinita=0.0, stfact: float = 0.01, devices=None, n_blocks: int = 0) -> dict:
    """`runsnowmodel()` (the slow method, data.frame weather, a complete micropoint) reduced over space on the device: the snow
    model's series `vars` at logger sites and their per-step statistics over `zones` instead of the five [rows, cols, steps]
    arrays.  The days past the last whole 5-day chunk (NA in runsnowmodel's arrays) are NA.
    -> {"points": {series: [tsteps, npoints]}, "zones": {series: {statistic: [tsteps, nzones]}}, "cells"}"""
    from . import snow as S
    names = _names(vars, api._abi.SNOWDRIVER_OUT, "vars")
    if not names:
        raise ValueError("vars: nothing selected")
    si = runsnowmodel(weather, micropoint, vegp, soilc, dtm, snowenv=snowenv, method="slow", snowinitd=snowinitd, snowinita=snowinita,
                      stfact=stfact, inputs_only=True)
    rows, cols = np.asarray(dtm["z"]).shape[:2]
    cells = series_cells(dtm, rows, cols, points, xy)
    res = S.snowmodel1_series(si["obstime"], si["climdata"], si["pointm"], si["vegp"], si["other"], si["snowenv"], si["dtm"], si["res"],
                              si["tfact"], points=cells if cells.size else None, zones=zones, vars=names, stats=stats, devices=devices,
                              n_blocks=n_blocks)
    res["cells"] = cells
    return res


def runmicro_snow_nc(micropoint: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, snow_inputs: Mapping,
                     fileout=None, *, snow_fileout=None, vars=None, snow_vars=None, format: str = "classic", deflate_level: int = 0,
                     pai_a=None, tfact: float = 1.5, device: int = 0, devices=None, n_blocks: int = 0, _terrain=None) -> dict:
    """`runmicro(..., snow = TRUE)` followed by `writetonc()` without the arrays in between: the snow run with the netCDF sink of
    include/mcf.h as its only sink — `fileout` the merged outputs `vars` (writetonc's default for the height) as a `writetonc`
    file, `snow_fileout` the snow model's series `snow_vars` (default all five) in the snowpack's file; either may be None.
    Every merged ring chunk is packed on the device and written as int32; no [rows, cols, steps] array is made on either side.
    Days that are neither snow nor no-snow days, the steps past the last whole day and the snow series' days past the last
    whole 5-day chunk are missval.  `dtm` needs "xmin", "ymax" besides "z" / "res" for the files' coordinates.  reqhgt < 0 is
    not available here (snow.runmicrosnow_nc runs it).  `devices` / `n_blocks`: row blocks, each writing its strips (classic
    container).  -> {"vars": the outputs' file's variables, "snow_vars": the snowpack's, "snowdays", "nosnowdays"}; the classic
    file is byte for byte ncsink.writetonc(runmicro_snow(..., one_call=True))."""
    if fileout is None and snow_fileout is None:
        raise ValueError("fileout and snow_fileout are both None")
    names = tuple(ncsink.default_vars(reqhgt) if vars is None else vars) if fileout is not None else ()
    snames = tuple(api._abi.SNOWDRIVER_OUT if snow_vars is None else snow_vars) if snow_fileout is not None else ()
    i = _snow_sink_inputs(micropoint, reqhgt, vegp, soilc, dtm, snow_inputs, names, snames, pai_a, tfact, device,
                          "the front end's file sink of the snow run needs reqhgt >= 0 (snow.runmicrosnow_nc runs below ground)")
    if fileout is not None and tuple(i.kept) != tuple(n for n in api._abi.OUT_NAMES if n in names):
        raise ValueError("a selected variable does not exist at this reqhgt")
    rows, cols = np.asarray(dtm["z"]).shape[:2]
    hours, east, north, crs = ncsink.grid_of(nc_extent(dtm, rows, cols), i.a["obstime"])
    kw = dict(crs_wkt=crs, format=format, deflate_level=deflate_level)
    w = ncsink.NcWriter(fileout, rows, cols, hours, east, north, reqhgt, i.kept, **kw) if fileout is not None else None
    pw = ncsink.SnowpackNcWriter(snow_fileout, rows, cols, hours, east, north, vars=i.snames, **kw) if snow_fileout is not None else None
    try:
        res = _snow_sink_run(i, devices, n_blocks, _terrain, lambda run: run.nc_enable(w, pw), lambda run: {})
    finally:
        for f in (w, pw):
            if f is not None:
                f.close()
    res.update(vars=tuple(i.kept) if w is not None else (), snow_vars=tuple(i.snames))
    return res


def runsnowmodel_nc(weather: Mapping, micropoint: Mapping, vegp: Mapping, soilc: Mapping, dtm: Mapping, fileout, *, vars=None,
                    format: str = "classic", deflate_level: int = 0, snowenv: str = "Taiga", snowinitd=0.0, snowinita=0.0,
                    stfact: float = 0.01, devices=None, n_blocks: int = 0) -> tuple:
    """`runsnowmodel()` (the slow method, data.frame weather, a complete micropoint) into the snowpack's netCDF file (include/mcf.h
    mcf_snowmodel1_nc; the convention: ncsink.SNOWPACK_SCALE / _UNITS / _LONG_NAME) instead of the five [rows, cols, steps]
    arrays: every chunk packed on the device, SWE maps straight to disk.  The days past the last whole 5-day chunk (NA in
    runsnowmodel's arrays) are missval.  `dtm` needs "xmin", "ymax".  -> the file's series names"""
    from . import snow as S
    si = runsnowmodel(weather, micropoint, vegp, soilc, dtm, snowenv=snowenv, method="slow", snowinitd=snowinitd, snowinita=snowinita,
                      stfact=stfact, inputs_only=True)
    rows, cols = np.asarray(dtm["z"]).shape[:2]
    return S.snowmodel1_nc(si["obstime"], si["climdata"], si["pointm"], si["vegp"], si["other"], si["snowenv"], si["dtm"], si["res"],
                           si["tfact"], fileout=fileout, grid=nc_extent(dtm, rows, cols), vars=vars, format=format,
                           deflate_level=deflate_level, devices=devices, n_blocks=n_blocks)


def runsnowmodel_summary(weather: Mapping, micropoint: Mapping, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, periods="month",
                         vars: Sequence = ("totalSWE",), stats: Sequence = ("mean", "max", "hours_above"), thresholds=None,
                         snowenv: str = "Taiga", snowinitd=0.0, snowinita=0.0, stfact: float = 0.01, devices=None, n_blocks: int = 0) -> dict:
    """`runsnowmodel()` (the slow method, data.frame weather, a complete micropoint) reduced over time on the device: per-cell
    statistics of the snow model's series `vars` over `periods` (summary_periods) instead of the five [rows, cols, steps]
    arrays.  hours_above of totalSWE with the default threshold 0 is the snow-cover duration, max of totalSWE the peak snow
    water equivalent.  The days past the last whole 5-day chunk (NA in runsnowmodel's arrays) are not counted.
    -> {series: {statistic: [rows, cols, nperiods]}, "periods": labels, "days": counted days per period}"""
    from . import snow as S
    names = _names(vars, api._abi.SNOWDRIVER_OUT, "vars")
    if not names:
        raise ValueError("vars: nothing selected")
    si = runsnowmodel(weather, micropoint, vegp, soilc, dtm, snowenv=snowenv, method="slow", snowinitd=snowinitd, snowinita=snowinita,
                      stfact=stfact, inputs_only=True)
    tab, labels = summary_periods(si["obstime"], periods)
    res = S.snowmodel1_summary(si["obstime"], si["climdata"], si["pointm"], si["vegp"], si["other"], si["snowenv"], si["dtm"], si["res"],
                               si["tfact"], periods=_pack_table(tab, len(si["obstime"]["year"]), 120), nperiods=len(labels), vars=names,
                               stats=stats, thresholds=0.0 if thresholds is None else thresholds, devices=devices, n_blocks=n_blocks)
    res["periods"] = labels
    return res



def runmicro_snow_array(micropointa: Sequence, crows: int, ccols: int, reqhgt: float, vegp: Mapping, soilc: Mapping,
                        dtm: Mapping, smod: Mapping | None = None, *, dtmc, lats, lons, altcorrect: int = 0, pai_a=None,
                        tfact: float = 1.5, out: Sequence = (1,) * 10, device: int = 0, one_call: bool = False, snow_inputs=None,
                        want_smod: bool = False, _solve=None, _microsnow=None, _terrain=None) -> dict:
    """`runmicro(..., snow = TRUE, snowmod = smod)` for array weather = `.runmicrosnow2` with `.prepsnowinputs2`
    (R/internal.R:3661-3742, 3445-3579): as `runmicro_snow`, with the no-snow days through the coarse-array solver and
    the snow days through gridmicrosnow2 on climate resampled to the fine raster (host numpy, as the reference does it in
    R; relative humidity from resampled vapour pressure, kept within 20 .. 100 %).  Reference behaviour kept: `.sortl2`
    sees no snow-covered step here (`micropoints$subs` of a list is NULL), so the vegetation layers are weighted as
    without snow.
    `one_call`: the whole run as ONE device-resident call with every coarse array left coarse (snow.runmicrosnow2_coarse): the
    snow model's chunk loop runs inside it, so it takes `snow_inputs` = runsnowmodela(..., method="slow", inputs_only=True) in
    place of `smod`; the solver interpolates the coarse arrays of `prepare_grid_inputs_array`, the snow days' weather is
    expanded on the device from the micropoints the host route reads.  `want_smod`: -> (outputs, the snow model's six series).
    reqhgt >= 0.  The default route is unchanged."""
    from . import snow as S
    if any(m is None for m in micropointa):
        raise ValueError("every coarse cell needs a micropoint")
    if one_call:
        return _runmicro_snow_array_one_call(micropointa, crows, ccols, reqhgt, vegp, soilc, dtm, snow_inputs, dtmc, lats, lons,
                                             altcorrect, pai_a, tfact, out, device, want_smod, _terrain)
    if smod is None:
        raise ValueError("smod (runsnowmodela's output) is needed; one_call=True takes snow_inputs instead")
    microsnow = S.gridmicrosnow2 if _microsnow is None else _microsnow

    def solve(mpa, **kw):
        if _solve is not None:
            return _solve(mpa, reqhgt, **kw)
        return runmicro_array(mpa, crows, ccols, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons, altcorrect=altcorrect, dtmc=dtmc,
                              device=device, **kw)
    veg, soil, z = cleanvars(vegp, soilc, dtm["z"])

    def solve_days(days, **kw):
        return solve([subsetpointmodel(m, days=days) for m in micropointa], **kw)

    def snow_days(sm, snowdays, ai, micro, outm):
        mps = [subsetpointmodel(m, days=snowdays) for m in micropointa]
        rowpos, colpos = api.coarse_positions(z.shape[0], crows), api.coarse_positions(z.shape[1], ccols)
        wc = {k: _stack_micropoints(mps, crows, ccols, lambda m, k=k: m["weather"][k]) for k in WEATHER}
        zc = np.nan_to_num(np.asarray(dtmc, dtype=np.float64), nan=0.0) if altcorrect else None
        w = S._fine_micro_inputs(wc, _stack_micropoints(mps, crows, ccols, lambda m: m["dfo"]["umu"]), slice(None), z, zc, rowpos, colpos,
                                 altcorrect)
        last = micropointa[-1]
        vg = sortl2(veg, np.zeros(last["ntme"]), reqhgt, pai_a)
        other = _snow_day_other(z, dtm, float(last["zref"]), np.asarray(lats, dtype=np.float64), np.asarray(lons, dtype=np.float64), soil,
                                device, _terrain)
        smods = {k: np.asfortranarray(np.asarray(sm[k])[:, :, ai]) for k in ("Tc", "Tg", "groundsnowdepth", "totalSWE", "snowden")}
        return microsnow(reqhgt, mps[0]["obstime"], w, smods, micro, vg, other, float(np.mean([m["matemp"] for m in micropointa])), outm)
    return _snow_host_route(smod, z, reqhgt, pai_a, tfact, out, device, solve_days, snow_days)


def snow_array_groups(micropointa: Sequence, crows: int, ccols: int, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping,
                      snow_inputs: Mapping, *, dtmc, lats, lons, altcorrect: int = 0, pai_a=None, tfact: float = 1.5,
                      out: Sequence = (1,) * 10, device: int = 0, _terrain=None):
    """-> (grid, snow, micro, mat): the three input groups of snow.runmicrosnow2_coarse / snow.SnowRun(micro_coarse=...) as
    `runmicro_snow_array` forms them — the solver's from `prepare_grid_inputs_array`, the snow model's = `snow_inputs`, the
    snow-day microclimate's coarse weather from the micropoints' own weather (each coarse cell's own wind direction) with
    `.sortl2`'s vegetation and the bare-ground terrain"""
    if reqhgt < 0:
        raise ValueError("the one-call snow run with array weather needs reqhgt >= 0")
    if snow_inputs is None or "clim_c" not in snow_inputs:
        raise ValueError('one_call: snow_inputs = runsnowmodela(..., method="slow", inputs_only=True) is needed')
    a = prepare_grid_inputs_array(micropointa, crows, ccols, reqhgt, vegp, soilc, dtm, lats=lats, lons=lons, pai_a=pai_a, out=out,
                                  device=device)
    a["tfact"] = float(tfact)
    veg, soil, z = cleanvars(vegp, soilc, dtm["z"])
    a["coarse"] = api._coarse_spec(a["vegp"], a["climdata"], None, None, altcorrect, dtmc, z, refuse_missing=False)
    last = micropointa[-1]
    vg = sortl2(veg, np.zeros(last["ntme"]), reqhgt, pai_a)
    other = _snow_day_other(z, dtm, float(last["zref"]), np.asarray(lats, dtype=np.float64), np.asarray(lons, dtype=np.float64), soil,
                            device, _terrain)
    grid = lambda get: _stack_micropoints(micropointa, crows, ccols, get)                      # noqa: E731
    micro = {"clim_c": {k: grid(lambda m, k=k: m["weather"][k]) for k in WEATHER}, "umu_c": grid(lambda m: m["dfo"]["umu"]),
             "obstime": micropointa[0]["obstime"], "vegp": vg, "other": other}
    return a, dict(snow_inputs), micro, float(np.mean([m["matemp"] for m in micropointa]))


def _runmicro_snow_array_one_call(micropointa, crows, ccols, reqhgt, vegp, soilc, dtm, snow_inputs, dtmc, lats, lons, altcorrect,
                                  pai_a, tfact, out, device, want_smod, _terrain):
    from . import snow as S
    g, sn, mi, mat = snow_array_groups(micropointa, crows, ccols, reqhgt, vegp, soilc, dtm, snow_inputs, dtmc=dtmc, lats=lats, lons=lons,
                                       altcorrect=altcorrect, pai_a=pai_a, tfact=tfact, out=out, device=device, _terrain=_terrain)
    if g.get("dfsel") is None:                                           # one vegetation layer: the library's one call
        return S.runmicrosnow2_coarse(g, sn, mi, mat, want_smod=want_smod, device=device)
    # time-varying vegetation: the staged form of the same run — pass 1 gives the no-snow days, which `.runmodel4Cpp` deals to
    # layers as a SUBSET (subset_day_layers); the solver's day -> layer map is set to that before pass 2
    with S.SnowRun(g, sn, device=device, micro_coarse=mi, want_umu=want_smod) as run:
        res = run.pass1(want_smod=want_smod)
        nd = np.flatnonzero(res[1]) + 1
        if nd.size:
            run.set_day_layers(subset_day_layers(micropointa[0], vegp, soilc, dtm, nd))
        outs = run.pass2(mi, mat)
        if not want_smod:
            return outs
        return outs, dict(res[2], umu=run.umu)


# ---- runbioclim() -> .runbioclim1 / .runbioclim3 ------------------------------------------------------------------
def biosel(obstime: Mapping, tc) -> dict:
    """`.biosel` (R/internal.R:1690-1729): the fourteen days a bioclim run models — for each month the day of median
    daily-mean temperature, then the hottest and the coldest day (of the median year when there are several).
    `seld`: 1-based day numbers, `selh`: 0-based hour indices."""
    tcd = np.asarray(tc, dtype=np.float64).reshape(-1, 24).mean(axis=1)
    mon = np.asarray(obstime["month"]).astype(int).reshape(-1, 24)[:, 12]       # the day's mean time falls on the day itself
    yr = np.asarray(obstime["year"]).astype(int).reshape(-1, 24)[:, 12]
    sel = []
    for m in range(1, 13):
        s = np.nonzero(mon == m)[0]
        o = np.argsort(tcd[s], kind="stable")
        sel.append(s[0] + o[len(o) // 2 - 1])                                   # s[1] - 1 + o[trunc(length(o) / 2)]
    mx, mn = [], []
    for y in dict.fromkeys(yr.tolist()):
        s = np.nonzero(yr == y)[0]
        mx.append(s[0] + int(np.argmax(tcd[s])))
        mn.append(s[0] + int(np.argmin(tcd[s])))
    mx = np.array(mx)[np.argsort(tcd[mx], kind="stable")]
    mn = np.array(mn)[np.argsort(tcd[mn], kind="stable")]
    k = len(mx) // 2                                                            # element trunc(n / 2) + 1, 1-based
    seld = np.array(sel + [mx[k], mn[k]]) + 1
    selh = (np.repeat((seld - 1) * 24, 24) + np.tile(np.arange(24), seld.size)).astype(np.int64)
    return {"seld": seld, "selh": selh}


def _quarter(values, months, how):
    """which.max / which.min of the circular three-month mean of the monthly aggregate (R/internal.R:1797-1802)"""
    ms = sorted(set(months.tolist()))
    agg = np.array([how(values[months == m]) for m in ms])
    sm = (np.roll(agg, 1) + agg + np.roll(agg, -1)) / 3
    return sm


def bioclim_quarters(precip, temp, months):
    """(wq, dq, hq, cq), 1-based months: the centre months of the wettest, driest, hottest and coldest quarter
    (R/internal.R:1796-1801 / 1911-1916; `precip`, `temp`: one value per step)"""
    pq = _quarter(precip, months, np.nanmean)
    tq = _quarter(temp, months, np.nansum)
    return int(np.argmax(pq)) + 1, int(np.argmin(pq)) + 1, int(np.argmax(tq)) + 1, int(np.argmin(tq)) + 1


def _bioclim_vegp14(veg, seld, n, vegpisannual, reqhgt, pai_a, mp) -> dict:
    """`.sortvegp2` (R/internal.R:2100-2130): the vegetation layer of each of the fourteen modelled days"""
    seld = seld % 365 if vegpisannual else seld
    nd = 365 if vegpisannual else int(round(n / 24))
    v14 = {}
    for k in VEG_KEYS:
        arr = as3d(veg[k])
        dmx = arr.shape[2]
        if dmx == 1:
            v14[k] = np.repeat(arr, 14, axis=2)
        else:
            sidx = layer_index(dmx, nd)
            sidx = np.concatenate([sidx, sidx[-1:]])
            v14[k] = arr[:, :, sidx[np.clip(seld, 1, len(sidx)) - 1] - 1]      # (seld = 0 would drop the day in R)
    pa = None if pai_a is None else intr(pai_a, mp["ntme"], mp["subs"])
    v14["leafden"], v14["paia"] = foliageden(reqhgt, v14["hgt"], v14["pai"], pa)
    return v14


def _getselq(mon2, iq):
    """`.getselq(iq, tme) - 1` (R/internal.R:1764-1774): the steps of the modelled series in the quarter around month iq"""
    imn, imx = (12 if iq == 1 else iq - 1), (1 if iq == 12 else iq + 1)
    return np.sort(np.concatenate([np.nonzero(mon2 == m)[0] for m in (imn, iq, imx)]))


def runbioclim(climdata: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, temp: str = "air",
               zref: float = 2.0, windhgt: float | None = None, soilm=None, pai_a=None, tfact: float = 1.5,
               out: Sequence = (1,) * 19, vegpisannual: bool = True, device: int = 0, _bioclim=None, _terrain=None) -> dict:
    """`runbioclim(climdata, reqhgt, vegp, soilc, dtm, ...)` for data.frame weather (R/Cppwrappers.R:628-651 ->
    `.runbioclim1` / `.runbioclim3`, R/internal.R:1776-1880 / 2083-2200): fourteen days are modelled (`biosel`) and the
    19 bioclim variables reduced from them on the device (mcf_runbioclim1 / 3).  Returns {bio1.. : [rows, cols]}."""
    ob_all = {k: np.asarray(climdata["obstime"][k]) for k in ("year", "month", "day", "hour")}
    mon_all = ob_all["month"].astype(int)
    t_all, p_all = np.asarray(climdata["temp"], dtype=np.float64), np.asarray(climdata["precip"], dtype=np.float64)
    wq, dq, hq, cq = bioclim_quarters(p_all, t_all, mon_all)
    sel = biosel(ob_all, t_all)
    w2 = {k: np.asarray(climdata[k])[sel["selh"]] for k in WEATHER}
    w2["obstime"] = {k: v[sel["selh"]] for k, v in ob_all.items()}
    veg, soil, z = cleanvars(vegp, soilc, dtm["z"])
    mp = runpointmodel(w2, reqhgt, dtm, vegp, soilc, zref=zref, windhgt=windhgt, soilm=soilm, yearG=False)
    layered = vegpdmx(veg) > 1
    ter_kw = {}
    if _terrain is not None:
        t = _terrain(z, dtm["res"] if np.isscalar(dtm["res"]) else dtm["res"][0], mp["zref"])
        ter_kw = dict(slr=t["slope"], apr=t["aspect"], hor=t["hor"], svf=t["svfa"], wsa=t["wsa"])
    static = {k: as3d(v)[:, :, 0] for k, v in veg.items()} if layered else vegp
    a = prepare_grid_inputs(mp, reqhgt, static, soilc, dtm, pai_a=None if layered else pai_a, device=device, **ter_kw)
    if layered:
        a["vegp"] = _bioclim_vegp14(veg, sel["seld"], len(t_all), vegpisannual, reqhgt, pai_a, mp)
    mon2 = np.asarray(w2["obstime"]["month"]).astype(int)
    args = {k: a[k] for k in ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp")}
    kw = dict(tfact=float(tfact), mat=a["mat"], out=[int(bool(v)) for v in out], wetq=_getselq(mon2, wq), dryq=_getselq(mon2, dq),
              hotq=_getselq(mon2, hq), colq=_getselq(mon2, cq), air=(temp == "air"))
    if _bioclim is not None:
        return _bioclim(layered, args, kw)
    fn = api.runbioclim3Cpp if layered else api.runbioclim1Cpp
    res = fn(**args, **kw, device=device)
    na = np.isnan(z)
    for v in res.values():
        v[na] = np.nan                                                          # mask(bior, dtm)
    return res


def runbioclim_depths(climdata: Mapping, depths, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, zref: float = 2.0,
                      windhgt: float | None = None, soilm=None, pai_a=None, tfact: float = 1.5, out: Sequence = (1,) * 19,
                      vegpisannual: bool = True, device: int = 0, chunk_days: int = 0, _bioclim=None, _terrain=None) -> dict:
    """`runbioclim` for soil temperatures at several depths from ONE solve (api.runbioclim_depths, mcf_runbioclim_depths):
    `runbioclim(climdata, reqhgt = depths[0], ..., temp = "air")` step by step — `biosel`, the quarters, the vegetation, and one
    `runpointmodel` at depths[0]: of the point model's series only `Tbz` depends on the height, and the run is made with
    complete = 1, which never reads it — with the library call replaced by the one that folds every depth.  `mask(bior, dtm)`
    is applied to every matrix.  Returns {"depths", "bio1" .. "bio11": [ndepths, rows, cols], "bio12" .. "bio19": [rows, cols]}.
    Array weather is not taken: `runbioclima` keeps its reqhgt < 0 refusal, because that route needs the per-cell point-model
    series this mirror does not carry."""
    d = np.atleast_1d(np.asarray(depths, dtype=np.float64)).ravel()
    if d.size < 1 or not np.all(d < 0):
        raise ValueError("runbioclim_depths: depths is a non-empty list of heights below ground (each < 0)")
    got = {}

    def capture(layered, args, kw):
        got.update(layered=layered, args=args, kw=kw)
        return {}

    runbioclim(climdata, float(d[0]), vegp, soilc, dtm, temp="air", zref=zref, windhgt=windhgt, soilm=soilm, pai_a=pai_a,
               tfact=tfact, out=out, vegpisannual=vegpisannual, device=device, _bioclim=capture, _terrain=_terrain)
    layered, args, kw = got["layered"], dict(got["args"]), got["kw"]
    args.pop("reqhgt")
    args["depths"] = d
    if _bioclim is not None:
        return _bioclim(layered, args, kw)
    res = api.runbioclim_depths(**args, **kw, layered=layered, device=device, chunk_days=chunk_days)
    na = np.isnan(cleanvars(vegp, soilc, dtm["z"])[2])
    for k, v in res.items():
        if k != "depths":
            v[..., na] = np.nan                                                 # mask(bior, dtm)
    return res


def bioclima_selection(climarray: Mapping, obstime: Mapping) -> dict:
    """What `.runbioclim2` / `.runbioclim4` decide from the weather alone (R/internal.R:1909-1916, 1749-1755): the four
    quarters from the spatial means of precipitation and temperature per step (`apply(..., 3, mean, na.rm = TRUE)`), and
    `biosel` on the spatial-mean temperature.  Returns {wq, dq, hq, cq (1-based months), seld, selh}."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                           # a step without data anywhere: NaN, as in R
        prech = np.nanmean(np.asarray(climarray["precip"], dtype=np.float64), axis=(0, 1))
        tc = np.nanmean(np.asarray(climarray["temp"], dtype=np.float64), axis=(0, 1))
    wq, dq, hq, cq = bioclim_quarters(prech, tc, np.asarray(obstime["month"]).astype(int))
    sel = biosel(obstime, tc)
    return dict(wq=wq, dq=dq, hq=hq, cq=cq, seld=sel["seld"], selh=sel["selh"])


def runbioclima(climarray: Mapping, obstime: Mapping, reqhgt: float, vegp: Mapping, soilc: Mapping, dtm: Mapping, *, lats, lons,
                clats, clons, dtmc=None, altcorrect: int = 0, temp: str = "air", zref: float = 2.0, windhgt: float | None = None,
                soilm=None, pai_a=None, tfact: float = 1.5, out: Sequence = (1,) * 19, vegpisannual: bool = True,
                device: int = 0, point_device: int | None = None, _bioclim=None, _terrain=None) -> dict:
    """`runbioclim()` for array weather (R/Cppwrappers.R:628-651 -> `.runbioclim2` / `.runbioclim4`, R/internal.R:1896-2081 /
    2200-2388): `climarray[k]` [crows, ccols, T] for the weather variables, `obstime` = {year, month, day, hour}.  The
    fourteen days `biosel` picks from the spatial-mean temperature are cut out of every array, the point model runs once per
    climate cell on them (`.biomicropoint`; `point_device`: as one batch on that device), and the solver interpolates the
    coarse climate and point-model arrays itself while the nineteen variables are reduced from its day chunks
    (runbioclim2Cpp_coarse / 4Cpp_coarse).  `lats`, `lons`: [rows, cols] of the raster; `clats`, `clons`: [crows, ccols] of
    the climate grid; `altcorrect` 1 / 2 with `dtmc` [crows, ccols]: as runmicro_array.  Returns {bio1.. : [rows, cols]}."""
    if reqhgt < 0:
        raise ValueError("coarse array forcing below ground needs the per-cell point-model series: not mirrored")
    if altcorrect and dtmc is None:
        raise ValueError("altcorrect needs dtmc, the elevations of the climate cells")
    ob_all = {k: np.asarray(obstime[k]) for k in ("year", "month", "day", "hour")}
    s = bioclima_selection(climarray, ob_all)
    cut = {k: np.asfortranarray(np.asarray(climarray[k], dtype=np.float64)[:, :, s["selh"]]) for k in WEATHER}
    ob2 = {k: v[s["selh"]] for k, v in ob_all.items()}
    cr, cc, n_all = np.shape(climarray["temp"])
    veg, soil, z = cleanvars(vegp, soilc, dtm["z"])
    mpa = runpointmodela(cut, ob2, reqhgt, dtm, vegp, soilc, lats=clats, lons=clons, zref=zref,
                         windhgt=zref if windhgt is None else windhgt, soilm=soilm, yearG=False, device=point_device)
    if any(m is None for m in mpa):
        raise ValueError("every coarse cell needs a micropoint")
    layered = vegpdmx(veg) > 1
    ter_kw = {}
    if _terrain is not None:
        t = _terrain(z, dtm["res"] if np.isscalar(dtm["res"]) else dtm["res"][0], mpa[0]["zref"])
        ter_kw = dict(slr=t["slope"], apr=t["aspect"], hor=t["hor"], svf=t["svfa"], wsa=t["wsa"])
    static = {k: as3d(v)[:, :, 0] for k, v in veg.items()} if layered else vegp
    a = prepare_grid_inputs_array(mpa, cr, cc, reqhgt, static, soilc, dtm, lats=lats, lons=lons,
                                  pai_a=None if layered else pai_a, device=device, **ter_kw)
    if layered:
        a["vegp"] = _bioclim_vegp14(veg, s["seld"], n_all, vegpisannual, reqhgt, pai_a, mpa[0])
    mon2 = ob2["month"].astype(int)
    args = {k: a[k] for k in ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "Sminp", "Smaxp")}
    args.update(lats=a["lat"], lons=a["lon"])
    R, Cc = z.shape
    kw = dict(tfact=float(tfact), mat=a["mat"], out=[int(bool(v)) for v in out], wetq=_getselq(mon2, s["wq"]),
              dryq=_getselq(mon2, s["dq"]), hotq=_getselq(mon2, s["hq"]), colq=_getselq(mon2, s["cq"]), air=(temp == "air"),
              rowpos=api.coarse_positions(R, cr), colpos=api.coarse_positions(Cc, cc))
    if altcorrect:
        kw.update(altcorrect=int(altcorrect), dtmc=dtmc, dtm=z)
    if _bioclim is not None:
        return _bioclim(layered, args, kw)
    fn = api.runbioclim4Cpp_coarse if layered else api.runbioclim2Cpp_coarse
    res = fn(**args, **kw, device=device)
    na = np.isnan(z)
    for v in res.values():
        v[na] = np.nan                                                          # mask(bior, dtm)
    return res


# ---- runmicro_big(): tiles of a large raster, one netCDF file each ---------------------------------------------------
def tile_size(nt: int, toverlap: int = 0) -> int:
    """the reference's automatic tile size (R/Cppwrappers.R:469-471): about 2e7 cell-steps per tile"""
    osize = np.sqrt(20000000 / nt) - 2 * toverlap
    sizeo = np.array([10, 20, 50, 100, 200, 500, 1000, 2000])
    return int(sizeo[np.argmin(np.abs(osize - sizeo))])


def tile_window(rw: int, cl: int, rows: int, cols: int, tilesize: int, toverlap: int):
    """`.croprast` (R/internal.R:1663-1676) in cell indices for unit-free overlap (the reference subtracts `toverlap` in
    map units): rows [r0, r1), cols [c0, c1) of tile (rw, cl), 1-based tile numbers, clipped to the raster"""
    r0, r1 = max((rw - 1) * tilesize - toverlap, 0), min(rw * tilesize + toverlap, rows)
    c0, c1 = max((cl - 1) * tilesize - toverlap, 0), min(cl * tilesize + toverlap, cols)
    return r0, r1, c0, c1


def runmicro_big(micropoint, reqhgt: float, pathout: str, vegp: Mapping, soilc: Mapping, dtm: Mapping, *,
                 tilesize: int | None = None, toverlap: int = 0, pai_a=None, tfact: float = 1.5,
                 vars: Sequence[str] | None = None, days_per_chunk: int = 5, device: int = 0, rank: int = 0,
                 world: int = 1, crows: int | None = None, ccols: int | None = None, lats=None, lons=None, dtmc=None,
                 altcorrect: int = 0) -> list:
    """`runmicro_big(micropoint, reqhgt, pathout, vegp, soilc, dtm, ..., writeasnc = TRUE)` for data.frame weather
    (R/Cppwrappers.R:446-541): slope, aspect, wetness index, horizons, sky view and wind shelter once for the WHOLE raster
    (wind shelter from the surface model dtm + hgt at 8 m, as there), then tile by tile the solver and
    `microut/area_RR_CC.nc`.  Each tile is solved in day chunks straight into its file (`pipeline.run_to_nc`): no tile's
    output ever exists on the host, and the tile size is only a file layout — the default keeps the reference's.
    `dtm` needs "xmin", "ymax" besides "z" / "res" / "lat" / "long" for the files' coordinates.  Returns the files written.
    With `world` > 1 (one process per GPU) the tiles are dealt round-robin: tile k goes to rank k % world; the universal
    variables are computed by every rank (seconds), no exchange is needed.
    (In the reference this function stops at an undefined `svfi`, R/Cppwrappers.R:520; what it sets out to do is done.)
    Array weather (`runmicro_big(micropointa, ..., dtm, dtmc, altcorrect)`, vignette "Running the model over large
    areas"): `micropoint` is `runpointmodela`'s list for a `crows` x `ccols` climate grid over the whole raster, `lats`,
    `lons` [rows, cols]; every tile interpolates the coarse arrays inside the solver at its own place in that grid, so
    tiles join without a seam in the forcing.
    reqhgt < 0: every tile runs the streamed below-ground plan through api.runmicro_nc (include/mcf.h mcf_runmicro_nc), so the
    whole series need not be resident; each file is ncsink.writetonc(runmicro(tile))."""
    import os
    from . import pipeline
    z_all = np.asarray(dtm["z"], dtype=np.float64)
    rows, cols = z_all.shape
    res = dtm["res"] if np.isscalar(dtm["res"]) else dtm["res"][0]
    array = not isinstance(micropoint, Mapping)
    if array and (crows is None or ccols is None or lats is None or lons is None or len(micropoint) != crows * ccols):
        raise ValueError("array weather needs crows, ccols (matching the list of micropoints), lats and lons")
    first = micropoint[0] if array else micropoint
    nt = len(first["weather"]["temp"])
    ts = tile_size(nt, toverlap) if tilesize is None else int(tilesize)
    os.makedirs(os.path.join(pathout, "microut"), exist_ok=True)
    # universal variables, R/Cppwrappers.R:482-499
    ter = terrain.precompute_terrain(z_all, res, first["zref"], what=("slope", "aspect", "hor", "svfa"), device=device)
    slr, apr = ter["slope"], ter["aspect"]
    slr[np.isnan(z_all)] = np.nan
    apr[np.isnan(z_all)] = np.nan
    twi = terrain.topidx(z_all, res)
    dsm = z_all + np.nan_to_num(as3d(vegp["hgt"])[:, :, 0], nan=0.0)
    wsa = terrain.precompute_terrain(dsm, res, 8.0, what=("wsa",), device=device)["wsa"]
    written = []
    k_tile = 0
    for rw in range(1, -(-rows // ts) + 1):
        for cl in range(1, -(-cols // ts) + 1):
            r0, r1, c0, c1 = tile_window(rw, cl, rows, cols, ts, toverlap)
            zi = z_all[r0:r1, c0:c1]
            if np.count_nonzero(~np.isnan(zi)) <= 1:
                continue
            k_tile += 1
            if (k_tile - 1) % world != rank:
                continue
            crop = lambda a: np.asarray(a)[r0:r1, c0:c1]                           # noqa: E731
            dtmi = dict(dtm, z=zi)
            vegi, soili = {k: crop(v) for k, v in vegp.items()}, {k: crop(v) for k, v in soilc.items()}
            pre = dict(pai_a=None if pai_a is None else crop(pai_a), slr=crop(slr), apr=crop(apr), hor=crop(ter["hor"]),
                       twi=crop(twi), wsa=crop(wsa), svf=crop(ter["svfa"]), device=device)
            if array:
                a = prepare_grid_inputs_array(micropoint, crows, ccols, reqhgt, vegi, soili, dtmi, lats=crop(lats), lons=crop(lons),
                                              **pre)
                a["coarse"] = {"rowpos": api.coarse_positions(rows, crows)[r0:r1], "colpos": api.coarse_positions(cols, ccols)[c0:c1]}
                if altcorrect:
                    a["coarse"].update(altcorrect=int(altcorrect), dtmc=dtmc, dtm=cleanvars(vegi, soili, zi)[2])
            else:
                a = prepare_grid_inputs(micropoint, reqhgt, vegi, soili, dtmi, **pre)
            a["tfact"] = float(tfact)
            fo = os.path.join(pathout, "microut", f"area_{rw:02d}_{cl:02d}.nc")
            ext = {"xmin": dtm["xmin"] + c0 * res, "xmax": dtm["xmin"] + c1 * res, "ymin": dtm["ymax"] - r1 * res,
                   "ymax": dtm["ymax"] - r0 * res, "res": res, "crs": dtm.get("crs", "")}
            if reqhgt < 0:      # below ground: the streamed plan's chunks through the same file sink (mcf_runmicro_nc)
                b = {k: v for k, v in a.items() if k != "out"}      # (the file's variables are what the solver computes)
                api.runmicro_nc(**b, fileout=fo, grid=ext, vars=vars, days_per_chunk=days_per_chunk, device=device, array_forcing=array)
            else:
                pipeline.run_to_nc(a, fo, ext, vars=vars, days_per_chunk=days_per_chunk, device=device, array_forcing=array)
            written.append(fo)
    return written
