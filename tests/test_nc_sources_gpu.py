"""netCDF sink: further sources, on the device (include/mcf.h "netCDF sink: further sources").  The yardstick is
literal: a file written by a one-call entry is, byte for byte, the file ncsink.writetonc writes from the arrays of the
array-returning entry of the same run (classic container).  23 x 31 cells: no multiple of the 32-wide transpose tiles nor of the
21-cell ring tiles; 4 days + 5 hours in chunks of 3 days: a short last chunk and steps past the last whole day."""
import filecmp

import numpy as np
import pytest

from microclimf_amd import _abi, api, ncsink, synthetic
from microclimf_amd import snow as S
from microclimf_amd.api import runmicro1Cpp, runmicro2Cpp

pytestmark = pytest.mark.gpu
ROWS, COLS, T = 23, 31, 4 * 24 + 5
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
GRID = dict(xmin=1000.0, xmax=1000.0 + COLS, ymin=500.0, ymax=500.0 + ROWS, res=1.0, crs="wkt of the test raster")
SERIES = _abi.SNOWDRIVER_OUT
_cache = {}


def same_file(got, want, what):
    assert filecmp.cmp(got, want, shallow=False), f"{what}: the files differ"


def records(path, rows, cols, nvars, nsteps):
    """(time words [nsteps], values [nsteps, nvars, rows, cols]) of a classic file: the records are its tail"""
    raw = np.fromfile(path, dtype=np.uint8)
    rec = 8 + nvars * rows * cols * 4
    tail = raw[raw.size - nsteps * rec:].reshape(nsteps, rec)
    return tail[:, :8].copy().view(">f8")[:, 0], tail[:, 8:].copy().view(">i4").reshape(nsteps, nvars, rows, cols)


def pack(x, scale):
    """writetonc's `atonc` by numpy: [rows, cols, n] -> [n, rows, cols] int32, round half even, NA / out of range -> -9999"""
    with np.errstate(invalid="ignore"):
        q = np.rint(np.asarray(x, dtype=np.float64) * scale)
        ok = (q > -2147483648.0) & (q < 2147483648.0)
    return np.transpose(np.where(ok, q, -9999.0).astype(np.int32), (2, 0, 1))


# ---- 1. crafted planes through k_pack_nc_planes ----------------------------------------------------------------------------------
def crafted(rows, cols, n, seed):
    rng = np.random.default_rng(seed)
    x = {v: np.asfortranarray(np.round(rng.normal(size=(rows, cols, n)) * 40, 4)) for v in SERIES}
    flat = x["Tc"].reshape(-1, order="F")
    special = [0.005, 0.015, 0.025, -0.005, -0.015, 1.125, np.nan, 3e9, -3e9, -0.0, 21474836.47, 21474836.48, -21474836.48, np.inf, -np.inf]
    flat[:min(len(special), flat.size)] = special[:flat.size]      # x 100: ties at .5, both signs; the int32 range's two edges
    x["Tc"] = np.asfortranarray(flat.reshape((rows, cols, n), order="F"))
    x["snowden"][-1, -1, -1] = 2.5       # x 1: a tie
    x["groundsnowdepth"][0, -1, 0] = 0.0125      # x 1000: a tie
    return x


@pytest.mark.parametrize("rows,cols,n", [(23, 31, 3), (1, 1, 2), (33, 65, 2)], ids=["23x31", "one-cell", "33x65"])
def test_1_crafted_planes_equal_numpys_rint_packing(tmp_path, rows, cols, n):
    x = crafted(rows, cols, n, rows)
    hours, east, north = 400000.0 + np.arange(n), np.arange(cols) + 0.5, np.arange(rows) + 0.5
    f = tmp_path / "planes.nc"
    with ncsink.SnowpackNcWriter(f, rows, cols, hours, east, north) as w:
        ms = w.write_planes(0, 0, x, timing=True)
        assert ms > 0.0
    tw, got = records(f, rows, cols, 5, n)
    assert np.array_equal(tw, hours)
    for k, v in enumerate(SERIES):
        assert np.array_equal(got[:, k], pack(x[v], ncsink.SNOWPACK_SCALE[v])), v
    if rows * cols * n >= 15:
        assert (got[:, 0] == -9999).sum() >= 5 and (got[:, 0] == 2147483647).sum() == 1 and (got[:, 0] == 0).sum() >= 2
    # the same planes as three row strips in descending order, the later step first: the same file
    if rows >= 3:
        g = tmp_path / "strips.nc"
        with ncsink.SnowpackNcWriter(g, rows, cols, hours, east, north) as w:
            for r0, r1 in ((2 * rows // 3, rows), (rows // 3, 2 * rows // 3), (0, rows // 3)):
                w.write_planes(r0, 1, {v: x[v][r0:r1, :, 1:] for v in SERIES})
                w.write_planes(r0, 0, {v: x[v][r0:r1, :, :1] for v in SERIES})
        same_file(g, f, "row strips of planes")
    # a subset of the series: the file's variables in mcf_snowdriver_out's order
    h = tmp_path / "two.nc"
    with ncsink.SnowpackNcWriter(h, rows, cols, hours, east, north, vars=("totalSWE", "Tg")) as w:
        w.write_planes(0, 0, x)
        with pytest.raises(_abi.McfError, match="error 1: mcf_nc_write_planes: step range outside the file"):
            w.write_planes(0, n, x)
        with pytest.raises(_abi.McfError, match="error 1: mcf_nc_write_planes: .*not a row strip"):
            w.write_planes(1, 0, x)
    _, got2 = records(h, rows, cols, 2, n)
    assert np.array_equal(got2[:, 0], pack(x["Tg"], 100)) and np.array_equal(got2[:, 1], pack(x["totalSWE"], 100))


# ---- 2. - 5. the solver ------------------------------------------------------------------------------------------------------------
def solver_case(key):
    """(arguments, the file writetonc makes of the array entry's outputs) per case, made once"""
    if key in _cache:
        return _cache[key]
    reqhgt, af, complete = key
    a = synthetic.workload(ROWS, COLS, T, reqhgt=reqhgt, variety=True, na_frac=0.04, start_doy=150, complete=bool(complete),
                           array_forcing=af)
    names = ncsink.default_vars(reqhgt)
    a["out"] = [1 if n in names else 0 for n in _abi.OUT_NAMES]
    want = (runmicro2Cpp if af else runmicro1Cpp)(*[a[k] for k in ARGS], a["out"], days_per_chunk=3)
    for v in want.values():
        v.setflags(write=False)
    _cache[key] = (a, names, want)
    return _cache[key]


def reference_file(tmp_path, key):
    a, names, want = solver_case(key)
    f = tmp_path / "reference.nc"
    ncsink.writetonc(dict(want, tme=a["obstime"]), f, GRID, key[0], names)
    return f


def nc_args(a):
    return {k: a[k] for k in ARGS}


@pytest.mark.parametrize("reqhgt,af", [(0.05, False), (0.0, False), (2.5, True)], ids=["0.05m", "surface", "2.5m-arrays"])
def test_2_runmicro_nc_equals_writetonc_of_the_arrays(tmp_path, reqhgt, af):
    key = (reqhgt, af, 1)
    a, names, want = solver_case(key)
    ref = reference_file(tmp_path, key)
    f = tmp_path / "direct.nc"
    got = api.runmicro_nc(**nc_args(a), fileout=f, grid=GRID, array_forcing=af, days_per_chunk=3)
    assert got == names
    same_file(f, ref, f"runmicro_nc at {reqhgt}")
    # the steps past the last whole day are missval, the others are not all
    tw, vals = records(f, ROWS, COLS, len(names), T)
    assert (vals[96:] == -9999).all() and (vals[:96, 0] != -9999).any() and (vals[:96, 0] == -9999).any()
    assert np.array_equal(tw, ncsink.hours_since_epoch(a["obstime"]))
    if not af:      # one-day chunks and the chunk the ring budget gives: the same file
        for chunk in (1, 0):
            g = tmp_path / f"chunk{chunk}.nc"
            api.runmicro_nc(**nc_args(a), fileout=g, grid=GRID, days_per_chunk=chunk)
            same_file(g, ref, f"chunks of {chunk}")


@pytest.mark.parametrize("complete", (0, 1))
def test_3_below_ground_streamed(tmp_path, complete):
    key = (-0.1, False, complete)
    a, names, want = solver_case(key)
    assert names == ("Tz", "soilm")
    ref = reference_file(tmp_path, key)
    f = tmp_path / "below.nc"
    api.runmicro_nc(**nc_args(a), fileout=f, grid=GRID, days_per_chunk=3)
    same_file(f, ref, f"below ground, complete {complete}")
    _, vals = records(f, ROWS, COLS, 2, T)
    # the steps past the last whole day: what the array entry returns there, soilm missval; with complete = 1 Tbelowgroundv's
    # means run over every step and Tz is there (complete = 0 adds the ground temperature's anomaly, which those steps lack)
    assert np.array_equal(vals[96:, 0], pack(want["Tz"][:, :, 96:], 100)) and (vals[96:, 1] == -9999).all()
    assert (vals[96:, 0] != -9999).any() == bool(complete)
    g = tmp_path / "tz.nc"      # Tz alone, one-day chunks
    api.runmicro_nc(**nc_args(a), fileout=g, grid=GRID, vars=("Tz",), days_per_chunk=1)
    _, tz = records(g, ROWS, COLS, 1, T)
    assert np.array_equal(tz[:, 0], vals[:, 0])


@pytest.mark.parametrize("complete", (0, 1))
def test_4_three_depths_from_one_solve(tmp_path, complete):
    from test_below_depths_gpu import at_depth, tbp_rows
    depths = (-0.1, -0.02, -0.5)
    a, names, want = solver_case((-0.1, False, complete))
    tbp = tbp_rows(a, depths)
    files = [tmp_path / f"depth{d}.nc" for d in range(3)]
    b = {k: a[k] for k in ARGS if k != "reqhgt"}
    api.runmicro_depths_nc(**b, depths=depths, tbp=None if complete else tbp, files=files, grid=GRID, days_per_chunk=3)
    for d, depth in enumerate(depths):      # test 3's route at that depth
        one = tmp_path / f"one{d}.nc"
        api.runmicro_nc(**nc_args(at_depth(a, depth, tbp[d])), fileout=one, grid=GRID, days_per_chunk=3)
        same_file(files[d], one, f"depth {depth}, complete {complete}")
        assert f"Soil temperature at depth {abs(depth):g} m".encode() in files[d].read_bytes()
    assert not filecmp.cmp(files[0], files[1], shallow=False)


@pytest.mark.parametrize("key", [(0.05, False, 1), (-0.1, False, 0), (-0.1, False, 1)], ids=["0.05m", "below-0", "below-1"])
def test_5_three_row_blocks_on_one_device_write_the_one_block_file(tmp_path, key):
    a, names, want = solver_case(key)
    ref = reference_file(tmp_path, key)
    f = tmp_path / "blocks.nc"
    api.runmicro_nc(**nc_args(a), fileout=f, grid=GRID, days_per_chunk=3, devices=[0, 0], n_blocks=3)
    same_file(f, ref, f"three row blocks, {key}")


# ---- 7. the snowpack ------------------------------------------------------------------------------------------------------------------
def snow_case():
    """22 x 13 cells, 22 days in 5-day chunks: four whole chunks and two days no chunk covers (tests/test_series_sources_gpu.py)"""
    if "snow" not in _cache:
        from test_snowrun_gpu import _case
        sw, a, dtm, snow, micro = _case(0.05, 0.0, 90, ndays=22)
        args = (sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
        _cache["snow"] = (sw, args, dtm)
    return _cache["snow"]


def check_snowpack_file(f, series, obstime, what):
    rows, cols, n = series["Tc"].shape
    tw, got = records(f, rows, cols, 5, n)
    assert np.array_equal(tw, ncsink.hours_since_epoch(obstime)), what
    for k, v in enumerate(SERIES):
        assert np.array_equal(got[:, k], pack(series[v], ncsink.SNOWPACK_SCALE[v])), (what, v)
    return got


@pytest.mark.parametrize("blocks", (1, 3))
def test_7_snowmodel1_nc_equals_the_packed_arrays(tmp_path, blocks):
    sw, args, dtm = snow_case()
    kw = dict(devices=[0, 0], n_blocks=3) if blocks == 3 else {}
    series = S.snowmodel1_chunks(*args, **kw)      # (snow blocks differ from one block in last bits: the arrays of the same count)
    rows, cols = dtm.shape
    grid = dict(xmin=0.0, xmax=float(cols), ymin=0.0, ymax=float(rows), res=1.0)
    f = tmp_path / "pack.nc"
    assert S.snowmodel1_nc(*args, fileout=f, grid=grid, **kw) == SERIES
    got = check_snowpack_file(f, series, sw["obstime"], f"{blocks} block(s)")
    assert (got[480:] == -9999).all() and (got[:480, 3] > 0).any() and (got[:480, 3] == -9999).any()      # the tail; snow; NA cells
    if blocks == 1:      # the stepwise plan with the chunks written in descending order
        g = tmp_path / "stepwise.nc"
        hours, east, north, _ = ncsink.grid_of(grid, sw["obstime"])
        with ncsink.SnowpackNcWriter(g, rows, cols, hours, east, north) as w, S.SnowPlan(*args, keep_results=False) as p:
            for ch in range(p.chunks):
                p.checkpoint(ch)
                ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
                p.run_chunk(ch, ts / tn)
            for ch in reversed(range(p.chunks)):
                p.restore(ch)
                ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
                if ch == 1:      # a run that leaves a series of the file out cannot be written
                    p.set_series(S.SnowPlan.SERIES_PASS1)
                    p.run_chunk(ch, ts / tn)
                    with pytest.raises(_abi.McfError, match="error 5: mcf_snowplan_nc_write: .*switched off"):
                        p.nc_write(w, ch)
                    p.set_series(S.SnowPlan.SERIES_ALL)
                    p.restore(ch)
                    ts, tn = p.prepare_chunk(ch, surface_mean=np.divide(*p.surface_partial()))
                p.run_chunk(ch, ts / tn)
                p.nc_write(w, ch)
            with pytest.raises(_abi.McfError, match="error 1: mcf_snowplan_nc_write: chunk out of range"):
                p.nc_write(w, p.chunks)
        same_file(g, f, "stepwise, descending")


# ---- 8. the netCDF-4 container: one block -------------------------------------------------------------------------------------------
def test_8_netcdf4_files_hold_the_classic_files_values(tmp_path):
    import h5mini
    if h5mini.load() is None:
        pytest.skip("no HDF5 library on this host (the netCDF-4 container needs one)")
    for key in ((0.05, False, 1), (-0.1, False, 1)):
        a, names, want = solver_case(key)
        f = tmp_path / "n4.nc"
        api.runmicro_nc(**nc_args(a), fileout=f, grid=GRID, days_per_chunk=3, format="netcdf4")
        _, vals = records(reference_file(tmp_path, key), ROWS, COLS, len(names), T)
        h = h5mini.File(f)
        for k, n in enumerate(names):
            assert np.array_equal(h.read(n), vals[:, k]), (key, n)
        assert np.array_equal(h.read("time"), ncsink.hours_since_epoch(a["obstime"]))
        h.close()
        api.runmicro_nc(**nc_args(a), fileout=f, grid=GRID, days_per_chunk=3, format="netcdf4", devices=[0], n_blocks=1)      # one block
    sw, args, dtm = snow_case()
    rows, cols = dtm.shape
    grid = dict(xmin=0.0, xmax=float(cols), ymin=0.0, ymax=float(rows), res=1.0)
    S.snowmodel1_nc(*args, fileout=tmp_path / "p4.nc", grid=grid, format="netcdf4")
    S.snowmodel1_nc(*args, fileout=tmp_path / "pc.nc", grid=grid)
    _, vals = records(tmp_path / "pc.nc", rows, cols, 5, 528)
    h = h5mini.File(tmp_path / "p4.nc")
    for k, n in enumerate(SERIES):
        assert np.array_equal(h.read(n), vals[:, k]), n
    h.close()


# ---- 6. the snow run ----------------------------------------------------------------------------------------------------------------
MAT = 7.5


def snowrun_case(reqhgt, blocks=1):
    """22 x 13 cells, 22 days: four merged ring chunks and two days past the last whole chunk; the arrays of the one-call run"""
    key = ("snowrun", reqhgt, blocks)
    if key not in _cache:
        from test_snowrun_gpu import _case
        sw, a, dtm, snow, micro = _case(reqhgt, 0.0, 90, ndays=22)
        names = ncsink.default_vars(reqhgt)
        a["out"] = [1 if n in names else 0 for n in _abi.OUT_NAMES]
        kw = dict(devices=[0, 0], n_blocks=3) if blocks == 3 else {}
        arrays, smod = S.runmicrosnow1(a, snow, micro, MAT, want_smod=True, below=reqhgt < 0, **kw)
        for v in list(arrays.values()) + list(smod.values()):
            v.setflags(write=False)
        rows, cols = dtm.shape
        grid = dict(xmin=0.0, xmax=float(cols), ymin=0.0, ymax=float(rows), res=1.0, crs="wkt")
        _cache[key] = dict(sw=sw, a=a, snow=snow, micro=micro, names=names, arrays=arrays, smod=smod, grid=grid, kw=kw)
    return _cache[key]


def snowrun_reference(tmp_path, c, reqhgt):
    ref = tmp_path / "reference.nc"
    ncsink.writetonc(dict(c["arrays"], tme=c["sw"]["obstime"]), ref, c["grid"], reqhgt, c["names"])
    return ref


@pytest.mark.parametrize("reqhgt,blocks", [(0.05, 1), (0.0, 1), (-0.1, 1), (0.05, 3), (-0.1, 3)],
                         ids=["0.05m", "surface", "below", "0.05m-3-blocks", "below-3-blocks"])
def test_6_file_only_snow_run_equals_writetonc_of_the_runs_arrays(tmp_path, reqhgt, blocks):
    c = snowrun_case(reqhgt, blocks)
    ref = snowrun_reference(tmp_path, c, reqhgt)
    f, g = tmp_path / "run.nc", tmp_path / "pack.nc"
    res = S.runmicrosnow_nc(c["a"], c["snow"], c["micro"], MAT, fileout=f, pack_fileout=g, nc_grid=c["grid"], **c["kw"])
    assert res["out"] is None and res["snowdays"].sum() > 0 and res["nosnowdays"].sum() > 0
    same_file(f, ref, f"snow run at {reqhgt}, {blocks} block(s)")
    check_snowpack_file(g, c["smod"], c["sw"]["obstime"], "the snow run's pack_file")
    _, vals = records(f, 22, 13, len(c["names"]), 528)
    assert (vals[:, 0] != -9999).any() and (vals[480:, 0] != -9999).any()      # the days past the last whole chunk are the solver's


def test_6b_the_file_beside_the_arrays_changes_no_bit_and_no_counter(tmp_path):
    c = snowrun_case(0.05)
    hours, east, north, crs = ncsink.grid_of(c["grid"], c["sw"]["obstime"])
    with S.SnowRun(c["a"], c["snow"]) as plain:
        sd0, nd0 = plain.pass1()
        arrays0, stats0 = plain.pass2(c["micro"], MAT), plain.stats()
    f, g = tmp_path / "run.nc", tmp_path / "pack.nc"
    with S.SnowRun(c["a"], c["snow"]) as run, ncsink.NcWriter(f, 22, 13, hours, east, north, 0.05, c["names"], crs) as w, \
            ncsink.SnowpackNcWriter(g, 22, 13, hours, east, north, crs_wkt=crs) as pw:
        with pytest.raises(_abi.McfError, match="error 1: mcf_snowrun_nc_enable: the outputs' file holds the snowpack's series"):
            run.nc_enable(pw, None)
        with pytest.raises(_abi.McfError, match="error 1: mcf_snowrun_nc_enable: the snowpack's file was not made by mcf_nc_create_snowpack"):
            run.nc_enable(None, w)
        run.nc_enable(w, pw)
        with pytest.raises(_abi.McfError, match="error 5: mcf_snowrun_nc_enable: .*already enabled"):
            run.nc_enable(w, pw)
        sd, nd, smod = run.pass1(want_smod=True)
        arrays, stats = run.pass2(c["micro"], MAT), run.stats()
    assert np.array_equal(sd, sd0) and np.array_equal(nd, nd0) and stats == stats0
    for k in arrays0:
        assert np.array_equal(arrays[k].view(np.uint64), arrays0[k].view(np.uint64)), k
        assert np.array_equal(arrays[k].view(np.uint64), c["arrays"][k].view(np.uint64)), k
    same_file(f, snowrun_reference(tmp_path, c, 0.05), "the file beside the arrays")
    check_snowpack_file(g, smod, c["sw"]["obstime"], "pack_file beside the arrays")
    with S.SnowRun(c["a"], c["snow"]) as late:
        late.pass1()
        with ncsink.NcWriter(tmp_path / "late.nc", 22, 13, hours, east, north, 0.05, c["names"], crs) as w:
            with pytest.raises(_abi.McfError, match="error 5: mcf_snowrun_nc_enable: .*before mcf_snowrun_pass1"):
                late.nc_enable(w)


def test_6c_array_weather_snow_run(tmp_path):
    from test_snowrun2_gpu import _case as case2
    sw, a, dtm, snow, micro = case2(0.05, 0.0, 90, ndays=12)      # two whole chunks and two days past them
    names = ncsink.default_vars(0.05)
    a["out"] = [1 if n in names else 0 for n in _abi.OUT_NAMES]
    arrays = S.runmicrosnow2(a, snow, micro, 6.5)
    rows, cols = dtm.shape
    grid = dict(xmin=0.0, xmax=float(cols), ymin=0.0, ymax=float(rows), res=1.0)
    ref, f = tmp_path / "reference.nc", tmp_path / "run.nc"
    ncsink.writetonc(dict(arrays, tme=snow["obstime"]), ref, grid, 0.05, names)
    S.runmicrosnow_nc(a, snow, micro, 6.5, fileout=f, nc_grid=grid)
    same_file(f, ref, "array weather")


# ---- 9. the front end on the bundled site -------------------------------------------------------------------------------------------
def test_9_runmicro_big_below_ground_writes_writetonc_of_runmicro_per_tile(tmp_path):
    from bundled import load
    from microclimf_amd import frontend as F
    w, vegp, soilc, dtm = load(4 * 24)      # (the front end's grid model takes whole days)
    mp = F.runpointmodel(w, -0.1, dtm, vegp, soilc)
    rows, cols = np.shape(dtm["z"])
    dtm = dict(dtm, xmin=float(dtm["extent"][0]), ymax=float(dtm["extent"][3]))
    files = F.runmicro_big(mp, -0.1, str(tmp_path), vegp, soilc, dtm, tilesize=20, toverlap=3, days_per_chunk=3)
    assert len(files) == 9
    # each file against runmicro on the tile with the universal variables cropped as runmicro_big crops them
    z_all = np.asarray(dtm["z"], dtype=np.float64)
    res = dtm["res"]
    ter = F.terrain.precompute_terrain(z_all, res, mp["zref"], what=("slope", "aspect", "hor", "svfa"))
    slr, apr = ter["slope"], ter["aspect"]
    slr[np.isnan(z_all)] = np.nan
    apr[np.isnan(z_all)] = np.nan
    twi = F.terrain.topidx(z_all, res)
    wsa = F.terrain.precompute_terrain(z_all + np.nan_to_num(F.as3d(vegp["hgt"])[:, :, 0], nan=0.0), res, 8.0, what=("wsa",))["wsa"]
    k = 0
    for rw in range(1, -(-rows // 20) + 1):
        for cl in range(1, -(-cols // 20) + 1):
            r0, r1, c0, c1 = F.tile_window(rw, cl, rows, cols, 20, 3)
            zi = z_all[r0:r1, c0:c1]
            if np.count_nonzero(~np.isnan(zi)) <= 1:
                continue
            crop = lambda a: np.asarray(a)[r0:r1, c0:c1]      # noqa: E731
            got = F.runmicro(mp, -0.1, {q: crop(v) for q, v in vegp.items()}, {q: crop(v) for q, v in soilc.items()}, dict(dtm, z=zi),
                             out=(1, 0, 0, 1, 0, 0, 0, 0, 0, 0), slr=crop(slr), apr=crop(apr), hor=crop(ter["hor"]), twi=crop(twi),
                             wsa=crop(wsa), svf=crop(ter["svfa"]))
            ref = tmp_path / f"ref_{rw}_{cl}.nc"
            ncsink.writetonc(dict(got, tme=w["obstime"]), ref, F.nc_extent(dtm, r1 - r0, c1 - c0, r0, c0), -0.1, ("Tz", "soilm"))
            same_file(files[k], ref, f"tile {rw}, {cl}")
            k += 1
    assert k == len(files)


# ---- 6d. a day of neither class, and steps past the last whole day, through pass 2 --------------------------------------------------
def odd_snow_case(reqhgt):
    """22 days + 5 hours on 22 x 13 cells (tests/test_snowrun_gpu.py's case with a ragged end)"""
    T = 22 * 24 + 5
    sw = synthetic.snow_workload(22, 13, T, cold=0.0, zref=3.5, start_doy=90)
    a = synthetic.workload(22, 13, T, reqhgt=reqhgt, zref=3.5, hgt_range=(0.05, 3.0), start_doy=90, variety=True)
    _, _, dtm = synthetic.rasters(22, 13)
    dtm = np.where(np.isnan(sw["vegp"]["hgt"]), np.nan, dtm)
    names = ncsink.default_vars(reqhgt)
    a["out"] = [1 if n in names else 0 for n in _abi.OUT_NAMES]
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    return sw, a, snow, micro, names, T


def days_to_drop(sd, nd):
    """a day of the solver alone inside the chunk loop that has classed days on both sides in its chunk where there is one, and
    the first day past the last whole chunk"""
    alone = np.flatnonzero((sd == 0) & (nd == 1))
    inside = [int(d) for d in alone if d < 20]
    assert inside and 20 in alone, (sd, nd)
    mid = [d for d in inside if d % 5 not in (0, 4)]
    return [mid[0] if mid else inside[0], 20]


@pytest.mark.parametrize("reqhgt,blocks", [(0.05, 1), (0.05, 3), (-0.1, 1)], ids=["0.05m", "0.05m-3-blocks", "below"])
def test_6d_days_of_neither_class_and_a_ragged_end_through_pass2(tmp_path, reqhgt, blocks):
    sw, a, snow, micro, names, T = odd_snow_case(reqhgt)
    kw = dict(devices=[0, 0], n_blocks=3) if blocks == 3 else {}
    grid = dict(xmin=0.0, xmax=13.0, ymin=0.0, ymax=22.0, res=1.0, crs="wkt")
    hours, east, north, crs = ncsink.grid_of(grid, sw["obstime"])
    with S.SnowRun(a, snow, below=reqhgt < 0, **kw) as run:
        sd, nd = run.pass1()
        drop = days_to_drop(sd, nd)
        with pytest.raises(_abi.McfError, match="error 1: mcf_snowrun_drop_days: day .* is a snow day"):
            run.drop_days([int(np.flatnonzero(sd)[0])])
        run.drop_days(drop)
        arrays = run.pass2(micro, MAT)
    for d in drop:      # no day of either model: NA for every cell
        assert np.isnan(arrays["Tz"][:, :, d * 24:(d + 1) * 24]).all(), d
    assert np.isnan(arrays["Tz"][:, :, 528:]).all() and np.isfinite(arrays["Tz"][:, :, 504:528]).any()
    ref, f = tmp_path / "reference.nc", tmp_path / "run.nc"
    ncsink.writetonc(dict(arrays, tme=sw["obstime"]), ref, grid, reqhgt, names)
    with S.SnowRun(a, snow, below=reqhgt < 0, **kw) as run, ncsink.NcWriter(f, 22, 13, hours, east, north, reqhgt, names, crs) as w:
        run.nc_enable(w)
        sd2, nd2 = run.pass1()
        assert np.array_equal(sd2, sd) and np.array_equal(nd2, nd)
        run.drop_days(drop)
        assert run.pass2(micro, MAT, want_arrays=False) is None
    same_file(f, ref, f"dropped days {drop} and a ragged end at {reqhgt}, {blocks} block(s)")
    _, vals = records(f, 22, 13, len(names), T)
    for d in drop:
        assert (vals[d * 24:(d + 1) * 24] == -9999).all() and (vals[(d - 1) * 24:d * 24, 0] != -9999).any(), d
    assert (vals[528:] == -9999).all()
    # the one call on the ragged series (no day dropped): the file of its arrays
    if blocks == 1:
        one = S.runmicrosnow1(a, snow, micro, MAT, below=reqhgt < 0)
        ncsink.writetonc(dict(one, tme=sw["obstime"]), ref, grid, reqhgt, names)
        S.runmicrosnow_nc(a, snow, micro, MAT, fileout=f, nc_grid=grid)
        same_file(f, ref, f"one call, ragged end, {reqhgt}")


# ---- 8b. netcdf4 for the other sources: depth files, the snow run's two files ---------------------------------------------------------
def test_8b_netcdf4_depth_files_and_snow_run_files(tmp_path):
    import h5mini
    from test_below_depths_gpu import tbp_rows
    if h5mini.load() is None:
        pytest.skip("no HDF5 library on this host (the netCDF-4 container needs one)")
    depths = (-0.1, -0.5)
    a, names, want = solver_case((-0.1, False, 0))
    b = {k: a[k] for k in ARGS if k != "reqhgt"}
    tbp = tbp_rows(a, depths)
    n4 = [tmp_path / f"d{d}.nc4" for d in range(2)]
    cl = [tmp_path / f"d{d}.nc" for d in range(2)]
    api.runmicro_depths_nc(**b, depths=depths, tbp=tbp, files=n4, grid=GRID, days_per_chunk=3, format="netcdf4")
    api.runmicro_depths_nc(**b, depths=depths, tbp=tbp, files=cl, grid=GRID, days_per_chunk=3)
    for d in range(2):
        _, vals = records(cl[d], ROWS, COLS, 2, T)
        h = h5mini.File(n4[d])
        assert np.array_equal(h.read("Tz"), vals[:, 0]) and np.array_equal(h.read("soilm"), vals[:, 1]), d
        assert h.attr("Tz", "long_name") == f"Soil temperature at depth {abs(depths[d]):g} m".encode()
        h.close()
    # the snow run: runs of days, a dropped day and the ragged end arrive as pieces of whole rasters
    sw, a2, snow, micro, names2, T2 = odd_snow_case(0.05)
    grid = dict(xmin=0.0, xmax=13.0, ymin=0.0, ymax=22.0, res=1.0, crs="wkt")
    hours, east, north, crs = ncsink.grid_of(grid, sw["obstime"])
    files = {}
    for fmt in ("classic", "netcdf4"):
        f, g = tmp_path / f"run.{fmt}", tmp_path / f"pack.{fmt}"
        with S.SnowRun(a2, snow) as run, ncsink.NcWriter(f, 22, 13, hours, east, north, 0.05, names2, crs, format=fmt) as w, \
                ncsink.SnowpackNcWriter(g, 22, 13, hours, east, north, crs_wkt=crs, format=fmt) as pw:
            run.nc_enable(w, pw)
            sd, nd = run.pass1()
            run.drop_days(days_to_drop(sd, nd))
            run.pass2(micro, MAT, want_arrays=False)
        files[fmt] = (f, g)
    _, vals = records(files["classic"][0], 22, 13, len(names2), T2)
    _, pvals = records(files["classic"][1], 22, 13, 5, T2)
    h = h5mini.File(files["netcdf4"][0])
    for k, n in enumerate(names2):
        assert np.array_equal(h.read(n), vals[:, k]), n
    h.close()
    h = h5mini.File(files["netcdf4"][1])
    for k, n in enumerate(SERIES):
        assert np.array_equal(h.read(n), pvals[:, k]), n
    h.close()
    with pytest.raises(_abi.McfError, match="error 1: mcf_snowrun_nc_enable: .*netCDF-4 container .* one block"):
        with S.SnowRun(a2, snow, devices=[0, 0], n_blocks=3) as run, \
                ncsink.NcWriter(tmp_path / "x.nc4", 22, 13, hours, east, north, 0.05, names2, crs, format="netcdf4") as w:
            run.nc_enable(w)


# ---- 9b. the front ends on the bundled site -------------------------------------------------------------------------------------------
def bundled_snow():
    from bundled import load
    from microclimf_amd import frontend as F
    weather, vegp, soilc, dtm = load(12 * 24)
    t = np.arange(12 * 24)
    weather = dict(weather, temp=weather["temp"] - 9.0 + 7.0 * (t > 4 * 24) + 6.0 * (t > 8 * 24))      # (tests/test_snow_summary_gpu.py)
    dtm = dict(dtm, xmin=float(dtm["extent"][0]), ymax=float(dtm["extent"][3]))
    return F, weather, vegp, soilc, dtm


def test_9b_front_end_runmicro_nc_and_depths_nc(tmp_path):
    from bundled import load
    from microclimf_amd import frontend as F
    w, vegp, soilc, dtm = load(3 * 24)
    dtm = dict(dtm, xmin=float(dtm["extent"][0]), ymax=float(dtm["extent"][3]))
    ext = F.nc_extent(dtm, 50, 50)
    assert ext["xmax"] - ext["xmin"] == 50 * dtm["res"] and ext["ymax"] == dtm["ymax"]
    mp = F.runpointmodel(w, 0.05, dtm, vegp, soilc)
    names = ("Tz", "relhum", "Rswup")
    got = F.runmicro(mp, 0.05, vegp, soilc, dtm, out=[1 if n in names else 0 for n in _abi.OUT_NAMES])
    ref, f = tmp_path / "ref.nc", tmp_path / "f.nc"
    ncsink.writetonc(dict(got, tme=w["obstime"]), ref, ext, 0.05, names)
    assert F.runmicro_nc(mp, 0.05, vegp, soilc, dtm, f, vars=names, days_per_chunk=2) == names
    same_file(f, ref, "frontend.runmicro_nc")
    F.runmicro_nc(mp, 0.05, vegp, soilc, dtm, f, vars=names, devices=[0, 0], n_blocks=3)
    same_file(f, ref, "frontend.runmicro_nc, three blocks")
    depths = (-0.05, -0.2)
    mpb = F.runpointmodel(w, depths[0], dtm, vegp, soilc)
    full = F.runmicro_depths(mpb, depths, vegp, soilc, dtm)
    files = [tmp_path / "d0.nc", tmp_path / "d1.nc"]
    F.runmicro_depths_nc(mpb, depths, vegp, soilc, dtm, files, days_per_chunk=2)
    for d in range(2):
        ncsink.writetonc(dict(Tz=full["Tz"][d], soilm=full["soilm"], tme=w["obstime"]), ref, ext, depths[d], ("Tz", "soilm"))
        same_file(files[d], ref, f"frontend.runmicro_depths_nc, depth {depths[d]}")


def test_9c_front_end_runmicro_snow_nc_and_runsnowmodel_nc(tmp_path):
    F, weather, vegp, soilc, dtm = bundled_snow()
    ext = F.nc_extent(dtm, 50, 50)
    mp = F.runpointmodel(weather, 0.05, dtm, vegp, soilc)
    sin = F.runsnowmodel(weather, mp, vegp, soilc, dtm, inputs_only=True)
    names = ("Tz", "relhum")
    arrays = F.runmicro_snow(mp, 0.05, vegp, soilc, dtm, None, one_call=True, snow_inputs=sin,
                             out=[1 if n in names else 0 for n in _abi.OUT_NAMES])
    smod = F.runsnowmodel(weather, mp, vegp, soilc, dtm)
    ref, f, g = tmp_path / "ref.nc", tmp_path / "run.nc", tmp_path / "pack.nc"
    ncsink.writetonc(dict(arrays, tme=weather["obstime"]), ref, ext, 0.05, names)
    res = F.runmicro_snow_nc(mp, 0.05, vegp, soilc, dtm, sin, f, snow_fileout=g, vars=names, snow_vars=("totalSWE", "Tg"))
    assert res["vars"] == names and res["snow_vars"] == ("totalSWE", "Tg") and res["snowdays"].sum() > 0 and res["nosnowdays"].sum() > 0
    same_file(f, ref, "frontend.runmicro_snow_nc")
    _, got = records(g, 50, 50, 2, 288)
    assert np.array_equal(got[:, 0], pack(smod["Tg"], 100)) and np.array_equal(got[:, 1], pack(smod["totalSWE"], 100))
    h = tmp_path / "alone.nc"
    assert F.runsnowmodel_nc(weather, mp, vegp, soilc, dtm, h) == SERIES
    check_snowpack_file(h, smod, weather["obstime"], "frontend.runsnowmodel_nc")
    with pytest.raises(ValueError, match="reqhgt >= 0"):
        F.runmicro_snow_nc(mp, -0.1, vegp, soilc, dtm, sin, f)
