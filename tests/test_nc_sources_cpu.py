"""netCDF sink: further sources, CPU side (include/mcf.h "netCDF sink: further sources"): the new entries exist beside an
unchanged ABI, every refusal that needs no device comes before one is touched with the entry's name at the start of the message,
row strips written by several threads in any order give the bytes of the whole-raster write with every time word in place, and the
file layer's stand-alone harness runs clean under AddressSanitizer + UBSan as a plain program."""
import ctypes as C
import filecmp
import re
import shutil
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

import stages_cases as SC
from microclimf_amd import _abi, api, ncsink
from microclimf_amd import snow as S

ROOT = Path(__file__).resolve().parents[1]
NEW = ("mcf_nc_write_plan_rows", "mcf_nc_write_missing", "mcf_nc_write_host_rows", "mcf_runmicro_nc", "mcf_runmicro_depths_nc",
       "mcf_nc_create_snowpack", "mcf_snowplan_nc_write", "mcf_snowmodel1_nc", "mcf_nc_write_planes", "mcf_snowrun_nc_enable",
       "mcf_runmicrosnow_nc", "mcf_snowrun_drop_days")
ARGS = ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp", "Smaxp", "tfact", "complete", "mat")
E_ARG = 1
GRID = dict(xmin=0.0, xmax=float(SC.COLS), ymin=0.0, ymax=float(SC.ROWS), res=1.0, crs="wkt")


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def test_new_entries_are_declared_exported_and_bound(tmp_path):
    lib = _lib()
    hdr = (ROOT / "include" / "mcf.h").read_text()
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert getattr(lib, n).argtypes is not None, n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION and "#define MCF_ABI_VERSION 8" in hdr
    assert "netCDF sink: further sources" in hdr
    # the new struct against the compiled header; mcf_nc_spec as it was
    fields = ["rows", "cols", "nsteps", "east", "north", "time_hours", "crs_wkt", "series", "scale", "units", "long_name", "format",
              "deflate_level"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcf.h"', 'int main(void) {',
           'printf("size %zu\\n", sizeof(mcf_ncpack_spec));', 'printf("ncspec %zu\\n", sizeof(mcf_nc_spec));']
    src += [f'printf("{f} %zu\\n", offsetof(mcf_ncpack_spec, {f}));' for f in fields] + ['return 0; }']
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split("\n") if line)
    assert int(got["size"]) == C.sizeof(_abi.NcPackSpec) and int(got["ncspec"]) == C.sizeof(_abi.NcSpec) == 112
    for f in fields:
        assert int(got[f]) == getattr(_abi.NcPackSpec, f).offset, f


# ---- refusals that need no device: MCF_ERR_ARG, not "no HIP device" ------------------------------------------------------------
def _args(**over):
    a = dict(SC.build("s170_h005"), **over)
    return {k: a[k] for k in ARGS}


def _below(**over):
    a = _args(reqhgt=-0.1, **over)
    a["pointm"] = dict(a["pointm"])
    return a


def _refused(msg, call):
    with pytest.raises(_abi.McfError, match=r"error 1: " + msg) as ei:
        call()
    assert "no HIP device" not in str(ei.value)


def test_runmicro_nc_refuses_before_a_device(tmp_path):
    lib = _lib()
    f = tmp_path / "x.nc"
    _refused(r"mcf_runmicro_nc: writetonc defines no variable 'tleaf' at this reqhgt",
             lambda: api.runmicro_nc(**_args(reqhgt=0.0), fileout=f, grid=GRID, vars=("Tz", "tleaf")))
    _refused(r"mcf_runmicro_nc: writetonc defines no variable 'Rswup' at this reqhgt",
             lambda: api.runmicro_nc(**_below(), fileout=f, grid=GRID, vars=("Tz", "Rswup")))
    _refused(r"mcf_runmicro_nc: the netCDF-4 container .* one block",
             lambda: api.runmicro_nc(**_args(), fileout=f, grid=GRID, vars=("Tz",), format="netcdf4", devices=[0, 0], n_blocks=3))
    _refused(r"mcf_runmicro_nc: no variable selected", lambda: api.runmicro_nc(**_args(), fileout=f, grid=GRID, vars=()))
    # a spec that disagrees with the inputs: every field by name
    m = api.marshal(*_args().values(), [1] + [0] * 9, False)
    hours, east, north, crs = ncsink.grid_of(GRID, SC.build("s170_h005")["obstime"])
    for field, kw in (("rows", dict(rows=SC.ROWS + 1, north=np.arange(SC.ROWS + 1.0))), ("cols", dict(cols=SC.COLS - 1, east=east[:-1])),
                      ("nsteps", dict(time_hours=hours[:-1])), ("reqhgt", dict(reqhgt=0.1))):
        k = dict(dict(rows=SC.ROWS, cols=SC.COLS, time_hours=hours, east=east, north=north, reqhgt=0.05), **kw)
        sp, _ = ncsink.nc_spec(k["rows"], k["cols"], k["time_hours"], k["east"], k["north"], k["reqhgt"], ("Tz",))
        assert lib.mcf_runmicro_nc(C.byref(m.inputs), C.byref(m.options), None, str(f).encode(), C.byref(sp)) == E_ARG, field
        assert re.match(rb"mcf_runmicro_nc: " + field.encode() + rb" of the mcf_nc_spec", lib.mcf_last_error()), lib.mcf_last_error()
    sp, _ = ncsink.nc_spec(SC.ROWS, SC.COLS, hours, east, north, 0.05, ("Tz",))
    for call in (lambda: lib.mcf_runmicro_nc(None, C.byref(m.options), None, b"x", C.byref(sp)),
                 lambda: lib.mcf_runmicro_nc(C.byref(m.inputs), None, None, b"x", C.byref(sp)),
                 lambda: lib.mcf_runmicro_nc(C.byref(m.inputs), C.byref(m.options), None, None, C.byref(sp)),
                 lambda: lib.mcf_runmicro_nc(C.byref(m.inputs), C.byref(m.options), None, b"x", None)):
        assert call() == E_ARG and lib.mcf_last_error().startswith(b"mcf_runmicro_nc: null"), lib.mcf_last_error()
    assert not f.exists()      # no file is made for a run that is refused


def test_runmicro_depths_nc_refuses_before_a_device(tmp_path):
    lib = _lib()
    a = {k: v for k, v in _below().items() if k != "reqhgt"}
    T = len(a["obstime"]["year"])
    f = [tmp_path / "a.nc", tmp_path / "b.nc"]
    # the refusals of mcf_plan_below_set_depths that need no plan, under this entry's name
    _refused(r"mcf_runmicro_depths_nc: ", lambda: api.runmicro_depths_nc(**dict(a, complete=True), depths=[-0.1, 0.0], files=f, grid=GRID))
    _refused(r"mcf_runmicro_depths_nc: ", lambda: api.runmicro_depths_nc(**dict(a, complete=True), depths=[-0.1, float("nan")], files=f, grid=GRID))
    _refused(r"mcf_runmicro_depths_nc: ", lambda: api.runmicro_depths_nc(**dict(a, complete=False), depths=[-0.1, -0.2], files=f, grid=GRID))      # null tbp
    _refused(r"mcf_runmicro_depths_nc: ", lambda: api.runmicro_depths_nc(**dict(a, complete=True), depths=[-0.1] * 9, files=[f[0]] * 9, grid=GRID))
    _refused(r"mcf_runmicro_depths_nc: ", lambda: api.runmicro_depths_nc(**dict(a, complete=True), depths=[], files=[], grid=GRID))
    m = api.marshal(*_below(complete=True).values(), [1, 0, 0, 1] + [0] * 6, False)
    hours, east, north, crs = ncsink.grid_of(GRID, a["obstime"])
    d = np.array([-0.1, -0.3])
    dp = d.ctypes.data_as(_abi.c_double_p)
    paths = (C.c_char_p * 2)(str(f[0]).encode(), str(f[1]).encode())
    sp, _ = ncsink.nc_spec(SC.ROWS, SC.COLS, hours, east, north, -0.1, ("soilm",))
    assert lib.mcf_runmicro_depths_nc(C.byref(m.inputs), C.byref(m.options), dp, 2, None, paths, C.byref(sp)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_depths_nc: a file per depth holds Tz")
    sp, _ = ncsink.nc_spec(SC.ROWS, SC.COLS, hours[:-1], east, north, -0.1, ("Tz",))
    assert lib.mcf_runmicro_depths_nc(C.byref(m.inputs), C.byref(m.options), dp, 2, None, paths, C.byref(sp)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_depths_nc: nsteps of the mcf_nc_spec")
    paths[1] = None
    sp, _ = ncsink.nc_spec(SC.ROWS, SC.COLS, hours, east, north, -0.1, ("Tz",))
    assert lib.mcf_runmicro_depths_nc(C.byref(m.inputs), C.byref(m.options), dp, 2, None, paths, C.byref(sp)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_depths_nc: paths[1] is null")
    assert lib.mcf_runmicro_depths_nc(C.byref(m.inputs), C.byref(m.options), dp, 2, None, None, C.byref(sp)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_depths_nc: null")
    assert T > 24 and not f[0].exists() and not f[1].exists()


def test_snowmodel1_nc_and_the_plan_entries_refuse_before_a_device(tmp_path, monkeypatch):
    lib = _lib()
    from microclimf_amd import synthetic
    rows, cols, T = 6, 5, 120
    sw = synthetic.snow_workload(rows, cols, T, cold=0.0, zref=3.5, start_doy=90)
    _, _, dtm = synthetic.rasters(rows, cols)
    args = (sw["obstime"], sw["climdata"], sw["pointm"], sw["vegp"], sw["other"], sw["snowenv"], dtm, 1.0, 0.02)
    f = tmp_path / "p.nc"
    grid = dict(xmin=0.0, xmax=float(cols), ymin=0.0, ymax=float(rows), res=1.0)
    _refused(r"mcf_snowmodel1_nc: the netCDF-4 container .* one block",
             lambda: S.snowmodel1_nc(*args, fileout=f, grid=grid, format="netcdf4", devices=[0, 0], n_blocks=3))
    with pytest.raises(ValueError, match="east / north"):
        S.snowmodel1_nc(*args, fileout=f, grid=dict(grid, xmax=cols + 1.0))
    orig = ncsink.ncpack_spec

    def one_step_short(*a, **k):
        sp, names = orig(*a, **k)
        sp.nsteps -= 1
        return sp, names
    monkeypatch.setattr(ncsink, "ncpack_spec", one_step_short)
    _refused(r"mcf_snowmodel1_nc: nsteps of the mcf_ncpack_spec", lambda: S.snowmodel1_nc(*args, fileout=f, grid=grid))
    monkeypatch.undo()
    assert lib.mcf_snowmodel1_nc(None, None, b"x", None) == E_ARG and lib.mcf_last_error().startswith(b"mcf_snowmodel1_nc: null")
    assert not f.exists()
    for call, name in ((lambda: lib.mcf_nc_write_plan_rows(None, None, 0, 0, 0, 0, 0, 0, None), b""),
                       (lambda: lib.mcf_snowplan_nc_write(None, None, 0, 0), b"mcf_snowplan_nc_write"),
                       (lambda: lib.mcf_nc_write_planes(None, None, 1, 0, 0, 0, 0, None), b"mcf_nc_write_planes"),
                       (lambda: lib.mcf_nc_write_missing(None, 0, 1, 0, 0), b"mcf_nc_write_missing"),
                       (lambda: lib.mcf_nc_write_host_rows(None, 0, 1, 0, 0, None), b"mcf_nc_write_host_rows"),
                       (lambda: lib.mcf_nc_create_snowpack(None, None, None), b"mcf_nc_create_snowpack")):
        assert call() == E_ARG and lib.mcf_last_error().startswith(name) and b"null" in lib.mcf_last_error(), name


# ---- the file side of row strips ------------------------------------------------------------------------------------------------
def _values(rows, cols, T, rng):
    x = np.asfortranarray(np.round(rng.normal(size=(rows, cols, T)) * 30, 3))
    x[1, 2, 0] = np.nan
    x[0, 0, T - 1] = 0.125          # a tie at .5 after x 100
    return x


def test_three_strips_written_in_descending_order_by_three_threads_equal_the_whole_write(tmp_path):
    _lib()
    rows, cols, T = 5, 7, 3
    rng = np.random.default_rng(5)
    hours, east, north = 400000.0 + np.arange(T), np.arange(cols) + 0.5, np.arange(rows) + 0.5
    tz, sm = _values(rows, cols, T, rng), _values(rows, cols, T, rng)
    miss = (slice(3, 5), slice(None), slice(2, 3))      # the last strip's last step is never computed: missval
    tz[miss] = sm[miss] = np.nan
    whole, strips = tmp_path / "whole.nc", tmp_path / "strips.nc"
    with ncsink.NcWriter(whole, rows, cols, hours, east, north, 0.0, ("Tz", "soilm"), "wkt") as w:
        w.write_host(0, {"Tz": tz, "soilm": sm})
    cuts = [(3, 5), (1, 3), (0, 1)]      # descending
    errs = []
    with ncsink.NcWriter(strips, rows, cols, hours, east, north, 0.0, ("Tz", "soilm"), "wkt") as w:
        def block(r0, r1):
            try:
                n = 2 if r0 == 3 else T
                w.write_host_rows(r0, 1, {"Tz": tz[r0:r1, :, 1:n], "soilm": sm[r0:r1, :, 1:n]})      # the later steps first
                w.write_host_rows(r0, 0, {"Tz": tz[r0:r1, :, :1], "soilm": sm[r0:r1, :, :1]})
                if r0 == 3:
                    w.write_missing(r0, r1 - r0, 2, 1)
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=block, args=c) for c in cuts]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        # a strip or a step range outside the file
        for bad in (lambda: w.write_missing(4, 2, 0, 1), lambda: w.write_missing(0, 0, 0, 1), lambda: w.write_missing(0, 1, 3, 1),
                    lambda: w.write_host_rows(4, 0, {"Tz": tz[:2], "soilm": sm[:2]})):
            with pytest.raises(_abi.McfError, match="error 1: mcf_nc_write_(missing|host_rows): "):
                bad()
    assert filecmp.cmp(whole, strips, shallow=False)
    # the time words are in the file: read back with the classic reader of tests/test_ncsink_cpu.py's kind
    raw = strips.read_bytes()
    rec_bytes = 8 + 2 * rows * cols * 4
    begin = len(raw) - T * rec_bytes
    assert [np.frombuffer(raw, ">f8", 1, begin + k * rec_bytes)[0] for k in range(T)] == list(hours)
    vals = np.frombuffer(raw, ">i4", rows * cols, begin + 8).reshape(rows, cols)
    want = np.where(np.isnan(tz[:, :, 0]), -9999, np.rint(tz[:, :, 0] * 100)).astype(np.int32)
    assert np.array_equal(vals, want)


def test_netcdf4_takes_no_row_strip(tmp_path):
    import h5mini
    _lib()
    if h5mini.load() is None:
        pytest.skip("no HDF5 library on this host")
    rows, cols, T = 5, 7, 2
    x = np.zeros((rows, cols, T))
    with ncsink.NcWriter(tmp_path / "x.nc", rows, cols, np.arange(T) + 1.0, np.arange(cols) + 0.5, np.arange(rows) + 0.5, 0.0, ("Tz",),
                         format="netcdf4") as w:
        with pytest.raises(_abi.McfError, match="error 1: mcf_nc_write_missing: the netCDF-4 container .* not a row strip"):
            w.write_missing(0, 2, 0, 1)
        with pytest.raises(_abi.McfError, match="error 1: mcf_nc_write_host_rows: the netCDF-4 container .* not a row strip"):
            w.write_host_rows(2, 0, {"Tz": x[2:]})
        w.write_host_rows(0, 0, {"Tz": x})      # one block: the whole raster, as before
        w.write_missing(0, rows, 1, 1)


def test_snowpack_file_header_carries_the_table(tmp_path):
    _lib()
    rows, cols, T = 3, 4, 2
    f = tmp_path / "pack.nc"
    w = ncsink.SnowpackNcWriter(f, rows, cols, np.arange(T) + 1.0, np.arange(cols) + 0.5, np.arange(rows) + 0.5,
                                vars=("totalSWE", "Tc", "groundsnowdepth"), units={"Tc": "centi deg C"})
    assert w.vars == ("Tc", "groundsnowdepth", "totalSWE")      # the file's order: mcf_snowdriver_out's
    w.write_missing(0, rows, 0, T)
    w.close()
    raw = f.read_bytes()
    for text in (b"Tc", b"groundsnowdepth", b"totalSWE", b"centi deg C", b"mm x 100", b"Ground snow depth", b"Total snow water equivalent"):
        assert text in raw, text
    assert b"snowden" not in raw and b"Tg" not in raw
    assert len(raw) % 4 == 0 and np.all(np.frombuffer(raw, ">i4", rows * cols * 3, len(raw) - rows * cols * 12) == -9999)
    with pytest.raises(_abi.McfError, match="error 1: mcf_nc_create_snowpack: no series selected"):
        ncsink.SnowpackNcWriter(f, rows, cols, np.arange(T) + 1.0, np.arange(cols) + 0.5, np.arange(rows) + 0.5, vars=())


def test_strips_harness_is_clean_under_asan_and_ubsan(tmp_path):
    """tools/harness/nc_strips_harness.cpp as a plain program of its own (nothing is loaded into this interpreter)"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "nc_strips_asan"
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-I", str(ROOT / "microclimf_amd" / "csrc"), "-I", str(ROOT / "include"), "-pthread",
                    "-o", str(exe), str(ROOT / "tools" / "harness" / "nc_strips_harness.cpp")], check=True)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "37x29x5 in 4 strips ok" in r.stdout, r.stdout + r.stderr


def test_runmicrosnow_nc_refuses_before_a_device(tmp_path):
    lib = _lib()
    from microclimf_amd import synthetic
    rows, cols, T = 6, 5, 120
    sw = synthetic.snow_workload(rows, cols, T, cold=0.0, zref=3.5, start_doy=90)
    a = synthetic.workload(rows, cols, T, reqhgt=0.05, zref=3.5, hgt_range=(0.05, 3.0), start_doy=90, variety=True)
    _, _, dtm = synthetic.rasters(rows, cols)
    snow = dict(sw, dtm=dtm, res=1.0, tfact=0.02)
    micro = {"obstime": sw["obstime"], "climdata": sw["climdata"], "vegp": sw["vegp"], "other": sw["other"]}
    grid = dict(xmin=0.0, xmax=float(cols), ymin=0.0, ymax=float(rows), res=1.0)
    f, g = tmp_path / "m.nc", tmp_path / "p.nc"
    _refused(r"mcf_runmicrosnow_nc: the netCDF-4 container .* one block",
             lambda: S.runmicrosnow_nc(a, snow, micro, 7.5, fileout=f, nc_grid=grid, format="netcdf4", devices=[0, 0], n_blocks=3))
    _refused(r"mcf_runmicrosnow_nc: the netCDF-4 container .* one block",
             lambda: S.runmicrosnow_nc(a, snow, micro, 7.5, pack_fileout=g, nc_grid=grid, format="netcdf4", devices=[0, 0], n_blocks=3))
    _refused(r"mcf_runmicrosnow_nc: a variable of the mcf_nc_spec is not among the run's",
             lambda: S.runmicrosnow_nc(dict(a, out=[1] + [0] * 9), snow, micro, 7.5, fileout=f, nc_grid=grid, vars=("Tz", "relhum")))
    a0 = synthetic.workload(rows, cols, T, reqhgt=0.0, zref=3.5, hgt_range=(0.05, 3.0), start_doy=90, variety=True)
    _refused(r"mcf_runmicrosnow_nc: writetonc defines no variable 'relhum' at this reqhgt",
             lambda: S.runmicrosnow_nc(a0, snow, micro, 7.5, fileout=f, nc_grid=grid, vars=("Tz", "relhum")))
    _refused(r"mcf_runmicrosnow_nc: no series selected", lambda: S.runmicrosnow_nc(a, snow, micro, 7.5, pack_fileout=g, nc_grid=grid, pack_vars=()))
    _refused(r"mcf_runmicrosnow_nc: null path / spec", lambda: S.runmicrosnow_nc(a, snow, micro, 7.5, nc_grid=grid))
    _refused(r"mcf_runmicrosnow_nc: .*shape", lambda: S.runmicrosnow_nc(dict(a, obstime={k: v[:96] for k, v in a["obstime"].items()},
                                                                               climdata={k: v[:96] for k, v in a["climdata"].items()},
                                                                               pointm={k: v[:96] for k, v in a["pointm"].items()}),
                                                                          snow, micro, 7.5, fileout=f, nc_grid=grid))
    assert lib.mcf_runmicrosnow_nc(None, None, None, b"x", None, None, None, None) == E_ARG and lib.mcf_last_error().startswith(b"mcf_runmicrosnow_nc: null")
    assert lib.mcf_snowrun_nc_enable(None, None, None) == E_ARG and lib.mcf_last_error().startswith(b"mcf_snowrun_nc_enable: null")
    assert lib.mcf_snowrun_drop_days(None, None, 0) == E_ARG and lib.mcf_last_error().startswith(b"mcf_snowrun_drop_days: null")
    assert not f.exists() and not g.exists()
