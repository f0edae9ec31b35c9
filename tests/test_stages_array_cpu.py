"""The staged model's diagnostics for array weather, CPU side: the yardstick (tests/stages_ref_array.c) is tied to the unchanged
oracle's array-forcing driver, the cases hold the cell mix and the geometry they promise, and the C ABI's new entries exist,
check their arguments and need a device."""
import ctypes as C

import numpy as np
import pytest

import parity_bars as PB
import stages_array_cases as AC
import stages_ref_array as SRA
from microclimf_amd import _abi


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("name", AC.CASES)
def test_each_case_holds_what_it_promises(name):
    c = AC.build(name)
    hgt, pai = np.asarray(c.a["vegp"]["hgt"]), np.asarray(c.a["vegp"]["pai"])
    if hgt.ndim == 2:
        hgt, pai = hgt[:, :, None], pai[:, :, None]
    valid = ~np.isnan(hgt[:, :, 0])
    assert (~valid).sum() >= 1 and c.tsteps == 24 * c.ndays
    for l in range(hgt.shape[2]):
        assert (valid & (pai[:, :, l] == 0)).sum() >= 1
    n = c.rows * c.cols
    assert n > 32 and n % 32 != 0                    # more than one 32-cell tile, and a partial last one
    if name in AC.FINE:
        assert (c.rows, c.cols, c.ndays) == (5, 10, 4) and c.full is c.a and c.coarse is None
        assert np.shape(c.a["climdata"]["tc"]) == (5, 10, 96) and np.shape(c.a["lat"]) == (5, 10)
    else:
        rp = c.coarse["rowpos"]
        cr, cc = np.shape(c.a["climdata"]["temp"])[:2]
        assert (cr, cc) == ((3, 2) if name == "c_lds" else (2, 3))
        assert np.shape(c.full["climdata"]["tc"]) == (c.rows, c.cols, c.tsteps)
        # the staged taps' precondition (rows >= 32, row positions that do not decrease, <= 4 coarse rows per 32-cell window)
        lds = c.rows >= 32 and (np.diff(rp) >= 0).all() and \
            all(np.floor(rp[min(i + 31, c.rows - 1)]) - np.floor(rp[i]) + 2 <= 4 for i in range(c.rows))
        assert lds == (name == "c_lds")
        assert (c.coarse.get("altcorrect", 0) != 0) == name.startswith("c_alt")
        if "dtmc" in c.coarse:
            assert np.isnan(c.coarse["dtmc"]).sum() == 1 and np.ptp(c.coarse["dtm"][valid]) > 50.0
    if name == "alayered":
        assert list(c.a["dfsel"]["st"]) == [0, 48] and list(c.a["dfsel"]["ed"]) == [47, 95]
    night = np.asarray(c.full["climdata"]["swdown"]) == 0
    assert night.any() and (~night).any()


@pytest.mark.parametrize("name", AC.CASES)
def test_yardstick_is_tied_to_the_oracle(oracle, name):
    """what the yardstick shares with orc_run_grid's array-forcing branch it gives bit for bit, and T0 is that oracle's Tz at
    reqhgt = 0 (nothing in the ground temperature depends on reqhgt; the vegetation inputs must be the same ones)"""
    c = AC.build(name)
    got = SRA.run(c.full)
    want = oracle.run_grid(**c.full, array_forcing=True)
    for mine, theirs in (("Rbdown", "Rdirdown"), ("Rddown", "Rdifdown"), ("Rdup", "Rswup"), ("uz", "windspeed"), ("soilm", "soilm")):
        assert np.array_equal(bits(got[mine]), bits(want[theirs])), (mine, theirs)
    ground = oracle.run_grid(**dict(c.full, reqhgt=0.0), array_forcing=True)
    assert np.array_equal(bits(got["T0"]), bits(ground["Tz"]))


@pytest.mark.parametrize("name", ("a170_h005", "alayered", "c_lds", "c_alt2"))
def test_yardstick_identities(name):
    c = AC.build(name)
    r = SRA.run(c.full)
    hgt, pai = np.asarray(c.a["vegp"]["hgt"]), np.asarray(c.a["vegp"]["pai"])
    valid = ~np.isnan(hgt if hgt.ndim == 2 else hgt[:, :, 0])
    for k, v in r.items():          # NA cells carry R's NA_real_, every other cell-step is a number
        assert (bits(v[~valid]) == PB.NA_BITS).all(), k
        assert np.isfinite(v[valid]).all(), k
    night = np.asarray(c.full["climdata"]["swdown"]) == 0          # per cell-step here
    for k in ("radGsw", "radLsw", "radLpar"):
        assert (r[k][night & valid[:, :, None]] == 0).all(), k
    if pai.ndim == 2:
        bare = valid & (pai == 0)
        assert np.array_equal(bits(r["radCsw"][bare]), bits(r["radGsw"][bare]))
        assert (r["radLsw"][bare] == 0).all() and (r["radLpar"][bare] == 0).all()
    # the cells' own weather: lwout differs between cells (one value per step under vector weather)
    lw = r["lwout"][valid]
    assert not (bits(lw) == bits(lw[:1])).all()
    assert (r["uf"][valid] >= 0.001).all() and (r["gHa"][valid] >= 0.0001).all() and (r["kDDg"][valid] > 0).all()


def test_bars_stay_100x_below_the_exp32_slip():
    c = AC.build("a170_h005")
    want, bars, noise = SRA.bars_for("a170_h005", c.full)
    slip = SRA.run(c.full, "exp32")
    ratio = {k: PB.distance(slip[k], want[k]) / bars[k] for k in _abi.DIAG_NAMES if PB.same_pattern(slip[k], want[k])}
    assert all(PB.FLOOR <= bars[k] <= PB.CAP for k in want)
    for k in ("radGsw", "radGlw", "T0"):
        assert ratio[k] >= 100.0, (k, ratio[k], bars[k], noise[k])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


NEW = ("mcf_plan_diag_enable_array", "mcf_runmicro2_diag", "mcf_runmicro4_diag")


def test_new_symbols_and_unchanged_abi():
    import re
    from pathlib import Path
    lib = _lib()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    since = re.search(r"added since, functions only:(.*?)\) \*/", hdr, re.S).group(1)
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
        assert n in since and re.search(r"\bint " + n + r"\(", hdr), n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION
    assert C.sizeof(_abi.DiagOutputs) == 13 * 8


def test_null_arguments_are_refused():
    lib = _lib()
    sel = (C.c_int32 * 13)(*[1] * 13)
    E = 1   # MCF_ERR_ARG
    assert lib.mcf_plan_diag_enable_array(None, C.byref(sel)) == E
    assert b"null" in lib.mcf_last_error()
    from microclimf_amd.marshal import alloc_outputs, marshal
    a = AC.build("a170_h005").a
    m = marshal(*[a[k] for k in AC.ARGS], True)
    outs, _ = alloc_outputs(m)
    dout = _abi.DiagOutputs()
    for fn in (lib.mcf_runmicro2_diag, lib.mcf_runmicro4_diag):
        assert fn(C.byref(m.inputs), C.byref(m.options), None, C.byref(outs), C.byref(dout)) == E
        assert fn(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs), None) == E
        assert fn(None, C.byref(m.options), C.byref(sel), C.byref(outs), C.byref(dout)) == E
    assert lib.mcf_runmicro4_diag(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs), C.byref(dout)) == E
    assert b"veg_layers" in lib.mcf_last_error()
    # a selected diagnostic without a buffer, an empty selection, reqhgt < 0, vector weather: refused before any device is touched
    assert lib.mcf_runmicro2_diag(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs), C.byref(dout)) == E
    assert b"null buffer" in lib.mcf_last_error()
    none = (C.c_int32 * 13)()
    assert lib.mcf_runmicro2_diag(C.byref(m.inputs), C.byref(m.options), C.byref(none), C.byref(outs), C.byref(dout)) == E
    assert b"no diagnostic" in lib.mcf_last_error()
    m.options.reqhgt = -0.05
    assert lib.mcf_runmicro2_diag(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs), C.byref(dout)) == E
    assert b"reqhgt >= 0" in lib.mcf_last_error()
    import stages_cases as SC
    v = SC.build("s170_h005")
    mv = marshal(*[v[k] for k in AC.ARGS], False)
    outs_v, _ = alloc_outputs(mv)
    buf = np.empty((mv.rows, mv.cols, mv.tsteps), order="F")
    for i in range(13):
        dout.var[i] = buf.ctypes.data_as(_abi.c_double_p)
    assert lib.mcf_runmicro2_diag(C.byref(mv.inputs), C.byref(mv.options), C.byref(sel), C.byref(outs_v), C.byref(dout)) == E
    assert b"array_forcing" in lib.mcf_last_error()


def test_one_shot_needs_a_device():
    """no CPU fallback: MCF_ERR_NO_DEVICE where there is none (on a GPU host the entry is covered by tests/test_stages_array_gpu.py)"""
    lib = _lib()
    from microclimf_amd.api import runmicro2Cpp
    a = AC.build("a170_h005").a
    if lib.mcf_device_count() > 0:
        got = runmicro2Cpp(*[a[k] for k in AC.ARGS], diag=["radGsw"])
        assert list(got["diag"]) == ["radGsw"]
        return
    with pytest.raises(_abi.McfError, match="no HIP device"):
        runmicro2Cpp(*[a[k] for k in AC.ARGS], diag="all")


def test_front_end_refusals_without_a_device():
    from microclimf_amd import frontend as F
    with pytest.raises(NotImplementedError, match="array weather.*modelina"):
        F.modelin([{}, {}], {}, {}, {})
    with pytest.raises(ValueError, match="list of micropoints"):
        F.modelina({}, 1, 1, {}, {}, {}, lats=None, lons=None)
    with pytest.raises(ValueError, match="dtmc"):
        F.modelina([{}], 1, 1, {}, {}, {}, lats=None, lons=None, altcorrect=1)
    micro = {"progress": 4, "_array": {}, "_runs": {}}
    with pytest.raises(ValueError, match="coarse array forcing below ground"):
        F.belowground(micro, -0.05)
