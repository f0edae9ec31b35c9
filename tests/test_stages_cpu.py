"""The staged model's diagnostics, CPU side: the yardstick (tests/stages_ref.c) is tied to the unchanged oracle, obeys the
reference's identities, gives bars that see a single-precision slip; the cases hold the cell mix they promise; the C ABI's
new entries exist, check their arguments and need a device."""
import ctypes as C

import numpy as np
import pytest

import parity_bars as PB
import stages_cases as SC
import stages_ref as SR
from microclimf_amd import _abi


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("name", SC.CASES)
def test_each_case_holds_the_promised_cell_mix(name):
    """from the inputs alone: an NA cell, a bare cell, a cell with reqhgt above the canopy and one below it (in every layer),
    and NA / bare cells outside the first tile as well as inside the raster's partial last tile or a full one"""
    a = SC.build(name)
    hgt, pai = np.asarray(a["vegp"]["hgt"]), np.asarray(a["vegp"]["pai"])
    if hgt.ndim == 2:
        hgt, pai = hgt[:, :, None], pai[:, :, None]
    assert hgt.shape[:2] == (SC.ROWS, SC.COLS) and len(a["obstime"]["year"]) == SC.TSTEPS
    assert SC.ROWS * SC.COLS == 2 * 21 + 8 and SC.TSTEPS // 24 == 4
    valid = ~np.isnan(hgt[:, :, 0])
    assert (~valid).sum() >= 1
    for l in range(hgt.shape[2]):
        h, p = hgt[:, :, l], pai[:, :, l]
        assert (valid & (p == 0)).sum() >= 1
        assert (valid & (a["reqhgt"] >= h)).sum() >= 1
        assert (valid & (a["reqhgt"] < h)).sum() >= 1
    if name == "layered":
        assert list(a["dfsel"]["st"]) == [0, 48] and list(a["dfsel"]["ed"]) == [47, 95]


@pytest.mark.parametrize("name", SC.CASES)
def test_yardstick_is_tied_to_the_oracle(oracle, name):
    """what the yardstick shares with orc_run_grid it gives bit for bit"""
    a = SC.build(name)
    got = SR.run(a)
    want = oracle.run_grid(**a)
    for mine, theirs in (("Rbdown", "Rdirdown"), ("Rddown", "Rdifdown"), ("Rdup", "Rswup"), ("uz", "windspeed"), ("soilm", "soilm")):
        assert np.array_equal(bits(got[mine]), bits(want[theirs])), (mine, theirs)
    # nothing in the ground temperature depends on reqhgt: T0 is Tz of the same run at reqhgt = 0.  (uz does depend on it, but
    # soiltempG0 / soiltemp_hr take uf's conductance gHa, not uz.)  The vegetation inputs must be the same ones: paia is the
    # foliage above reqhgt, which the ground never sees either.
    ground = oracle.run_grid(**dict(a, reqhgt=0.0))
    assert np.array_equal(bits(got["T0"]), bits(ground["Tz"]))


@pytest.mark.parametrize("name", SC.CASES)
def test_yardstick_identities(name):
    a = SC.build(name)
    r = SR.run(a)
    hgt, pai = np.asarray(a["vegp"]["hgt"]), np.asarray(a["vegp"]["pai"])
    valid = ~np.isnan(hgt if hgt.ndim == 2 else hgt[:, :, 0])
    for k, v in r.items():          # NA cells carry R's NA_real_, every other cell-step is a number
        assert (bits(v[~valid]) == PB.NA_BITS).all(), k
        assert np.isfinite(v[valid]).all(), k
    night = np.asarray(a["climdata"]["swdown"]) == 0
    assert night.any() and (~night).any()
    assert (r["radGsw"][valid][:, night] == 0).all()
    assert (r["radLsw"][valid][:, night] == 0).all() and (r["radLpar"][valid][:, night] == 0).all()
    if pai.ndim == 2:
        bare = valid & (pai == 0)
        assert np.array_equal(bits(r["radCsw"][bare]), bits(r["radGsw"][bare]))
        assert np.array_equal(bits(r["radClw"][bare]), bits(r["radGlw"][bare]))
        assert (r["radLsw"][bare] == 0).all() and (r["radLpar"][bare] == 0).all()
        assert (r["radLsw"][valid & (pai > 0)][:, ~night] > 0).any()
    lw = r["lwout"][valid]
    assert (bits(lw) == bits(lw[:1])).all()          # one value per step
    assert (r["uf"][valid] >= 0.001).all() and (r["gHa"][valid] >= 0.0001).all() and (r["kDDg"][valid] > 0).all()


def test_bars_stay_100x_below_the_exp32_slip():
    """as tests/test_parity_bars_cpu.py asks of the ten outputs: the single-precision exp lies >= 100 bars from the yardstick
    in at least one diagnostic, for the midsummer case (every derived bar is at most the 1e-6 cap by construction)"""
    a = SC.build("s170_h005")
    want, bars, noise = SR.bars_for("s170_h005", a)
    slip = SR.run(a, "exp32")
    ratio = {k: PB.distance(slip[k], want[k]) / bars[k] for k in _abi.DIAG_NAMES if PB.same_pattern(slip[k], want[k])}
    assert all(PB.FLOOR <= bars[k] <= PB.CAP for k in want)
    assert max(ratio.values()) >= 100.0, ratio
    # ... and the variables exp feeds directly each see it
    for k in ("radGsw", "radGlw", "T0"):
        assert ratio[k] >= 100.0, (k, ratio[k], bars[k], noise[k])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


NEW = ("mcf_plan_diag_enable", "mcf_plan_diag_fetch", "mcf_plan_diag_slot_ptr", "mcf_plan_diag_ring_layout",
       "mcf_runmicro1_diag", "mcf_runmicro3_diag")


def test_new_symbols_and_unchanged_abi():
    lib = _lib()
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION
    assert _abi.NDIAG == 13 == len(_abi.DIAG_NAMES)
    # the existing structs as they were (LP64)
    assert C.sizeof(_abi.GridInputs) == 3 * 8 + 8 + (4 + 10 + 8 + 10 + 15) * 8 + 2 * 8 + 2 * 8 + 2 * 8 + 8 + 4 * 8 + 8 + 2 * 8 + 8
    assert C.sizeof(_abi.Options) == 6 * 8 + 4 + 40 + 3 * 4
    assert C.sizeof(_abi.Outputs) == 80
    assert C.sizeof(_abi.RingLayout) == 4 * 4 + 3 * 8
    assert C.sizeof(_abi.DiagOutputs) == 13 * 8


def test_header_enum_matches_the_names():
    import re
    from pathlib import Path
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    body = re.search(r"enum mcf_diag \{(.*?)\};", hdr, re.S).group(1)
    found = re.findall(r"MCF_DIAG_\w+ = (\d+),\s*/\* \"(\w+)\"", body)
    assert [n for _, n in found] == list(_abi.DIAG_NAMES) and [int(i) for i, _ in found] == list(range(13))
    assert "MCF_NDIAG = 13" in body


def test_null_arguments_are_refused():
    lib = _lib()
    sel = (C.c_int32 * 13)(*[1] * 13)
    q = C.c_void_p()
    lay = _abi.RingLayout()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(_abi.c_double_p)
    E = 1   # MCF_ERR_ARG
    assert lib.mcf_plan_diag_enable(None, C.byref(sel)) == E
    assert b"null" in lib.mcf_last_error()
    assert lib.mcf_plan_diag_fetch(None, 0, 0, 0, 1, p) == E
    assert lib.mcf_plan_diag_slot_ptr(None, 0, 0, C.byref(q)) == E
    assert lib.mcf_plan_diag_ring_layout(None, C.byref(lay)) == E
    from microclimf_amd.marshal import alloc_outputs, marshal
    a = SC.build("s170_h005")
    m = marshal(*[a[k] for k in ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp",
                                 "Smaxp", "tfact", "complete", "mat", "out")], False)
    outs, _ = alloc_outputs(m)
    dout = _abi.DiagOutputs()
    for fn in (lib.mcf_runmicro1_diag, lib.mcf_runmicro3_diag):
        assert fn(C.byref(m.inputs), C.byref(m.options), None, C.byref(outs), C.byref(dout)) == E
        assert fn(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs), None) == E
        assert fn(None, C.byref(m.options), C.byref(sel), C.byref(outs), C.byref(dout)) == E
    # a selected diagnostic without a buffer, an empty selection, reqhgt < 0: refused before any device is touched
    assert lib.mcf_runmicro1_diag(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs), C.byref(dout)) == E
    assert b"null buffer" in lib.mcf_last_error()
    none = (C.c_int32 * 13)()
    assert lib.mcf_runmicro1_diag(C.byref(m.inputs), C.byref(m.options), C.byref(none), C.byref(outs), C.byref(dout)) == E
    assert b"no diagnostic" in lib.mcf_last_error()
    m.options.reqhgt = -0.05
    assert lib.mcf_runmicro1_diag(C.byref(m.inputs), C.byref(m.options), C.byref(sel), C.byref(outs), C.byref(dout)) == E
    assert b"reqhgt >= 0" in lib.mcf_last_error()


def test_one_shot_needs_a_device():
    """no CPU fallback: MCF_ERR_NO_DEVICE where there is none (on a GPU host the entry is covered by tests/test_stages_gpu.py)"""
    lib = _lib()
    from microclimf_amd.api import runmicro1Cpp
    a = SC.build("s170_h005")
    if lib.mcf_device_count() > 0:
        got = runmicro1Cpp(**a, diag=["radGsw"])
        assert list(got["diag"]) == ["radGsw"]
        return
    with pytest.raises(_abi.McfError, match="no HIP device"):
        runmicro1Cpp(**a, diag="all")
    assert "no HIP device" in lib.mcf_last_error().decode()


def test_stage_map_fixture_holds_what_the_map_test_expects():
    """tests/golden/vignette_stage_maps.json (tools/digitize_vignette.py --stage-maps): image3's two panels, 50 x 50 cells, the
    128 NA cells of the bundled site's no-data block, class widths of about 2 W/m2 (short wave) and 0.56 W/m2 (long wave)"""
    import json
    from pathlib import Path
    import vignette_fixture as V
    fig = json.loads((Path(__file__).resolve().parent / "golden" / "vignette_stage_maps.json").read_text())["maps"]["image3"]
    assert fig["source"] == "vignettes/images/image3.png" and len(fig["panels"]) == 2
    sibling = np.isnan(V.map_panel("image3b", 0)["lo"])
    for p, (lo, hi), width in zip(fig["panels"], ((0, 800), (190, 420)), (2.04, 0.559)):
        cells = np.array(p["cells"])
        assert cells.shape == (50, 50) and (cells < 0).sum() == 128
        assert np.array_equal(cells < 0, sibling)          # the same no-data block as the sibling figure of the same run
        cls = np.array(p["classes"])
        assert cells.max() < len(cls) and ((np.diff(cls[:, 0]) < 0).all() or (np.diff(cls[:, 0]) > 0).all())
        assert lo <= cls.min() and cls.max() <= hi
        assert abs(np.median(cls[:, 1] - cls[:, 0]) - width) < 0.01 * width + 0.005
        assert p["legend"]["fit_resid_px"] <= 0.75
