"""Host entries of the vegetation pre-compute (mcf_find_lref, mcf_find_gref, mcf_fill_na, mcf_leafrfromalb; mcf_vegprep.cpp)
against the yardstick of tests/vegprep_ref.py, under the parity bar of tests/vegprep_cases.py; the refusals; the R glue's
entry names.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import vegprep_cases as VC
from microclimf_amd import _abi, frontend, vegprep as V

ROOT = Path(__file__).resolve().parent.parent
MCF_ERR_ARG = 1          # include/mcf.h
HOST = (None,)          # the entries whose residual error enters the bar: the host unit's


def test_the_bar_is_made_of_measured_errors():
    e_yard, e_host = VC.residual_errors(None)
    print(f"E yardstick {e_yard:.3e}, E host entry {e_host:.3e}, bar {VC.bar(HOST):.3e}")
    assert 0 < e_yard < 1e-11 and 0 < e_host < 1e-11        # far below tol = 1e-6, or the bar would mean nothing


@pytest.mark.parametrize("which", VC.WHICH)
@pytest.mark.parametrize("name", list(VC.SOLVE_CASES))
def test_solve_equals_the_yardstick(name, which):
    got = VC.check_solve(name, which, None, HOST)
    VC.check_solve_contents(name, which, got)
    # the seeds were chosen so that the yardstick alone flags no cell
    assert VC.solve_reference(name, which)[1].min() >= VC.bar(HOST)


@pytest.mark.parametrize("name", list(VC.FILL_CASES))
def test_fill_equals_the_queue(name):
    VC.check_fill(name, None)


@pytest.mark.parametrize("name", list(VC.FUSED_CASES))
def test_fused_loop_equals_the_yardstick(name):
    VC.check_fused(name, None, HOST)


def test_fused_loop_takes_both_branches_and_several_passes():
    first = {VC.fused_reference(n)["lref_first"] for n in VC.FUSED_CASES}
    assert first == {True, False}
    assert all(VC.fused_reference(n)["iterations"] > 3 for n in VC.FUSED_CASES)


def test_frontend_exports():
    for k in ("find_lref", "find_gref", "fill_na", "leafrfromalb"):
        assert getattr(frontend, k) is getattr(V, k)


def test_python_refusals():
    pai, x, alb = (np.full((4, 3), v) for v in (1.0, 1.0, 0.2))
    with pytest.raises(ValueError, match="single layer"):
        V.leafrfromalb(np.ones((4, 3, 2)), x, alb, device=None)
    with pytest.raises(ValueError, match="must match"):
        V.leafrfromalb(pai, x[:3], alb, device=None)
    with pytest.raises(ValueError, match="must match"):
        V.find_lref(pai, x, x, alb[:, :2], device=None)
    with pytest.raises(ValueError, match="must match"):
        V.fill_na(pai, x.T, device=None)
    with pytest.raises(_abi.McfError, match="holds no value"):
        V.leafrfromalb(np.full((4, 3), np.nan), x, alb, device=None)
    got = V.leafrfromalb(pai[:, :, None], x, alb, device=None)          # one layer is a single layer
    assert got["leafr"].shape == (4, 3)


@pytest.mark.parametrize("suffix,extra", [("", ()), ("_device", (0,))], ids=["host", "device"])
def test_abi_refusals(suffix, extra):
    """null pointers, dimensions below 1 and a non-finite ltrr are refused before anything runs, on the device entries too"""
    lib = _abi.load()
    a = np.ones(6)
    p = a.ctypes.data_as(_abi.c_double_p)
    out = _abi.LeafrOut()
    out.leafr = out.leaft = out.gref = p
    solve = [getattr(lib, "mcf_find_lref" + suffix), getattr(lib, "mcf_find_gref" + suffix)]
    for fn in solve:
        assert fn(3, 2, p, p, p, p, 0.5, None, *extra) == MCF_ERR_ARG
        assert fn(3, 2, None, p, p, p, 0.5, p, *extra) == MCF_ERR_ARG
        assert fn(0, 2, p, p, p, p, 0.5, p, *extra) == MCF_ERR_ARG
        assert fn(3, -1, p, p, p, p, 0.5, p, *extra) == MCF_ERR_ARG
        for bad in (np.nan, np.inf):
            assert fn(3, 2, p, p, p, p, bad, p, *extra) == MCF_ERR_ARG
            assert b"ltrr" in lib.mcf_last_error()
    fill = getattr(lib, "mcf_fill_na" + suffix)
    assert fill(3, 2, p, None, p, *extra) == MCF_ERR_ARG
    assert fill(3, 0, p, p, p, *extra) == MCF_ERR_ARG
    loop = getattr(lib, "mcf_leafrfromalb" + suffix)
    assert loop(3, 2, p, p, p, np.nan, C.byref(out), *extra) == MCF_ERR_ARG
    assert loop(3, 2, p, None, p, 0.5, C.byref(out), *extra) == MCF_ERR_ARG
    assert loop(0, 2, p, p, p, 0.5, C.byref(out), *extra) == MCF_ERR_ARG
    assert loop(3, 2, p, p, p, 0.5, None, *extra) == MCF_ERR_ARG
    out.gref = None
    assert loop(3, 2, p, p, p, 0.5, C.byref(out), *extra) == MCF_ERR_ARG
    assert b"mcf_leafrfromalb" in lib.mcf_last_error()


def test_r_glue_registers_the_three_entries():
    src = (ROOT / "r" / "mcfhip_glue.c").read_text()
    entries = {m.group(1): int(m.group(2)) for m in re.finditer(r'\{"(mcfhip_\w+)",\s*\(DL_FUNC\)&\1,\s*(\d+)\}', src)}
    assert entries.get("mcfhip_find_lref") == 5 and entries.get("mcfhip_find_gref") == 5 and entries.get("mcfhip_fill_na") == 2
    rsrc = (ROOT / "r" / "mcfhip_overrides.R").read_text()
    for nm in ("find_lref", "find_gref", "fill_naCpp"):
        assert f'"{nm}"' in rsrc
