"""Height profiles from one plan, CPU side: the host twin of the foliage kernel against scipy's gamma distribution, the new
entries' declarations and bindings, and the refusals that need no device — each with its sentence, which starts with the
entry's name."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi, api, frontend, synthetic
import parity_bars

NEW = ("mcf_foliageden", "mcf_foliageden_device", "mcf_plan_set_height", "mcf_plan_fetch_foliage", "mcf_runmicro_heights")
T = 24 * 2
E_ARG = 1
RATE = 1.5 / 7
BAR = 2.0 ** -40
assert BAR == parity_bars.FLOOR


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def rel(got, want):
    """largest relative distance where both are finite and non-zero"""
    m = np.isfinite(got) & np.isfinite(want) & (got != 0) & (want != 0)
    return float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m]))) if m.any() else 0.0


def same_pattern(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0) and \
        np.array_equal(np.isinf(got), np.isinf(want))


def sweep():
    """(hgt, pai, z) with t = rate x from 1e-12 to 15/7, the series / closed-form threshold and its neighbours, z = hgt, z > hgt,
    hgt = 0, NaN hgt, NaN pai and pai = 0"""
    z = 0.37
    t = np.concatenate([np.logspace(-12, np.log10(15 / 7 * (1 - 1e-9)), 3001), [0.4999999, 0.5, 0.5000001, 1e-4, 1.7e-4]])
    hgt = z / (1 - (t / RATE) / 10)                       # x = ((hgt - z) / hgt) 10 = t / rate
    pai = 0.1 + 3.9 * np.linspace(0, 1, hgt.size) ** 2
    special_h = np.array([z, 0.2, 0.1, 0.0, 0.0, np.nan, 2.0, 2.0, 5.0])
    special_p = np.array([1.0, 1.0, 0.0, 0.0, 1.5, 1.0, np.nan, 0.0, 0.0])
    return np.concatenate([hgt, special_h]), np.concatenate([pai, special_p]), z, t.size


def test_host_twin_matches_scipy_over_the_whole_range():
    _lib()
    hgt, pai, z, n = sweep()
    want_ld, want_pa = frontend.foliageden(z, hgt, pai)
    # the reference side first: scipy is finite and non-zero over the regular part of the sweep, so the bar below bites there
    assert np.isfinite(want_ld[:n]).all() and (want_ld[:n] > 0).all() and np.isfinite(want_pa[:n]).all() and (want_pa[:n] > 0).all()
    ld, pa = api.foliageden(hgt, pai, z)
    print(f"host twin against scipy: leafden {rel(ld, want_ld):.3e}, paia {rel(pa, want_pa):.3e} (bar {BAR:.3e})")
    assert same_pattern(ld, want_ld) and same_pattern(pa, want_pa)
    assert rel(ld, want_ld) <= BAR and rel(pa, want_pa) <= BAR
    # the special cells by name: z = hgt and z > hgt are exact zeros, hgt = 0 gives paia 0 and leafden NaN, NaN propagates
    s_ld, s_pa = ld[n:], pa[n:]
    assert (s_ld[:2] == 0).all() and (s_pa[:2] == 0).all()
    assert np.isnan(s_ld[3]) and s_pa[3] == 0 and np.isnan(s_ld[4]) and s_pa[4] == 0
    assert np.isnan(s_ld[5]) and np.isnan(s_pa[5]) and np.isnan(s_ld[6]) and np.isnan(s_pa[6])
    assert s_ld[7] == 0 and s_pa[7] == 0 and s_ld[8] == 0 and s_pa[8] == 0


def test_host_twin_on_rasters_and_layers():
    """[rows, cols, layers] arrays, canopies from 0 to 6 m with bare and NA cells, at the heights the GPU tests visit"""
    _lib()
    rng = np.random.default_rng(5)
    hgt = rng.uniform(0, 6, (23, 3, 2))
    pai = rng.uniform(0, 4, (23, 3, 2))
    hgt[2, 1, :] = 0.0
    pai[2, 1, :] = 0.0
    hgt[5, 0, :] = np.nan
    pai[5, 0, :] = np.nan
    for z in (0.02, 0.3, 1.5, 4.0):
        want_ld, want_pa = frontend.foliageden(z, hgt, pai)
        ld, pa = api.foliageden(hgt, pai, z)
        assert ld.shape == hgt.shape and same_pattern(ld, want_ld) and same_pattern(pa, want_pa)
        assert rel(ld, want_ld) <= BAR and rel(pa, want_pa) <= BAR
    with pytest.raises(ValueError, match="differ in shape"):
        api.foliageden(hgt, pai[:, :, 0], 1.0)


def test_new_entries_are_declared_exported_and_bound():
    lib = _lib()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "mcf.h").read_text()
    for n in NEW:
        assert n in _abi.EXPORTS and hasattr(lib, n), n
        assert re.search(r"^int " + n + r"\(", hdr, re.M), n
        assert getattr(lib, n).argtypes and getattr(lib, n).restype is C.c_int, n
        assert re.search(rf"added since, functions only:[^)]*\b{n}\b", hdr, re.S), n
    assert lib.mcf_abi_version() == 8 == _abi.ABI_VERSION and re.search(r"^#define MCF_ABI_VERSION 8\b", hdr, re.M)
    assert lib.mcf_foliageden_device.argtypes[-1] is C.c_int32
    for m in ("set_height", "fetch_foliage"):
        assert callable(getattr(api.Plan, m)), m
    for f in (api.foliageden, api.runmicro_heights, frontend.runmicro_heights, frontend.runmicro_heights_summary):
        assert callable(f)
    import inspect
    assert inspect.signature(frontend.prepare_grid_inputs).parameters["foliage"].default is True


def _args():
    a = synthetic.workload(5, 4, T, reqhgt=0.3)
    a.pop("reqhgt")
    return a


@pytest.mark.parametrize("heights,msg", [
    ([], "a null or empty list of heights"),
    ([0.5, 0.0], r"a height must be > 0 \(the ground surface, reqhgt = 0: mcf_runmicro1"),
    ([-0.1], r"a height must be > 0 \(below ground: mcf_runmicro_depths\)"),
    ([0.2, 1.0, float("nan")], "a height must be > 0, got NaN"),
], ids=["empty", "zero", "negative", "nan"])
def test_height_list_refusals_need_no_device(heights, msg):
    """MCF_ERR_ARG, the sentence led by the entry's name, before any device is touched: the same with and without one"""
    _lib()
    with pytest.raises(_abi.McfError, match=r"error 1: mcf_runmicro_heights: " + msg):
        api.runmicro_heights(**_args(), heights=heights)


def test_null_arguments_are_refused():
    lib = _lib()
    P = _abi.c_double_p
    buf = np.zeros(4)
    assert lib.mcf_plan_set_height(None, 1.0, None) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_plan_set_height: null plan")
    assert lib.mcf_plan_fetch_foliage(None, buf.ctypes.data_as(P), buf.ctypes.data_as(P)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_plan_fetch_foliage: null plan")
    h = np.array([0.5])
    assert lib.mcf_runmicro_heights(None, None, None, 1, None, None) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_heights: a null or empty list")
    assert lib.mcf_runmicro_heights(None, None, h.ctypes.data_as(P), 1, None, None) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_heights: null argument")
    assert lib.mcf_foliageden(0, buf.ctypes.data_as(P), buf.ctypes.data_as(P), 1.0, buf.ctypes.data_as(P), buf.ctypes.data_as(P)) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_foliageden: ")
    assert lib.mcf_foliageden_device(4, None, buf.ctypes.data_as(P), 1.0, buf.ctypes.data_as(P), buf.ctypes.data_as(P), 0) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_foliageden_device: ")


def test_vegp_needs_no_foliage_planes_and_fine_arrays_are_refused():
    """in->vegp.paia / leafden may be NULL; fine array forcing has no one-plan route (both judged before a device is needed)"""
    lib = _lib()
    a = _args()
    a["vegp"] = {k: v for k, v in a["vegp"].items() if k not in ("paia", "leafden")}
    if lib.mcf_device_count() > 0:
        got = api.runmicro_heights(**a, heights=[0.2, 1.0])
        assert len(got["Tz"]) == 2 and got["Tz"][1].shape == (5, 4, T)
    else:
        with pytest.raises(_abi.McfError, match=r"error 2: .*no HIP device"):      # no CPU fallback
            api.runmicro_heights(**a, heights=[0.2, 1.0])
    with pytest.raises(ValueError, match="pai_a: one entry per height"):
        api.runmicro_heights(**a, heights=[0.2, 1.0], pai_a=[None])
    af = synthetic.workload(5, 4, T, reqhgt=0.3, array_forcing=True)
    af.pop("reqhgt")
    m = api.marshal(**af, reqhgt=0.3, array_forcing=True)
    h = np.array([0.3])
    outs = (_abi.Outputs * 1)()
    assert lib.mcf_runmicro_heights(C.byref(m.inputs), C.byref(m.options), h.ctypes.data_as(_abi.c_double_p), 1, None, outs) == E_ARG
    assert lib.mcf_last_error().startswith(b"mcf_runmicro_heights: vector forcing or coarse array forcing")


def test_front_end_refuses_a_depth():
    for bad in ([0.5, -0.1], [0.0], [], [float("nan")]):
        with pytest.raises(ValueError, match="heights: one or more heights above ground"):
            frontend.runmicro_heights({}, bad, {}, {}, {})
    with pytest.raises(ValueError, match="heights"):
        frontend.runmicro_heights_summary({}, [-0.2], {}, {}, {})
    with pytest.raises(ValueError, match="vars"):
        frontend.runmicro_heights_summary({}, [0.2], {}, {}, {}, vars=("Tz", "nope"))
    with pytest.raises(ValueError, match="pai_a: one entry per height"):
        frontend.runmicro_heights({}, [0.2, 0.4], {}, {}, {}, pai_a=[None])
