"""CPU-side checks of the day subset of a streamed below-ground plan (include/mcf.h mcf_plan_below_set_days,
mcf_below_days_range): declared, exported and bound, the ABI version unchanged (functions only), the Python surface, and the
host bookkeeping — the day list's validation and calendar range -> subset positions, ranges without a day of the subset
included — through mcf_below_days_range, which needs no device."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import McfError, _abi
from microclimf_amd.api import Plan, below_days_range

ROOT = Path(__file__).resolve().parent.parent
DAYS = [0, 1, 4, 5, 6, 9, 12, 13, 16, 18, 19]


def _lib():
    import __graft_entry__ as g
    g.build_library()
    return _abi.load()


def test_entries_are_declared_exported_and_bound_and_the_abi_version_stays():
    hdr = (ROOT / "include" / "mcf.h").read_text()
    assert "int mcf_plan_below_set_days(mcf_plan *plan, const int32_t *days, int32_t n);" in hdr
    assert re.search(r"int mcf_below_days_range\(const int32_t \*days, int32_t n, int32_t total_days, int32_t day0, int32_t ndays, "
                     r"int32_t \*pos0,\s*int32_t \*npos\);", hdr)
    assert int(re.search(r"#define MCF_ABI_VERSION (\d+)", hdr).group(1)) == 8
    lib = _lib()
    assert lib.mcf_abi_version() == _abi.ABI_VERSION == 8
    assert lib.mcf_plan_below_set_days.restype is C.c_int
    assert lib.mcf_plan_below_set_days.argtypes == [C.c_void_p, _abi.c_int32_p, C.c_int32]
    assert lib.mcf_below_days_range.restype is C.c_int
    assert lib.mcf_below_days_range.argtypes == [_abi.c_int32_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _abi.c_int32_p,
                                                 _abi.c_int32_p]
    assert {"mcf_plan_below_set_days", "mcf_below_days_range"} <= set(_abi.EXPORTS)


def test_null_plan_is_refused_without_touching_a_device():
    lib = _lib()
    d = np.array(DAYS, dtype=np.int32)
    assert lib.mcf_plan_below_set_days(None, d.ctypes.data_as(_abi.c_int32_p), d.size) == 1          # MCF_ERR_ARG
    assert b"null plan" in lib.mcf_last_error()


def test_plan_method():
    assert list(inspect.signature(Plan.below_set_days).parameters) == ["self", "days"]


def test_calendar_ranges_to_subset_positions():
    _lib()
    total = 20
    # every way a chunk can meet the subset: one run, across a gap, a chunk inside a gap, the first and the last day
    for (d0, nd), want in {(0, 20): (0, 11), (0, 1): (0, 1), (0, 2): (0, 2), (2, 2): (2, 0), (1, 6): (1, 4), (7, 7): (5, 3),
                           (14, 1): (8, 0), (15, 5): (8, 3), (19, 1): (10, 1), (10, 2): (6, 0), (5, 0): (3, 0)}.items():
        assert below_days_range(DAYS, total, d0, nd) == want, (d0, nd)
    # chunks of any size deal every position out exactly once, in order
    for chunk in (1, 2, 3, 5, 7, 20):
        nxt = 0
        for d0 in range(0, total, chunk):
            pos0, npos = below_days_range(DAYS, total, d0, min(chunk, total - d0))
            if npos:
                assert pos0 == nxt
                assert DAYS[pos0] >= d0 and DAYS[pos0 + npos - 1] < d0 + chunk
                nxt = pos0 + npos
        assert nxt == len(DAYS)
    # the identity list: a range is its own positions
    assert below_days_range(np.arange(total), total, 6, 5) == (6, 5)


@pytest.mark.parametrize("days,why", [([3, 2, 5], "strictly ascending"), ([2, 2, 5], "strictly ascending"), ([0, 20], "out of range"),
                                      ([-1, 4], "out of range"), ([], "no days")])
def test_bad_day_lists(days, why):
    _lib()
    with pytest.raises(McfError, match=why):
        below_days_range(days, 20, 0, 20)


def test_bad_ranges():
    _lib()
    for d0, nd in ((-1, 2), (19, 2), (0, -1)):
        with pytest.raises(McfError, match="day range out of bounds"):
            below_days_range(DAYS, 20, d0, nd)
