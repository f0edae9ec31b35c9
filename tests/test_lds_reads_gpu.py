"""k_solve reads its operands from LDS one 8-byte read at a time (mcf_device.hpp `lds_operand`); how an operand is read
changes no arithmetic, so every output stays what it was, bit for bit.  One 9 x 5 raster — 45 cells: two full 21-cell tiles
and a partial one of three cells — with an NA cell, a bare cell and a vegetated cell, 72 hourly steps, all ten outputs:
  (i)   three one-day launches against one three-day launch: the same bits;
  (ii)  21-cell tiles against 32-cell tiles: the same bits;
  (iii) the oracle, under the bars derived from its own rounding sensitivity (parity_bars.py);
  (iv)  a forcing step that makes NaNs: the launch in the reference's clamp form (a NaN in the step table), and the canary path
        through k_solve_fix (a NaN in one cell's forcing array; a finite step that makes NaNs inside regular cells), which
        shares the accessors — the oracle's NA pattern each time."""
import functools

import numpy as np
import pytest

from microclimf_amd import synthetic
from microclimf_amd.api import Plan, runmicro1Cpp
import parity_bars

pytestmark = pytest.mark.gpu
ROWS, COLS, DAYS = 9, 5, 3
NAMES = ("Tz", "tleaf", "relhum", "soilm", "windspeed", "Rdirdown", "Rdifdown", "Rlwdown", "Rswup", "Rlwup")
NA_CELL, BARE_CELL, VEG_CELL = (1, 1), (2, 3), (4, 2)        # tiles 0, 1 and 1 (cell = row + 9 * column)


def _raster(array_forcing=False):
    a = synthetic.workload(ROWS, COLS, 24 * DAYS, reqhgt=0.05, variety=True, start_doy=170, array_forcing=array_forcing)
    v = a["vegp"]
    v["hgt"][NA_CELL] = np.nan
    for k in ("hgt", "pai", "paia"):
        v[k][BARE_CELL] = 0.0
    v["leafden"][BARE_CELL] = np.nan                          # 0 / 0, as the marshaller makes it
    v["hgt"][VEG_CELL], v["pai"][VEG_CELL] = 0.8, 2.0
    v["paia"][VEG_CELL], v["leafden"][VEG_CELL] = 0.7 * 2.0, 2.0 / 0.8
    return a


@functools.lru_cache(maxsize=None)
def _whole():
    """the raster's ten outputs from one three-day launch of the 21-cell kernel: the run (i), (ii) and (iii) share"""
    a = _raster()
    got = runmicro1Cpp(**a, days_per_chunk=DAYS, cells_per_block=21)
    assert list(got) == list(NAMES)
    return a, got


def _same_bits(x, y):
    for k in NAMES:
        assert x[k].shape == y[k].shape == (ROWS, COLS, 24 * DAYS), k
        assert np.array_equal(x[k].view(np.uint64), y[k].view(np.uint64)), k


def test_the_raster_has_its_three_kinds_of_cell():
    a, got = _whole()
    assert np.isnan(got["Tz"][NA_CELL]).all() and np.isnan(got["soilm"][NA_CELL]).all()
    assert np.isfinite(got["Tz"][BARE_CELL]).all() and np.isfinite(got["Tz"][VEG_CELL]).all()
    assert a["vegp"]["pai"][BARE_CELL] == 0.0 and a["vegp"]["hgt"][VEG_CELL] > a["reqhgt"]
    assert (got["Rdirdown"][VEG_CELL] > 0.0).any()           # a lit step below the canopy: the short-wave block ran


def test_three_one_day_launches_equal_one_three_day_launch():
    a, whole = _whole()
    _same_bits(runmicro1Cpp(**a, days_per_chunk=1, cells_per_block=21), whole)


def test_21_cell_tiles_equal_32_cell_tiles():
    a, whole = _whole()
    _same_bits(runmicro1Cpp(**a, days_per_chunk=DAYS, cells_per_block=32), whole)


def test_the_oracle_under_its_derived_bars(oracle):
    a, whole = _whole()
    want, bars = parity_bars.grid(oracle, a, key="lds_reads")
    worst = parity_bars.compare(whole, want, bars)
    for k in NAMES:
        print(f"  {k:10s} distance {worst[k]:.3e}  bar {bars[k]:.3e}")


def _plan_run(a, **kw):
    with Plan(**a, ring_days=DAYS, ring_slots=1, cells_per_block=21, **kw) as p:
        if kw.get("array_forcing"):
            p.upload_forcing_days(0, DAYS, 0)
        p.run_days(0, DAYS, 0)
        p.sync()
        got = {k: p.fetch(0, k, 0, 24 * DAYS) for k in NAMES}
        st = p.dispatch_stats()
    return got, st


def test_a_nan_forcing_step_keeps_the_oracles_na_pattern(oracle):
    """a NaN in the step table: the host sends the launch to the reference's clamp form (k_solve F = false)"""
    a = _raster()
    a["climdata"]["lwdown"] = a["climdata"]["lwdown"].copy()
    a["climdata"]["lwdown"][30] = np.nan                      # day 1, hour 6
    got, st = _plan_run(a)
    assert st["irregular_days"] == 1 and st["slow_launches"] >= 1, st
    want = oracle.run_grid(**a)
    assert np.isnan(want["Tz"][VEG_CELL][30]) and np.isfinite(want["Tz"][VEG_CELL][54])
    parity_bars.compare(got, want, tol=parity_bars.CAP)       # NaN / inf pattern, NA payload, values


def test_a_nan_in_one_cells_forcing_goes_through_the_fix_kernel(oracle):
    """array forcing has no step table to classify: the lane's canary trips and k_solve_fix redoes the tile"""
    a = _raster(array_forcing=True)
    a["climdata"]["tc"] = a["climdata"]["tc"].copy(order="F")
    a["climdata"]["tc"][VEG_CELL + (30,)] = np.nan            # tile 1, day 1, hour 6
    got, st = _plan_run(a, array_forcing=True)
    assert st["slow_tiles"] == 0 and st["fast_launches"] == 1 and st["canary_trips"] >= 1, st
    want = oracle.run_grid(**a, array_forcing=True)
    assert np.isnan(want["Tz"][VEG_CELL][30]) and np.isfinite(want["Tz"][VEG_CELL][6])
    parity_bars.compare(got, want, tol=parity_bars.CAP)


def test_a_finite_step_that_makes_nans_goes_through_the_fix_kernel(oracle):
    """vector forcing: a wind speed of 1e8 is a regular step, the NaNs are born inside the cells (k_solve_fix<21, 0>)"""
    a = _raster()
    a["climdata"]["windspeed"] = a["climdata"]["windspeed"].copy()
    a["climdata"]["windspeed"][30] = 1e8
    got, st = _plan_run(a)
    assert st["irregular_days"] == 0 and st["fast_launches"] == 1 and st["canary_trips"] >= 1, st
    want = oracle.run_grid(**a)
    assert np.isnan(want["Tz"][:, :, 30]).sum() > 1 and np.isfinite(want["Tz"][VEG_CELL][31])
    parity_bars.compare(got, want, tol=parity_bars.CAP)
