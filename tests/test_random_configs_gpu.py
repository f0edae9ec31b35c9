"""Seeded random configurations of the one-shot solver entries against the oracle: raster shape (incl. single rows /
columns and sizes that do not fill a workgroup), series length (whole days + a ragged tail), height class, season,
latitude, cold spells, NA share, output mask, forcing geometry, workgroup geometry, day chunking — the cross product the
hand-written cases of tests/parity_cases.py sample only along its axes."""
import pytest

from microclimf_amd import synthetic
from microclimf_amd.api import runmicro1Cpp, runmicro2Cpp
import parity_bars
from parity_cases import draw
from test_parity_gpu import compare

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(96))
def test_random_configuration(oracle, i):
    rows, cols, T, kw, extra = draw(i)
    a = synthetic.workload(rows, cols, T, **kw)
    af = kw["array_forcing"]
    want, bars = parity_bars.grid(oracle, a, af)
    if af:
        a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
        got = runmicro2Cpp(**a, **extra)
    else:
        got = runmicro1Cpp(**a, **extra)
    compare(got, want, bars)


@pytest.mark.parametrize("af,reqhgt", [(False, 0.05), (True, 0.6), (False, -0.05)])
def test_medium_raster_against_the_oracle(oracle, af, reqhgt):
    """~900 workgroups: more than one XCD round and both hour rotations of the tile schedule (blockIdx >> 8), which the
    small cases above never reach, compared value by value"""
    a = synthetic.workload(160, 120, 72, reqhgt=reqhgt, variety=True, start_doy=200, array_forcing=af, na_frac=0.03)
    want, bars = parity_bars.grid(oracle, a, af)
    if af:
        a["lats"], a["lons"] = a.pop("lat"), a.pop("lon")
        got = runmicro2Cpp(**a)
    else:
        got = runmicro1Cpp(**a)
    compare(got, want, bars)
