"""mcf_flowacc_device / mcf_topidx_device (mcf_hydro.hip: the elevation-ordered sweep restated as a subtree count found by
pointer doubling) against the restatement in oracle/hydro_oracle.py and the host code of mcf_hydro.cpp.  The counts are
integers: exact, and bit-identical from run to run; the index to the rounding of atan / tan."""
import numpy as np
import pytest

from microclimf_amd.terrain import flowaccCpp, topidx
from oracle import hydro_oracle as HO
from test_hydro_cpu import rasters
from test_terrain_cpu import synth_dtm

pytestmark = pytest.mark.gpu


def plateaus():
    """late edges (a cell whose receiver was processed before it) exist only where elevations tie"""
    yield "all_zero", np.zeros((9, 11))
    yield "integers", np.round(synth_dtm(23, 17))
    z = np.round(synth_dtm(21, 19))
    z[np.random.default_rng(5).random(z.shape) < 0.10] = np.nan
    yield "integers_with_na", z


CASES = list(rasters()) + list(plateaus()) + [("all_na", np.full((6, 5), np.nan))]


@pytest.mark.parametrize("name,z", CASES, ids=[n for n, _ in CASES])
def test_flowacc_equals_the_restatement(name, z):
    got = flowaccCpp(z, device=0)
    want = HO.flowacc(z) if name != "all_na" else np.full(z.shape, -2147483648.0)     # (the restatement underflows there)
    assert np.array_equal(got, want), (name, int((got != want).sum()))
    assert (got[np.isnan(z)] == -2147483648.0).all()
    assert np.array_equal(got, flowaccCpp(z))


def big_rasters():
    z = synth_dtm(700, 900)
    z[100:140, 300:360] = np.nan
    z[:, -1] = np.nan
    yield "na_patch", z
    yield "half_metres", np.round(synth_dtm(700, 900) * 2.0) / 2.0


@pytest.mark.parametrize("name,z", list(big_rasters()), ids=[n for n, _ in big_rasters()])
def test_flowacc_equals_the_host_sweep_and_is_reproducible(name, z):
    got = flowaccCpp(z, device=0)
    want = flowaccCpp(z)
    assert np.array_equal(got, want), int((got != want).sum())
    again = flowaccCpp(z, device=0)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


TOPIDX = [(n, z) for n, z in CASES if z.shape[0] >= 3 and z.shape[1] >= 3]


@pytest.mark.parametrize("name,z", TOPIDX, ids=[n for n, _ in TOPIDX])
@pytest.mark.parametrize("res", [1.0, (2.0, 5.0), 30.0])
def test_topidx_equals_the_host_code(name, z, res):
    got = topidx(z, res, device=0)
    want = topidx(z, res)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    na = np.isnan(z)
    assert (got[na].view(np.uint64) == 0x7FF00000000007A2).all()           # masked cells are R's NA_real_
    assert (got[~na] > 0).all()


@pytest.mark.parametrize("hole", [False, True], ids=["odd", "even"])
def test_median_of_an_odd_and_an_even_count_of_slopes(hole):
    """the cells with an NA slope (raster edge, beside NA cells) take R's median of the others: the middle order statistic
    of an odd count, the mean of the two middle ones of an even count"""
    z = synth_dtm(9, 9, seed=8) * 3.0                   # 7 x 7 = 49 interior slopes, all different and above the floor
    if hole:
        z[0, 0] = np.nan                                # takes the slope of (1, 1) away: 48
    count = 48 if hole else 49
    pad = np.isnan(np.pad(z, 1, constant_values=np.nan))
    ok = np.ones(z.shape, dtype=bool)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            ok &= ~pad[dr:dr + 9, dc:dc + 9]
    assert ok.sum() == count
    got = topidx(z, 1.0, device=0)
    want = topidx(z, 1.0)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    # the median as the wetness index of the edge cells implies it: tan(B) = a / twi
    fa = flowaccCpp(z, device=0)
    edge = ~ok & ~np.isnan(z)
    slopes = np.arctan((fa[ok] + 1.0) / got[ok])
    implied = np.arctan((fa[edge] + 1.0) / got[edge])
    np.testing.assert_allclose(implied, np.median(slopes), rtol=1e-12)
