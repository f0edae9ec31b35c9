"""Array-weather runbioclim on COARSE arrays (mcf_runbioclim2 / 4 with array_forcing == 2, api.runbioclim2Cpp_coarse /
4Cpp_coarse): the whole-series sink against expand-then-oracle, and the streamed sink — the solver in day chunks, the
variance's second pass tapping the resident coarse soil moisture series (k_bioclim_fin<true>) — bit for bit the whole-series
one.  Workloads and bars: tests/bioclim_coarse_cases.py."""
import math

import numpy as np
import pytest

from microclimf_amd import api
from microclimf_amd.api import runbioclim2Cpp_coarse, runbioclim4Cpp_coarse
import bioclim_coarse_cases as BC
import parity_bars

pytestmark = pytest.mark.gpu
NAMES = [f"bio{i}" for i in range(1, 20)]
NDAYS = BC.T // 24
assert NDAYS == 26
QUARTER_VARS = [f"bio{i}" for i in (8, 9, 10, 11, 16, 17, 18, 19)]


def run(shape, air, layered=False, **kw):
    a, rp, cp = BC.build(shape, layered)
    wq, dq, hq, cq = BC.quarters()
    fn = runbioclim4Cpp_coarse if layered else runbioclim2Cpp_coarse
    return fn(**a, out=BC.OUT, wetq=wq, dryq=dq, hotq=hq, colq=cq, air=air, rowpos=rp, colpos=cp, **kw)


def assert_same_bits(got, ref, what):
    assert list(got) == list(ref) == NAMES, what
    for k in ref:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (what, k)
        fin = np.isfinite(ref[k])
        assert np.array_equal(np.isfinite(got[k]), fin), (what, k)
        assert np.array_equal(got[k][fin].view(np.uint64), ref[k][fin].view(np.uint64)), (what, k)


def ring_gb(shape, days):
    """MCF_BIOCLIM_RING_GB for chunks of `days` days: two variables x 8 B x the 32-cell tiles' 768-double day blocks"""
    rows, cols = BC.SHAPES[shape][:2]
    return repr((days + 0.5) * 2 * 8 * math.ceil(rows * cols / 32) * 768 / 1e9)


def against_oracle(oracle, got, shape, air, altcorrect=0):
    want = BC.want(oracle, shape, air, False, altcorrect)
    bars, noise = BC.bars(oracle, shape, air, altcorrect)
    case = f"{shape}/{'air' if air else 'leaf'}/altcorrect{altcorrect}"
    BC.record(case, got, want, bars, noise)
    valid = ~np.isnan(want["bio1"])
    assert not valid[BC.NA_CELL[shape]] and valid.sum() > 0.8 * valid.size
    for k in QUARTER_VARS:                    # static vegetation: the quarter days are modelled, nothing of them is NA
        assert np.isfinite(want[k][valid]).all(), k
    worst = parity_bars.compare(got, want, bars)          # NaN pattern, R's NA payload, every variable under its bar
    print(case, " ".join(f"{k}={v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("air", [True, False])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_whole_series_sink_with_coarse_forcing_against_the_oracle(oracle, monkeypatch, shape, air):
    """k_bioclim over the whole series of a coarse plan: the route mcf_runbioclim2 has always had for array_forcing == 2 and
    nothing had run — pinned against expand-then-oracle before the streamed sink is compared with it"""
    monkeypatch.setenv("MCF_BIOCLIM_WHOLE", "1")
    got = run(shape, air)
    assert api.bioclim_last_chunks() == 0
    against_oracle(oracle, got, shape, air)


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_streamed_sink_with_coarse_forcing_is_bit_for_bit_the_whole_series_sink(monkeypatch, shape, layered):
    """one-day chunks, five-day chunks (which cut the three-day quarters) and the whole series in one chunk, Tz and tleaf;
    layered: the quarter days lie past the fourteenth layer and stay NA, as tests/test_bioclim_gpu.py documents"""
    monkeypatch.setenv("MCF_BIOCLIM_WHOLE", "1")
    whole = {air: run(shape, air, layered) for air in (True, False)}
    assert api.bioclim_last_chunks() == 0
    monkeypatch.delenv("MCF_BIOCLIM_WHOLE")
    valid = ~np.isnan(whole[True]["bio1"])
    for k in QUARTER_VARS:
        assert np.isnan(whole[True][k]).all() if layered else np.isfinite(whole[True][k][valid]).all(), k
    for days, chunks in ((1, NDAYS), (5, math.ceil(NDAYS / 5)), (NDAYS, 1)):
        monkeypatch.setenv("MCF_BIOCLIM_RING_GB", "8" if days == NDAYS else ring_gb(shape, days))
        for air in (True, False):
            got = run(shape, air, layered)
            assert api.bioclim_last_chunks() == chunks, (days, air)
            assert_same_bits(got, whole[air], (shape, layered, days, air))


def test_finish_kernel_matches_the_per_lane_taps_of_the_solver_too(monkeypatch):
    """shape A takes the LDS-staged taps in k_solve; with MCF_NO_COARSE_LDS=1 the solver taps per lane — the finish kernel's
    per-lane taps must reproduce the soil moisture of either form"""
    monkeypatch.setenv("MCF_NO_COARSE_LDS", "1")
    monkeypatch.setenv("MCF_BIOCLIM_WHOLE", "1")
    whole = run("A", True)
    monkeypatch.delenv("MCF_BIOCLIM_WHOLE")
    monkeypatch.setenv("MCF_BIOCLIM_RING_GB", ring_gb("A", 1))
    got = run("A", True)
    assert api.bioclim_last_chunks() == NDAYS
    assert_same_bits(got, whole, "per-lane taps")
    monkeypatch.delenv("MCF_NO_COARSE_LDS")
    assert_same_bits(run("A", True), whole, "staged taps")


@pytest.mark.parametrize("altcorrect", [1, 2])
def test_altitude_correction(oracle, monkeypatch, altcorrect):
    zc, z = BC.elevations("A")
    kw = dict(altcorrect=altcorrect, dtmc=zc, dtm=z)
    monkeypatch.setenv("MCF_BIOCLIM_WHOLE", "1")
    whole = run("A", True, **kw)
    monkeypatch.delenv("MCF_BIOCLIM_WHOLE")
    monkeypatch.setenv("MCF_BIOCLIM_RING_GB", ring_gb("A", 5))
    got = run("A", True, **kw)
    assert api.bioclim_last_chunks() == math.ceil(NDAYS / 5)
    assert_same_bits(got, whole, altcorrect)
    against_oracle(oracle, got, "A", True, altcorrect)
    plain = BC.want(oracle, "A", True)
    fin = np.isfinite(plain["bio1"])
    assert np.abs(got["bio1"][fin] - plain["bio1"][fin]).max() > 0.1     # the correction does something


def test_row_blocks_give_the_same_bits():
    """mcf_runbioclim2_multi / 4_multi with coarse forcing: 37 rows in three blocks — a block boundary inside a 32-cell tile's
    column, coarse_rowpos and the fine elevations offset per block (mcf_rowblocks.hpp)"""
    zc, z = BC.elevations("A")
    for layered, kw in ((False, {}), (True, {}), (False, dict(altcorrect=2, dtmc=zc, dtm=z))):
        single = run("A", True, layered, **kw)
        assert api.bioclim_last_chunks() == 1
        parts = run("A", True, layered, devices=[0, 0], n_blocks=3, **kw)
        assert api.bioclim_last_chunks() == 3                              # one streamed chunk per block
        assert_same_bits(parts, single, (layered, kw.get("altcorrect", 0)))


def test_refusals():
    from microclimf_amd import McfError
    a, rp, cp = BC.build("B")
    wq, dq, hq, cq = BC.quarters()
    kw = dict(out=BC.OUT, dryq=dq, hotq=hq, colq=cq, air=True, rowpos=rp, colpos=cp)
    with pytest.raises(McfError, match="quarter index outside the time series"):
        runbioclim2Cpp_coarse(**a, wetq=np.append(wq[:-1], BC.T), **kw)
    with pytest.raises(ValueError, match="dtmc"):
        runbioclim2Cpp_coarse(**a, wetq=wq, altcorrect=1, **kw)
    with pytest.raises(McfError, match="coarse_rowpos"):
        runbioclim2Cpp_coarse(**a, wetq=wq, **dict(kw, rowpos=rp + 5.0))
