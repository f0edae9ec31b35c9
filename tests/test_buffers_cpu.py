"""The Python bindings' buffer owner (marshal.Buffers) and what hangs on it, as far as no other test reaches: a pointer it
hands out stays good for as long as the owner (or the struct that holds the owner) is referenced, the two integer coercions are
what their names say, `f64` reads a vector of the right size in Fortran order, and the one coarse-wind function returns the
bits of the expressions the host loops used to spell out."""
import ctypes as C
import gc

import numpy as np
import pytest

from microclimf_amd import _abi, api
from microclimf_amd import snow as S
from microclimf_amd.marshal import Buffers, Marshalled, SnowMarshalled

INT_MIN = int(np.iinfo(np.int32).min)
SHAPES = [(5,), (2, 3)]


def _churn():
    """collect, then allocate and free a few MB so that freed blocks would be handed out again"""
    gc.collect()
    for _ in range(3):
        junk = [np.full(1 << 17, 7.0) for _ in range(4)]
        del junk
    gc.collect()


def _read(ptr, n):
    return [ptr[i] for i in range(n)]


def _values(shape, dtype=np.float64):
    return (np.arange(int(np.prod(shape)), dtype=np.float64) * 1.5 + 1).reshape(shape).astype(dtype)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("method", ["f64", "i32_plain", "i32_rcpp", "i64", "ptr"])
def test_a_temporary_outlives_every_other_reference(method, shape):
    b = Buffers()
    if method == "f64":
        ptr, want = b.f64(_values(shape) + 0.0, shape, "x"), _values(shape)
    elif method == "i32_plain":
        ptr, want = b.i32_plain(_values(shape, np.int64)), _values(shape, np.int64)
    elif method == "i32_rcpp":
        ptr, want = b.i32_rcpp(_values(shape) + 0.25, shape, "x"), np.trunc(_values(shape) + 0.25)
    elif method == "i64":
        ptr, want = b.i64(_values(shape, np.int32)), _values(shape, np.int32)
    else:
        ptr, want = b.ptr(np.asfortranarray(_values(shape))), _values(shape)
    _churn()
    assert _read(ptr, want.size) == want.ravel(order="F" if method in ("f64", "i32_rcpp", "ptr") else "C").tolist()
    assert b.ptr(None) is None


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, np.int32])
def test_an_output_array_outlives_the_callers_reference(shape, dtype):
    b = Buffers()
    a, ptr = b.out(shape, dtype)
    assert a.flags.f_contiguous and a.dtype == dtype and a.shape == shape
    a[...] = _values(shape, dtype)
    del a
    _churn()
    assert _read(ptr, int(np.prod(shape))) == _values(shape, dtype).ravel(order="F").tolist()
    z, zp = b.out(shape, dtype, zero=True)
    assert not z.any() and _read(zp, z.size) == [0] * z.size


@pytest.mark.parametrize("periods", [[0, 1, -1, 1, 2], [[0, 1, 1], [2, -1, 0]]])
def test_the_summary_specs_hold_their_period_tables(periods):
    want = np.asarray(periods).ravel().tolist()
    specs = [api.summary_spec(np.array(periods), ("Tz",), ("mean",))[0],
             S.snowpack_summary_spec(np.array(periods), ("totalSWE",), ("max",))[0]]
    _churn()
    for sp in specs:
        assert sp.nperiods == 3 and _read(sp.period_of_day, len(want)) == want
    assert len(api.summary_spec(periods, ("Tz",), ("mean",))) == 4 and len(S.snowpack_summary_spec(periods)) == 4


@pytest.mark.parametrize("devices", [[4, 0, 2, 1, 3], [1, 0, 1, 0, 1, 0]])
def test_multi_holds_its_device_list(devices):
    mu = _abi.multi(list(devices), 2)
    _churn()
    assert mu[0].n_devices == len(devices) and _read(mu[0].devices, len(devices)) == devices and mu[0].n_blocks == 2
    assert C.sizeof(mu) == C.sizeof(_abi.Multi) and _abi.multi(None, 0) is None


def test_the_two_integer_rules_side_by_side():
    x = [1.9, -1.9, np.nan, 2.0]
    b = Buffers()
    assert _read(b.i32_rcpp(x, (4,), "x"), 4) == [1, -1, INT_MIN, 2]
    assert _read(b.i32_plain([3, -7, 2 ** 31 - 1, 0], 4, "y"), 4) == [3, -7, 2 ** 31 - 1, 0]
    with pytest.raises(ValueError, match=r"other\$isnowac"):
        b.i32_rcpp(x, (2, 3), "other$isnowac")
    with pytest.raises(ValueError, match=r"obstime\$year"):
        b.i32_plain([1, 2, 3], 4, "obstime$year")
    # each marshalling keeps the rule it had: the grid solver's the plain one, the snow branch's Rcpp's
    assert Marshalled.i32 is Buffers.i32_plain and SnowMarshalled.i32 is Buffers.i32_rcpp
    assert _read(SnowMarshalled().i32(x, (4,), "x"), 4) == [1, -1, INT_MIN, 2]


def test_f64_reads_a_vector_of_the_right_size_in_fortran_order():
    b = Buffers()
    v = np.arange(6.0)                                      # C-ordered (6,) asked for as (2, 3): column-major, so memory = v
    assert _read(b.f64(v, (2, 3), "m"), 6) == v.tolist()
    assert b._keep[-1].shape == (2, 3) and b._keep[-1].flags.f_contiguous and b._keep[-1][1, 0] == 1.0
    c = np.arange(6.0).reshape(2, 3)                        # a C-ordered matrix of the right shape is copied to column-major
    assert _read(b.f64(c, (2, 3), "m"), 6) == c.ravel(order="F").tolist()
    assert _read(b.f64([1, 2, 3]), 3) == [1.0, 2.0, 3.0]    # no shape: as it comes
    with pytest.raises(ValueError, match=r"vegp\$hgt: expected shape \(2, 3\), got \(5,\)"):
        b.f64(np.zeros(5), (2, 3), "vegp$hgt")


def test_coarse_wind_has_the_bits_of_the_host_loops_expressions():
    rng = np.random.default_rng(17)
    speed, direction = rng.uniform(0.2, 9.0, (2, 3, 4)), rng.uniform(0.0, 360.0, (2, 3, 4))
    speed[1, 2, :] = np.nan                                 # one coarse cell without weather
    clim_c = {"windspeed": speed, "winddir": direction}
    # `snowmodel2_chunks`' own lines, as they stood before the function existed
    wd = np.asarray(clim_c["winddir"], dtype=np.float64) * np.pi / 180
    wu_c = np.asarray(clim_c["windspeed"], dtype=np.float64) * np.cos(wd)
    wv_c = np.asarray(clim_c["windspeed"], dtype=np.float64) * np.sin(wd)
    wuv, wvv = np.nanmean(wu_c, axis=(0, 1)), np.nanmean(wv_c, axis=(0, 1))
    winddir = (np.arctan2(wvv, wuv) * 180 / np.pi) % 360
    af_wind = np.sqrt(wuv ** 2 + wvv ** 2)
    got = S.coarse_wind(clim_c["windspeed"], clim_c["winddir"])
    assert len(got) == 4
    for g, w in zip(got, (wu_c, wv_c, winddir, af_wind)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    assert np.isfinite(got[2]).all() and np.isnan(got[0][1, 2]).all()
