"""Leaf and ground reflectance from albedo: the reference's exported leafrfromalb() (R/dataprep.R:1000-1050) and the three
compiled functions under it (find_lref, find_gref, fill_naCpp; src/microclimfCpp.cpp:5675-5777) through libmcfhip
(include/mcf.h, "leaf and ground reflectance from albedo").

`device`: a HIP ordinal runs the kernels of mcf_vegprep.hip there; None selects the host entries (one core).  Rasters are
[rows, cols] arrays, NaN = NA."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .marshal import Buffers


def _raster(a, name, shape=None):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim != 2:
        raise ValueError(f"{name} must be a single layer raster, got shape {a.shape}")
    if shape is not None and a.shape != shape:
        raise ValueError(f"Geometries of inputs must match: {name} is {a.shape}, expected {shape}")
    return np.asfortranarray(a)


def _p(a):
    return Buffers().ptr(a)          # (every array is a local of the entry that makes the call)


def _call(name, device, *args):
    lib = _abi.load()
    if device is None:
        _abi.check(getattr(lib, name)(*args))
    else:
        _abi.check(getattr(lib, name + "_device")(*args, int(device)))


def find_lref(pai, gref, x, albin, ltrr=0.5, device=0) -> np.ndarray:
    """find_lref (cpp:5675-5699): per cell the leaf reflectance whose diffuse albedo over ground `gref` is `albin`."""
    pai = _raster(pai, "pai")
    gref, x, albin = (_raster(a, n, pai.shape) for a, n in ((gref, "gref"), (x, "x"), (albin, "albin")))
    out = np.empty(pai.shape, dtype=np.float64, order="F")
    _call("mcf_find_lref", device, pai.shape[0], pai.shape[1], _p(pai), _p(gref), _p(x), _p(albin), float(ltrr), _p(out))
    return out


def find_gref(lref, pai, x, albin, ltrr=0.5, device=0) -> np.ndarray:
    """find_gref (cpp:5701-5724): per cell the ground reflectance; NA where the bisection finds no root."""
    pai = _raster(pai, "pai")
    lref, x, albin = (_raster(a, n, pai.shape) for a, n in ((lref, "lref"), (x, "x"), (albin, "albin")))
    out = np.empty(pai.shape, dtype=np.float64, order="F")
    _call("mcf_find_gref", device, pai.shape[0], pai.shape[1], _p(lref), _p(pai), _p(x), _p(albin), float(ltrr), _p(out))
    return out


def fill_na(m, mask, device=0) -> np.ndarray:
    """fill_naCpp (cpp:5727-5777): NA cells inside the mask take the value the reference's breadth-first search brings them."""
    m = _raster(m, "m")
    mask = _raster(mask, "mask", m.shape)
    out = np.empty(m.shape, dtype=np.float64, order="F")
    _call("mcf_fill_na", device, m.shape[0], m.shape[1], _p(m), _p(mask), _p(out))
    return out


def leafrfromalb(pai, x, alb, ltrr=0.5, device=0) -> dict:
    """leafrfromalb(pai, x, alb, ltrr) (R/dataprep.R:1000-1050) -> {"leafr", "leaft", "gref"} and, beside them, "iterations"
    (passes done), "mxdif_gref" / "mxdif_leaf" (the two mean absolute differences of the last pass) and "lref_first" (the
    tst < 0.5 branch).  Refuses a multi-layer pai and rasters of different shapes, as the reference does."""
    pai = np.asarray(pai, dtype=np.float64)
    if pai.ndim == 3 and pai.shape[2] > 1:
        raise ValueError("pai must be a single layer raster")
    pai = _raster(pai, "pai")
    x, alb = _raster(x, "x", pai.shape), _raster(alb, "alb", pai.shape)
    res = {k: np.empty(pai.shape, dtype=np.float64, order="F") for k in ("leafr", "leaft", "gref")}
    out = _abi.LeafrOut()
    for k, a in res.items():
        setattr(out, k, _p(a))
    _call("mcf_leafrfromalb", device, pai.shape[0], pai.shape[1], _p(pai), _p(x), _p(alb), float(ltrr), C.byref(out))
    res.update(iterations=int(out.iterations), mxdif_gref=float(out.mxdif_gref), mxdif_leaf=float(out.mxdif_leaf),
               lref_first=bool(out.lref_first))
    return res


def selftest_residual(lref, pai, gref, x, albin, ltrr, device=None) -> np.ndarray:
    """leafrcpp elementwise as the host unit (device None) or the device unit builds it (mcf_selftest_vegprep kind 0 / 1)."""
    v = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel()) for a in (lref, pai, gref, x, albin)]
    n = v[0].size
    assert all(a.size == n for a in v)
    out = np.empty(n, dtype=np.float64)
    lib = _abi.load()
    _abi.check(lib.mcf_selftest_vegprep(0 if device is None else 1, n, 1, *[_p(a) for a in v], float(ltrr), _p(out), 256,
                                        0 if device is None else int(device)))
    return out


def selftest_leafrfromalb(pai, x, alb, ltrr=0.5, block=256, device=0) -> dict:
    """the device loop with `block` threads per workgroup (mcf_selftest_vegprep kind 2): for tests of launch independence"""
    pai = _raster(pai, "pai")
    x, alb = _raster(x, "x", pai.shape), _raster(alb, "alb", pai.shape)
    n = pai.size
    out = np.empty(3 * n + 4, dtype=np.float64)
    lib = _abi.load()
    _abi.check(lib.mcf_selftest_vegprep(2, pai.shape[0], pai.shape[1], _p(pai), _p(x), _p(alb), None, None, float(ltrr), _p(out),
                                        int(block), int(device)))
    r = {k: out[i * n:(i + 1) * n].reshape(pai.shape, order="F") for i, k in enumerate(("leafr", "leaft", "gref"))}
    r.update(iterations=int(out[3 * n]), mxdif_gref=float(out[3 * n + 1]), mxdif_leaf=float(out[3 * n + 2]),
             lref_first=bool(out[3 * n + 3]))
    return r
