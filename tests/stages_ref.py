"""The staged model's yardstick (tests/stages_ref.c) built and run from Python, and the parity bars derived from it.

The C unit includes the unchanged oracle (oracle/mcf_oracle.c) and is built here with gcc into tests/_stages_build/ (ignored by
git) with the flags of oracle/Makefile: the default build, the three noise builds (`fma`, `ulp`, `ulpfma`: force-included
oracle/variants/ headers and the FMA flags, exactly how the oracle's variant libraries are made) and the `exp32` slip.  The
bar of (case, variable) is tests/parity_bars.py `bar_of` — K, FLOOR and CAP as they are — of the spread between the noise
builds and the default build."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import parity_bars as PB
from microclimf_amd import _abi
from microclimf_amd.marshal import marshal

_DIR = Path(__file__).resolve().parent
_OUT = _DIR / "_stages_build"
_ORC = _DIR.parent / "oracle"
CFLAGS = ["-O2", "-ffp-contract=off", "-fPIC", "-Wall", "-std=c99"]        # oracle/Makefile CFLAGS (its warnings: unused statics here)
FMAFLAGS = ["-ffp-contract=fast", "-mfma"]                                  # oracle/Makefile FMAFLAGS
BUILDS = {                                                                   # name -> (extra flags, force-included header)
    None: ([], None),
    "fma": (FMAFLAGS, "probe.h"),
    "ulp": ([], "ulp.h"),
    "ulpfma": (FMAFLAGS, "ulp.h"),
    "exp32": ([], "exp32.h"),
}
NOISE = ("fma", "ulp", "ulpfma")
EXTRA = ("Rbdown", "Rddown", "Rdup", "uz", "soilm")
NAMES = tuple(_abi.DIAG_NAMES) + EXTRA
_libs = {}
_bars = {}


class StagesOut(C.Structure):
    _fields_ = [("var", _abi.c_double_p * len(NAMES))]


def lib_path(name):
    return _OUT / f"libstages_ref{'_' + name if name else ''}.so"


def build(name=None):
    out = lib_path(name)
    deps = [_DIR / "stages_ref.c", _ORC / "mcf_oracle.c", _ORC / "mcf_oracle.h", _DIR.parent / "include" / "mcf.h"] + \
        sorted((_ORC / "variants").glob("*.h"))
    if out.exists() and all(d.stat().st_mtime <= out.stat().st_mtime for d in deps):
        return out
    _OUT.mkdir(exist_ok=True)
    flags, hdr = BUILDS[name]
    cmd = ["gcc"] + CFLAGS + ["-Wno-unused-function"] + flags
    if hdr:
        cmd += ["-include", str(_ORC / "variants" / hdr)]
    tmp = out.with_suffix(f".tmp{id(out)}.so")
    r = subprocess.run(cmd + ["-shared", "-o", str(tmp), str(_DIR / "stages_ref.c"), "-lm"], capture_output=True, text=True,
                       cwd=str(_ORC))
    if r.returncode != 0:
        raise RuntimeError("stages_ref build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    tmp.replace(out)
    return out


def load(name=None):
    if name not in _libs:
        lib = C.CDLL(str(build(name)))
        if name is not None:
            lib.orc_variant_probe.restype = C.c_int
            if lib.orc_variant_probe() != 1:
                raise RuntimeError(f"yardstick build {name!r} needs fused multiply-add, which this CPU does not have")
        lib.stages_run.restype = C.c_int
        lib.stages_run.argtypes = [C.POINTER(_abi.GridInputs), C.POINTER(_abi.Options), C.POINTER(StagesOut)]
        lib.stages_count.restype = C.c_int
        assert lib.stages_count() == len(NAMES)
        _libs[name] = lib
    return _libs[name]


def run(a, name=None):
    """{variable: [rows, cols, tsteps]} of the argument dict `a` (stages_cases.build) under build `name`"""
    a = dict(a)
    dfsel = a.pop("dfsel", None)
    m = marshal(*[a[k] for k in ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp",
                                 "Smaxp", "tfact", "complete", "mat", "out")], False, dfsel=dfsel)
    so = StagesOut()
    res = {}
    for i, n in enumerate(NAMES):
        res[n] = np.empty((m.rows, m.cols, m.tsteps), dtype=np.float64, order="F")
        so.var[i] = res[n].ctypes.data_as(_abi.c_double_p)
    rc = load(name).stages_run(C.byref(m.inputs), C.byref(m.options), C.byref(so))
    if rc != 0:
        raise RuntimeError(f"stages_run failed: {rc}")
    return res


def bars_for(key, a):
    """(want, bars, noise) of a case: the default yardstick's values, and per variable parity_bars.bar_of of the largest
    distance of a noise build from them; computed once per key"""
    if key not in _bars:
        want = run(a)
        noise = {k: 0.0 for k in want}
        for v in NOISE:
            for k, d in PB.distances(want, run(a, v), f"noise build {v}: ").items():
                noise[k] = max(noise[k], d)
        _bars[key] = (want, {k: PB.bar_of(n) for k, n in noise.items()}, noise)
    return _bars[key]
