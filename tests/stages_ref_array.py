"""The array-weather yardstick of the staged model (tests/stages_ref_array.c) built and run from Python: tests/stages_ref.py's
flags, builds (the default, the three noise builds, the `exp32` slip), output names and bars — `parity_bars.bar_of` of the spread
between the noise builds and the default build, K, FLOOR and CAP as they are — for the oracle's array-forcing driver."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import parity_bars as PB
import stages_ref as SR
from microclimf_amd import _abi
from microclimf_amd.marshal import marshal

_DIR = Path(__file__).resolve().parent
_SRC = _DIR / "stages_ref_array.c"
NAMES, NOISE, EXTRA = SR.NAMES, SR.NOISE, SR.EXTRA
_libs = {}
_bars = {}


def lib_path(name):
    return SR._OUT / f"libstages_ref_array{'_' + name if name else ''}.so"


def build(name=None):
    out = lib_path(name)
    deps = [_SRC, SR._ORC / "mcf_oracle.c", SR._ORC / "mcf_oracle.h", _DIR.parent / "include" / "mcf.h"] + \
        sorted((SR._ORC / "variants").glob("*.h"))
    if out.exists() and all(d.stat().st_mtime <= out.stat().st_mtime for d in deps):
        return out
    SR._OUT.mkdir(exist_ok=True)
    flags, hdr = SR.BUILDS[name]
    cmd = ["gcc"] + SR.CFLAGS + ["-Wno-unused-function"] + flags
    if hdr:
        cmd += ["-include", str(SR._ORC / "variants" / hdr)]
    tmp = out.with_suffix(f".tmp{id(out)}.so")
    r = subprocess.run(cmd + ["-shared", "-o", str(tmp), str(_SRC), "-lm"], capture_output=True, text=True, cwd=str(SR._ORC))
    if r.returncode != 0:
        raise RuntimeError("stages_ref_array build failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    tmp.replace(out)
    return out


def load(name=None):
    if name not in _libs:
        lib = C.CDLL(str(build(name)))
        if name is not None:
            lib.orc_variant_probe.restype = C.c_int
            if lib.orc_variant_probe() != 1:
                raise RuntimeError(f"yardstick build {name!r} needs fused multiply-add, which this CPU does not have")
        lib.stages_run_array.restype = C.c_int
        lib.stages_run_array.argtypes = [C.POINTER(_abi.GridInputs), C.POINTER(_abi.Options), C.POINTER(SR.StagesOut)]
        lib.stages_count.restype = C.c_int
        assert lib.stages_count() == len(NAMES)
        _libs[name] = lib
    return _libs[name]


def run(a, name=None):
    """{variable: [rows, cols, tsteps]} of the array-forcing argument dict `a` (stages_array_cases `Case.full`) under build `name`"""
    a = dict(a)
    dfsel = a.pop("dfsel", None)
    m = marshal(*[a[k] for k in ("obstime", "climdata", "pointm", "vegp", "soilc", "reqhgt", "zref", "lat", "lon", "Sminp",
                                 "Smaxp", "tfact", "complete", "mat", "out")], True, dfsel=dfsel)
    so = SR.StagesOut()
    res = {}
    for i, n in enumerate(NAMES):
        res[n] = np.empty((m.rows, m.cols, m.tsteps), dtype=np.float64, order="F")
        so.var[i] = res[n].ctypes.data_as(_abi.c_double_p)
    rc = load(name).stages_run_array(C.byref(m.inputs), C.byref(m.options), C.byref(so))
    if rc != 0:
        raise RuntimeError(f"stages_run_array failed: {rc}")
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
