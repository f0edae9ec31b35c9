"""Workloads of the staged-model tests (tests/test_stages_cpu.py, tests/test_stages_gpu.py): the smallest shapes that still
exercise the diagnostics ring's layout.

5 x 10 cells: two full 21-cell tiles and a partial tile of 8.  96 h: four days, so the solver's three rotating day-reduction
buffers wrap.  Midsummer and midwinter, reqhgt 0.05 and 0; one layered run of two layers of two days each.  The seeds put an
NA cell and bare cells (pai == 0, which are also the cells with reqhgt above the canopy) into different tiles:
seed 16: NA at cell 23, bare at 33, 34, 46, 49; seed 33: NA at 38, bare at 0, 16, 19, 31 (column-major cell numbers) —
tests/test_stages_cpu.py asserts the mix from the inputs alone."""
from microclimf_amd import synthetic

ROWS, COLS, TSTEPS = 5, 10, 96
_SPEC = {
    "s170_h005": dict(seed=16, start_doy=170, reqhgt=0.05),
    "s355_h005": dict(seed=33, start_doy=355, reqhgt=0.05),
    "s170_h0": dict(seed=16, start_doy=170, reqhgt=0.0),
    "s355_h0": dict(seed=33, start_doy=355, reqhgt=0.0),
    "layered": dict(seed=16, start_doy=170, reqhgt=0.05, layers=2),
}
CASES = tuple(_SPEC)
_built = {}


def build(name):
    """-> the argument dict of runmicro1Cpp (runmicro3Cpp with its `dfsel` for the layered case); built once, not to be modified"""
    if name not in _built:
        kw = dict(_SPEC[name])
        layers = kw.pop("layers", 0)
        a = synthetic.workload(ROWS, COLS, TSTEPS, variety=True, na_frac=0.04, **kw)
        if layers:
            a = synthetic.layered(a, layers)
        _built[name] = a
    return _built[name]
