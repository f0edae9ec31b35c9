"""What mcf_plan_create refuses, with which code and which sentence, and which of two faults it reports: plan set-up runs its
checks in a fixed order between its uploads, and callers (and the R glue's error messages) see that order.  Every case is
refused by a host check; the sentences are the library's own, word for word."""
import ctypes as C

import numpy as np
import pytest

from microclimf_amd import _abi, synthetic
from microclimf_amd.marshal import marshal

pytestmark = pytest.mark.gpu

ROWS, COLS, T = 5, 4, 48
ERR_ARG = 1
COARSE_NEEDS = "coarse array forcing needs coarse_rows/cols, coarse_rowpos/colpos, coarse_relhum and coarse_winddir"
ROWPOS_RANGE = "coarse_rowpos must lie in [0, coarse_rows - 1]"
PITCH = "row_pitch smaller than rows"


def vector_inputs(**kw):
    a = synthetic.workload(ROWS, COLS, T, variety=True, start_doy=170, **kw)
    return marshal(**a, array_forcing=False)


def coarse_inputs(rowpos=None):
    a, rp, cp = synthetic.coarse_workload(ROWS, COLS, T, 2, 2, variety=True, start_doy=170)
    return marshal(**a, array_forcing=True, coarse={"rowpos": rp if rowpos is None else rowpos, "colpos": cp})


def bad_rowpos():
    rp = np.linspace(0.0, 1.0, ROWS)
    rp[3] = 1.5                      # past the last coarse row
    return rp


def pitch_too_small(m):
    m.inputs.row_pitch = ROWS - 1


def missing_coarse_relhum(m):
    m.inputs.coarse_relhum = None


def altcorrect_3(m):
    m.inputs.coarse_altcorrect = 3


def altcorrect_without_dtms(m):
    m.inputs.coarse_altcorrect = 1
    m.inputs.coarse_dtm = None
    m.inputs.fine_dtm = None


def coarse_below_incomplete(m):
    m.options.reqhgt = -0.1
    m.options.complete = 0


def missing_pai(m):
    m.inputs.vegp.pai = None


def missing_Vq(m):
    m.inputs.soilc.Vq = None


def missing_swdown(m):
    m.inputs.clim.swdown = None


def missing_winddir(m):
    m.inputs.clim.winddir = None


def missing_Tg(m):
    m.inputs.pointm.Tg = None


def below_incomplete():
    return vector_inputs(reqhgt=-0.1, complete=False, out=[1, 0, 0, 1, 0, 0, 0, 0, 0, 0])


# (inputs, the faults put into them, return code, sentence)
CASES = {
    "row_pitch smaller than rows": (vector_inputs, [pitch_too_small], ERR_ARG, PITCH),
    "a missing coarse input": (coarse_inputs, [missing_coarse_relhum], ERR_ARG, COARSE_NEEDS),
    "coarse_rowpos out of range": (lambda: coarse_inputs(bad_rowpos()), [], ERR_ARG, ROWPOS_RANGE),
    "coarse_altcorrect = 3": (coarse_inputs, [altcorrect_3], ERR_ARG, "coarse_altcorrect must be 0, 1 or 2"),
    "altitude correction without its dtms": (coarse_inputs, [altcorrect_without_dtms], ERR_ARG,
                                             "altitude correction needs coarse_dtm and fine_dtm"),
    "coarse forcing below ground with complete = 0": (coarse_inputs, [coarse_below_incomplete], ERR_ARG,
                                                      "coarse array forcing: reqhgt < 0 needs complete = 1"),
    "a missing vegetation plane": (vector_inputs, [missing_pai], ERR_ARG, "missing input array: pai"),
    "a missing soil plane": (vector_inputs, [missing_Vq], ERR_ARG, "missing input array: Vq"),
    "a missing forcing array": (vector_inputs, [missing_swdown], ERR_ARG, "missing forcing array: swdown"),
    "missing winddir": (vector_inputs, [missing_winddir], ERR_ARG, "missing forcing array: winddir"),
    "missing pointm$Tg below ground": (below_incomplete, [missing_Tg], ERR_ARG, "missing input array: pointm$Tg"),
    # two faults: the one that set-up meets first
    "vegetation plane before forcing array": (vector_inputs, [missing_swdown, missing_pai], ERR_ARG, "missing input array: pai"),
    "coarse_rowpos before coarse_altcorrect": (lambda: coarse_inputs(bad_rowpos()), [altcorrect_3], ERR_ARG, ROWPOS_RANGE),
    "row_pitch before soil plane": (vector_inputs, [missing_Vq, pitch_too_small], ERR_ARG, PITCH),
}


@pytest.mark.parametrize("name", list(CASES))
def test_plan_create_refuses(name):
    make, faults, code, sentence = CASES[name]
    lib = _abi.load()
    m = make()
    for fault in faults:
        fault(m)
    p = C.c_void_p()
    status = lib.mcf_plan_create(C.byref(m.inputs), C.byref(m.options), 1, 1, C.byref(p))
    msg = lib.mcf_last_error().decode()
    print(f"{name}: status {status}, message {msg!r}")
    try:
        assert (status, msg) == (code, sentence)
        assert not p.value
    finally:
        if p.value:
            lib.mcf_plan_destroy(p)


def test_the_inputs_are_good_without_the_faults():
    """(the table's refusals are the faults', not the inputs')"""
    lib = _abi.load()
    for make in (vector_inputs, coarse_inputs, below_incomplete):
        m = make()
        p = C.c_void_p()
        assert lib.mcf_plan_create(C.byref(m.inputs), C.byref(m.options), 1, 1, C.byref(p)) == 0, lib.mcf_last_error().decode()
        lib.mcf_plan_destroy(p)
