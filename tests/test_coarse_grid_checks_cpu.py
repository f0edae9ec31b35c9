"""The entries that take a coarse grid refuse a bad one through one check (mcf_snow.hip coarse_grid_checks): for the same
fault their sentences are the same apart from the entry's name and the microclimate group's tag.  No device is needed."""
import pytest

from microclimf_amd import snow as S
import test_snowfast2_onecall_cpu as Q2
import test_snowmodel2_coarse_cpu as M2
import test_snowrun2_coarse_cpu as R2
from test_snowmodel2_coarse_cpu import MCF_ERR_ARG, R, lib      # noqa: F401

FAULTS = {"coarse_rows = 0": "coarse_rows", "a position at coarse_rows": "coarse_rowpos", "altcorrect = 3": "altcorrect",
          "altcorrect = 1 without coarse_dtm": "coarse_dtm"}


def _spoil(cin, fault):
    if fault == "coarse_rows = 0":
        cin.coarse_rows = 0
    elif fault == "a position at coarse_rows":
        cin.coarse_rowpos[R - 1] = float(cin.coarse_rows)
    elif fault == "altcorrect = 3":
        cin.altcorrect = 3
    else:
        assert cin.altcorrect == 1
        cin.coarse_dtm = None
    return cin


@pytest.mark.parametrize("fault", FAULTS)
def test_the_four_entries_refuse_a_bad_coarse_grid_in_the_same_words(lib, fault):
    alt = 1 if "coarse_dtm" in fault else 0
    mq, fin = S.marshal_snowfast2(*Q2._args(altcorrect=alt))
    mm, cin = M2._marshal(altcorrect=alt)
    mx, xin = M2._marshal(altcorrect=alt)
    run = R2._run(altcorrect=alt)
    got = {"mcf_snowmodelq2": Q2._status(lib, _spoil(fin, fault)),
           "mcf_snowmodel2_coarse": M2._model(lib, _spoil(cin, fault)),
           "mcf_snow_expand_coarse_device": M2._expand(lib, _spoil(xin, fault)),
           "mcf_microsnow_expand_coarse_device": R2._call_expand(lib, _spoil(run._mci, fault))}
    sentences = set()
    for entry, (rc, msg) in got.items():
        assert rc == MCF_ERR_ARG and msg.startswith(entry + ": "), (entry, rc, msg)
        sentence = msg[len(entry) + 2:]
        sentences.add(sentence[len("micro: "):] if entry.startswith("mcf_microsnow") and sentence.startswith("micro: ") else sentence)
    assert len(sentences) == 1 and FAULTS[fault] in next(iter(sentences)), (fault, got)
