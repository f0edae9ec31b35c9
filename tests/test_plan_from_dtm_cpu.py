"""The entries that take the dtm (include/mcf.h mcf_dtm_spec, ABI 8) without a device: the struct's layout as gcc sees it
against the ctypes mirror, and no quiet fall-back."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from microclimf_amd import _abi, synthetic
from test_terrain_cpu import synth_dtm

ROOT = Path(__file__).resolve().parents[1]


def test_dtm_spec_layout_matches_the_compiled_header(tmp_path):
    fields = [n for n, _ in _abi.DtmSpec._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcf.h"', 'int main(void) {',
           'printf("size %zu\\n", sizeof(mcf_dtm_spec));']
    src += [f'printf("{f} %zu\\n", offsetof(mcf_dtm_spec, {f}));' for f in fields]
    src.append('return 0; }')
    (tmp_path / "probe.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.splitlines() if line)
    assert int(got["size"]) == C.sizeof(_abi.DtmSpec) == 56
    for f in fields:
        assert int(got[f]) == getattr(_abi.DtmSpec, f).offset, f


def test_abi_version_is_8():
    import __graft_entry__ as g
    g.build_library()
    assert _abi.load().mcf_abi_version() == _abi.ABI_VERSION == 8


def test_dtm_entries_have_no_cpu_fallback():
    import __graft_entry__ as g
    g.build_library()
    lib = _abi.load()
    if lib.mcf_device_count() > 0:
        pytest.skip("a GPU is present")
    from microclimf_amd import api
    from microclimf_amd.terrain import flowaccCpp, topidx
    z = synth_dtm(6, 5)
    with pytest.raises(_abi.McfError, match="no HIP device"):
        flowaccCpp(z, device=0)
    with pytest.raises(_abi.McfError, match="no HIP device"):
        topidx(z, 1.0, device=0)
    assert flowaccCpp(z).shape == z.shape                                  # the host code needs none
    a = synthetic.workload(6, 5, 24)
    for k in api.DTM_DERIVED:
        del a["soilc"][k]
    dtm = {"z": z, "res": 1.0}
    with pytest.raises(_abi.McfError, match="no HIP device"):
        api.runmicro1Cpp(**a, dtm=dtm)
    with pytest.raises(_abi.McfError, match="no HIP device"):
        api.runmicro1Cpp(**a, dtm=dtm, devices=[0], n_blocks=2)
    a.pop("device", None)
    with pytest.raises(_abi.McfError, match="no HIP device"):
        api.Plan(**a, dtm=dtm)


def test_missing_planes_without_a_dtm_stay_an_error():
    a = synthetic.workload(4, 4, 24)
    del a["soilc"]["twi"]
    from microclimf_amd.marshal import marshal
    with pytest.raises(KeyError):
        marshal(**a, array_forcing=False)
