"""Device entries of the vegetation pre-compute (mcf_find_lref_device, mcf_find_gref_device, mcf_fill_na_device,
mcf_leafrfromalb_device; mcf_vegprep.hip) against the yardstick of tests/vegprep_ref.py under the parity bar of
tests/vegprep_cases.py, and against the host entries: bit-equal wherever the bar flags no fragile cell."""
import numpy as np
import pytest

import vegprep_cases as VC
from microclimf_amd import vegprep as V

pytestmark = pytest.mark.gpu
BOTH = (None, 0)        # the entries whose residual error enters the bar: the host unit's and the device unit's


def test_the_bar_is_made_of_measured_errors():
    e_yard, e_host = VC.residual_errors(None)
    _, e_dev = VC.residual_errors(0)
    print(f"E yardstick {e_yard:.3e}, E host entry {e_host:.3e}, E device entry {e_dev:.3e}, bar {VC.bar(BOTH):.3e}")
    assert 0 < e_dev < 1e-11


@pytest.mark.parametrize("which", VC.WHICH)
@pytest.mark.parametrize("name", list(VC.SOLVE_CASES))
def test_solve_equals_the_yardstick_and_the_host(name, which):
    got = VC.check_solve(name, which, 0, BOTH)
    VC.check_solve_contents(name, which, got)
    if VC.solve_reference(name, which)[1].min() >= VC.bar(BOTH):          # no fragile cell: the host entry's bits
        c = VC.SOLVE_CASES[name]
        host = (V.find_lref(c["pai"], c["gref"], c["x"], c["alb"], c["ltrr"], device=None) if which == "lref" else
                V.find_gref(c["lref"], c["pai"], c["x"], c["alb"], c["ltrr"], device=None))
        assert np.array_equal(VC.bits(got), VC.bits(host))


@pytest.mark.parametrize("name", list(VC.FILL_CASES))
def test_fill_equals_the_queue(name):
    VC.check_fill(name, 0)


@pytest.mark.parametrize("name", list(VC.FUSED_CASES))
def test_fused_loop_equals_the_yardstick_and_the_host(name):
    got = VC.check_fused(name, 0, BOTH)
    pai, x, alb, ltrr = VC.fused_inputs(name)
    host = V.leafrfromalb(pai, x, alb, ltrr, device=None)
    for k in ("leafr", "leaft", "gref"):
        assert np.array_equal(VC.bits(got[k]), VC.bits(host[k])), k
    for k in ("iterations", "lref_first", "mxdif_gref", "mxdif_leaf"):      # the sums are taken in one order on both sides
        assert got[k] == host[k], k


def test_fused_loop_does_not_depend_on_the_workgroup_size():
    pai, x, alb, ltrr = VC.fused_inputs("37x29_ground_first")
    a = V.selftest_leafrfromalb(pai, x, alb, ltrr, block=256)
    b = V.selftest_leafrfromalb(pai, x, alb, ltrr, block=64)
    want = V.leafrfromalb(pai, x, alb, ltrr, device=0)
    for r in (a, b):
        for k in ("leafr", "leaft", "gref"):
            assert np.array_equal(VC.bits(r[k]), VC.bits(want[k])), k
        for k in ("iterations", "lref_first", "mxdif_gref", "mxdif_leaf"):
            assert r[k] == want[k], k
