"""Cases and checks shared by tests/test_vegprep_cpu.py (host entries) and tests/test_vegprep_gpu.py (device entries): the
library's find_lref / find_gref / fill_na / leafrfromalb against the yardstick of tests/vegprep_ref.py.

The parity bar.  Bisection results are dyadic combinations of the bracket ends, so an entry and the yardstick agree bit for
bit unless a root test |f_mid| < tol falls differently.  E is the largest absolute error of the residual against its
np.longdouble evaluation over every point the yardstick evaluates in the solve and fused cases below, taken for the yardstick and for
each entry under test (mcf_selftest_vegprep); a cell is fragile for a call when its smallest | |f_mid| - tol | is below
64 max(E).  Non-fragile cells must be bit-equal, fragile ones may also hold the yardstick's result with that one test taken
the other way, and at most 1 % of the cells with data may be fragile.  The seeds below were chosen on the CPU so that the
yardstick flags no cell at all (seeds: solve 100, 100, 100, 100, 106, 104; fused 213, 201, 219, 227, 202, 204)."""
import functools

import numpy as np

import vegprep_ref as R
from microclimf_amd import vegprep as V

FRAGILE_FACTOR = 64.0


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- per-cell solves -----------------------------------------------------------------------------------------------------------
def _start(pai, x, alb):
    with np.errstate(all="ignore"):
        return (x * 0 + 0.5) * (1 - 0.5) + 0.5 * alb, x * 0 + 0.15


def _solve_cases():
    cases = {}

    def add(name, pai, x, alb, ltrr=0.5, lref=None, gref=None):
        l0, g0 = _start(pai, x, alb)
        cases[name] = dict(pai=pai, x=x, alb=alb, ltrr=ltrr, lref=l0 if lref is None else lref, gref=g0 if gref is None else gref)

    add("1x1", *R.synthetic(1, 1, 2.0, 100, na=0.0, zero_pai=0.0))
    add("1x130", *R.synthetic(1, 130, 2.0, 100))
    add("130x1", *R.synthetic(130, 1, 0.5, 100))
    pai, x, alb = R.synthetic(37, 29, 2.0, 100)
    assert (x == 1.0).any() and (pai == 0.0).any()
    add("37x29", pai, x, alb)
    add("37x29_ltrr1", pai, x, alb, ltrr=1.0)
    p2 = pai.copy()
    p2[5, :] = np.nan
    add("na_row", p2, x, alb)
    add("all_na", np.full((6, 5), np.nan), np.full((6, 5), np.nan), np.full((6, 5), np.nan))
    a2 = alb.copy()
    a2[::3, ::4] = 0.99                      # above anything the bracket reaches
    add("bright", pai, x, a2)
    add("64x64", *R.synthetic(64, 64, 1.0, 106))
    add("64x64_ltrr1", *R.synthetic(64, 64, 1.0, 106), ltrr=1.0)
    # an albedo that is the model's own output for a known leaf reflectance over a known ground
    pai, x, _ = R.synthetic(20, 17, 2.0, 104, na=0.0)
    lref, gref = np.full(pai.shape, 0.3), np.full(pai.shape, 0.2)
    add("own_albedo", pai, x, R.leafr(lref, pai, gref, x, np.zeros(pai.shape), 0.5), lref=lref, gref=gref)
    return cases


SOLVE_CASES = _solve_cases()
WHICH = ("lref", "gref")


@functools.lru_cache(maxsize=None)
def solve_reference(name, which):
    """(yardstick raster, margins, steps, trace) of one case, computed once"""
    c = SOLVE_CASES[name]
    tr = R.Trace()
    if which == "lref":
        r = R.find_lref(c["pai"], c["gref"], c["x"], c["alb"], c["ltrr"], tr)
    else:
        r = R.find_gref(c["lref"], c["pai"], c["x"], c["alb"], c["ltrr"], tr)
    for a in r:
        a.setflags(write=False)
    return r + (tr,)


@functools.lru_cache(maxsize=None)
def residual_errors(device):
    """E of the yardstick and of the entry's unit (host: device None) over every point the yardstick evaluates in the solve
    cases and in the fused cases"""
    e_yard = e_entry = 0.0
    traces = [(solve_reference(name, which)[3], SOLVE_CASES[name]["ltrr"]) for name in SOLVE_CASES for which in WHICH]
    traces += [(fused_reference(name)["trace"], FUSED_CASES[name][4]) for name in FUSED_CASES]
    for tr, ltrr in traces:
        if not tr.points:
            continue
        e_yard = max(e_yard, tr.E)
        *pts, ld = tr.stacked()
        err = np.abs(V.selftest_residual(*pts, ltrr, device=device).astype(np.longdouble) - ld)
        err = err[np.isfinite(err)]
        if err.size:
            e_entry = max(e_entry, float(err.max()))
    return e_yard, e_entry


def bar(devices):
    """64 max(E) over the yardstick and the entries under test"""
    es = [residual_errors(d) for d in devices]
    return FRAGILE_FACTOR * max(max(e) for e in es)


def check_solve(name, which, device, devices):
    c = SOLVE_CASES[name]
    want, margin, step, _ = solve_reference(name, which)
    if which == "lref":
        got = V.find_lref(c["pai"], c["gref"], c["x"], c["alb"], c["ltrr"], device=device)
    else:
        got = V.find_gref(c["lref"], c["pai"], c["x"], c["alb"], c["ltrr"], device=device)
    limit = bar(devices)
    data = ~(np.isnan(c["pai"]) | np.isnan(c["x"]) | np.isnan(c["alb"]) | np.isnan(c["gref" if which == "lref" else "lref"]))
    fragile = data & (margin < limit)
    print(f"{name} {which}: bar {limit:.3e}, smallest margin {margin.min():.3e}, fragile {int(fragile.sum())} of {int(data.sum())}")
    assert fragile.sum() <= 0.01 * data.sum()
    nan_got = np.isnan(got)
    assert (bits(got)[nan_got] == R.NA_BITS).all(), "NA cells must hold R's NA_real_"
    firm = ~fragile
    assert np.array_equal(nan_got[firm], np.isnan(want)[firm])
    assert np.array_equal(bits(np.where(nan_got, 0.0, got))[firm], bits(np.where(np.isnan(want), 0.0, want))[firm])
    if fragile.any():
        flip = np.where(fragile, step, -1)
        if which == "lref":
            alt = R.find_lref(c["pai"], c["gref"], c["x"], c["alb"], c["ltrr"], flip=flip)[0]
        else:
            alt = R.find_gref(c["lref"], c["pai"], c["x"], c["alb"], c["ltrr"], flip=flip)[0]
        g = np.where(nan_got, -1.0, got)
        ok = (bits(g) == bits(np.where(np.isnan(want), -1.0, want))) | (bits(g) == bits(np.where(np.isnan(alt), -1.0, alt)))
        assert ok[fragile].all()
    return got


def check_solve_contents(name, which, got):
    """what the special cases are there for, beside parity"""
    c = SOLVE_CASES[name]
    if name == "all_na":
        assert np.isnan(got).all()
    if name == "na_row":
        assert np.isnan(got[5, :]).all() and not np.isnan(got).all()
    if name == "bright":
        hit = np.zeros(got.shape, dtype=bool)
        hit[::3, ::4] = True
        hit &= ~(np.isnan(c["pai"]) | np.isnan(c["x"]) | np.isnan(c["alb"]))
        assert hit.any()
        if which == "gref":
            assert np.isnan(got[hit]).all()                       # solve_gref: NA
        else:
            lit = hit & (c["pai"] > 0)
            assert np.all(np.abs(got[lit] - R.LREF[1]) < 1e-12)   # solve_lref: the bracket end
    if name == "own_albedo":
        if which == "lref":
            res = R.leafr(got, c["pai"], c["gref"], c["x"], c["alb"], c["ltrr"])
            deep = c["pai"] > 1.0             # (a thin canopy's albedo hardly depends on its leaves)
            assert np.all(np.abs(res) < R.TOL) and deep.any() and np.all(np.abs(got[deep] - 0.3) < 1e-3)
        else:
            res = R.leafr(c["lref"], c["pai"], got, c["x"], c["alb"], c["ltrr"])
            ok = ~np.isnan(got)
            assert ok.mean() > 0.5 and np.all(np.abs(res[ok]) < R.TOL)


# ---- nearest fill -----------------------------------------------------------------------------------------------------------------
def _fill_cases():
    nan = np.nan
    cases = {}
    m = np.full((1, 70), nan)
    m[0, 0] = 5.0
    cases["strip_depth_69"] = (m, np.ones((1, 70)))
    m = np.full((70, 1), nan)
    m[69, 0] = 7.0
    cases["strip_from_the_far_end"] = (m, np.ones((70, 1)))
    m = np.arange(21.0 * 21.0).reshape(21, 21) + 0.5
    m[6:15, 6:15] = nan
    cases["hole_9x9_in_21x21"] = (m, np.ones((21, 21)))
    # two sources next to one NA cell, every pair of the four neighbours; the rest of the raster is outside the mask
    nbs = {"up": (0, 1), "down": (2, 1), "left": (1, 0), "right": (1, 2)}
    names = list(nbs)
    for i in range(4):
        for j in range(i + 1, 4):
            m = np.full((3, 3), nan)
            mask = np.full((3, 3), nan)
            mask[1, 1] = 1.0
            for k, v in ((names[i], 10.0), (names[j], 20.0)):
                m[nbs[k]] = v
                mask[nbs[k]] = 1.0
            cases[f"tie_{names[i]}_{names[j]}"] = (m, mask)
            # the same two directions two cells away, every cell inside the mask
            m = np.full((5, 5), nan)
            for k, v in ((names[i], 10.0), (names[j], 20.0)):
                r, c = nbs[k]
                m[2 * r, 2 * c] = v
            cases[f"tie2_{names[i]}_{names[j]}"] = (m, np.ones((5, 5)))
    # a wall outside the mask: (3, 3) is two cells from the source behind the wall and ten steps from it around the wall
    m = np.full((7, 9), nan)
    mask = np.ones((7, 9))
    mask[0:6, 4] = nan
    m[3, 5] = 1.0
    m[3, 0] = 2.0
    cases["wall"] = (m, mask)
    # an island inside the mask, cut off by cells outside it, with no source
    m = np.arange(81.0).reshape(9, 9)
    mask = np.ones((9, 9))
    mask[2, 2:7] = mask[6, 2:7] = mask[2:7, 2] = mask[2:7, 6] = nan
    m[3:6, 3:6] = nan
    cases["island"] = (m, mask)
    # a cell outside the mask that holds a value: kept, no source, no path
    m = np.full((3, 5), nan)
    mask = np.ones((3, 5))
    mask[:, 2] = nan
    m[1, 2] = 99.0
    m[1, 0] = 3.0
    cases["value_outside_the_mask"] = (m, mask)
    cases["no_holes"] = (np.arange(35.0).reshape(5, 7), np.ones((5, 7)))
    cases["no_sources"] = (np.full((6, 4), nan), np.ones((6, 4)))
    rng = np.random.default_rng(31)
    for rows, cols, holes in ((37, 29, 0.3), (64, 64, 0.9), (130, 3, 0.5), (300, 270, 0.05)):
        m = rng.normal(size=(rows, cols))
        m[rng.random((rows, cols)) < holes] = nan
        mask = np.ones((rows, cols))
        mask[rng.random((rows, cols)) < 0.1] = nan
        cases[f"random_{rows}x{cols}"] = (m, mask)
    return cases


FILL_CASES = _fill_cases()


@functools.lru_cache(maxsize=None)
def fill_reference(name):
    r = R.fill_na(*FILL_CASES[name])
    r.setflags(write=False)
    return r


def check_fill(name, device):
    m, mask = FILL_CASES[name]
    want = fill_reference(name)
    got = V.fill_na(m, mask, device=device)
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())     # NaN payloads included
    if name == "wall":
        assert got[3, 3] == 2.0
    if name == "island":
        assert np.isnan(got[3:6, 3:6]).all()
    if name == "value_outside_the_mask":
        assert got[1, 2] == 99.0 and np.isnan(got[:, 3:]).all() and (got[:, :2] == 3.0).all()
    if name == "strip_depth_69":
        assert (got == 5.0).all()


# ---- the fused loop ---------------------------------------------------------------------------------------------------------------
FUSED_CASES = {                      # rows, cols, mean pai, seed, ltrr, share of NA per input
    "24x20_leaf_first": (24, 20, 2.0, 213, 0.5, 0.05),
    "24x20_ground_first": (24, 20, 0.5, 201, 0.5, 0.05),
    "37x29_leaf_first": (37, 29, 2.0, 219, 0.5, 0.05),
    "37x29_ground_first": (37, 29, 0.5, 227, 0.5, 0.05),
    "24x20_ltrr1": (24, 20, 2.0, 202, 1.0, 0.05),
    "24x20_many_holes": (24, 20, 2.0, 204, 0.5, 0.15),
}


def fused_inputs(name):
    rows, cols, mean_pai, seed, ltrr, na = FUSED_CASES[name]
    return R.synthetic(rows, cols, mean_pai, seed, na=na) + (ltrr,)


@functools.lru_cache(maxsize=None)
def fused_reference(name):
    pai, x, alb, ltrr = fused_inputs(name)
    tr = R.Trace()
    r = R.leafrfromalb(pai, x, alb, ltrr, tr)
    r["trace"] = tr
    return r


def check_fused(name, device, devices, run=None):
    pai, x, alb, ltrr = fused_inputs(name)
    want = fused_reference(name)
    limit = bar(devices)
    print(f"{name}: bar {limit:.3e}, smallest margin {min(want['margins']):.3e}, passes {want['iterations']}, filled {want['filled']}, "
          f"tst {want['tst']:.4f}, last mxdif {want['history'][-1]:.3e}")
    # the case is one the bar says must be equal: no fragile cell in any pass, no decision of the loop near its threshold
    assert min(want["margins"]) >= limit
    assert all(abs(h - 0.001) > 1e-6 for h in want["history"]) and abs(want["tst"] - 0.5) > 1e-6
    assert want["lref_first"] == ("leaf_first" in name or "ltrr1" in name or "holes" in name)
    assert all(f > 0 for f in want["filled"]), "the fill must have work in every pass"
    got = (run or V.leafrfromalb)(pai, x, alb, ltrr, device=device)
    assert got["iterations"] == want["iterations"] and got["lref_first"] == want["lref_first"]
    for k in ("leafr", "leaft", "gref"):
        nan_got = np.isnan(got[k])
        assert np.array_equal(nan_got, np.isnan(want[k])), k
        assert (bits(got[k])[nan_got] == R.NA_BITS).all(), k
        assert np.array_equal(bits(np.where(nan_got, 0.0, got[k])), bits(np.where(nan_got, 0.0, want[k]))), k
    for k in ("mxdif_gref", "mxdif_leaf"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    return got
