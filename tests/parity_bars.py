"""Per-case, per-variable bars of the GPU-against-oracle comparisons, derived from the reference side only.

How far apart may two CORRECT fp64 evaluations of a workload lie?  The oracle is asked: it is built three more times with
legitimate rounding perturbations (oracle/variants/: `fma` contracts a*b+c, `ulp` moves every result of the ten libm
functions the device replaces by -2..+2 ulp, `ulpfma` does both), the same inputs are run, and the spread

    N[var] = max over the noise variants of d(variant, oracle),   d(x, y) = max |x - y| / (1 + |y|)

is a property of the problem, not of the kernel.  The bar of a comparison is

    bar[var] = min(CAP, max(FLOOR, K * N[var]))

CAP = 1e-6 is what every comparison asserted before bars were derived: no assertion can get weaker than it was.
FLOOR = 2^-40: the kernels use, by design, quotients bounded at 2^-44 relative (tests/test_math_gpu.py, frcp2_m) directly in
Penman-Monteith temperatures and series conductances; sixteen of them in a row are allowed.
K = 16: the noise variants perturb the libm families and the contraction; the kernels legitimately differ in more places
(every division, reciprocal and square root, reassociation from hoisting, the order of daily means), so their distance
is expected to be a small multiple of N.  Four bits of headroom still leave three orders and more to the faintest
single-precision slip (tests/test_parity_bars_cpu.py asserts >= 100x for every case; profiles/parity_bars_cpu.txt has the
figures), so the choice is not delicate.

K and FLOOR live here and nowhere else.  They are NOT adjusted to make a GPU run pass: a kernel beyond its bar is a finding
("Tolerance").  There is no table of exceptions because no (case, variable) pair needs one: the kernels
lie at most 0.15 bars from the oracle (profiles/parity_margins_gpu.txt).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

K = 16.0
FLOOR = 2.0 ** -40
CAP = 1e-6
NA_BITS = 0x7FF00000000007A2

_cache = {}


def distance(x, y):
    """max |x - y| / (1 + |y|) over the elements finite in both: the metric of compare / assert_close"""
    fin = np.isfinite(x) & np.isfinite(y)
    if not fin.any():
        return 0.0
    return float((np.abs(x[fin] - y[fin]) / (1.0 + np.abs(y[fin]))).max())


def same_pattern(x, y):
    return (x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y))
            and np.array_equal(np.isfinite(x), np.isfinite(y)))


def run_variants(O, run, names):
    """`run(lib) -> {variable: array}` under the default oracle (lib=None) and each named variant build.  Every build is a
    library of its own, so they run side by side; a variant this host cannot execute raises (oracle.load_variant)."""
    libs = [None] + [O.load_variant(v) for v in names]
    with ThreadPoolExecutor(len(libs)) as pool:
        res = list(pool.map(run, libs))
    return res[0], dict(zip(names, res[1:]))


def distances(want, other, what=""):
    """d per variable; the NaN / inf pattern must be the oracle's (a case on a discontinuity needs a written decision,
    never a silent exclusion)"""
    assert list(other) == list(want), what
    out = {}
    for k, w in want.items():
        assert same_pattern(other[k], w), f"{what}{k}: NaN / inf pattern differs from the oracle's"
        out[k] = distance(other[k], w)
    return out


def bar_of(noise):
    return min(CAP, max(FLOOR, K * noise))


def bars_for(O, run, key=None):
    """(want, bars, N) of a workload: the oracle's output, the bar and the noise per variable.  `key` (a case name, a draw
    index) keeps the result for the session: parametrisations that solve the same inputs pay the variant runs once."""
    if key is not None and key in _cache:
        return _cache[key]
    want, var = run_variants(O, run, O.NOISE_VARIANTS)
    noise = {k: 0.0 for k in want}
    for v, res in var.items():
        for k, d in distances(want, res, f"noise variant {v}: ").items():
            noise[k] = max(noise[k], d)
    out = (want, {k: bar_of(n) for k, n in noise.items()}, noise)
    if key is not None:
        _cache[key] = out
    return out


def grid(O, a, array_forcing=False, key=None):
    """(want, bars) of oracle.run_grid(**a, array_forcing=...)"""
    return bars_for(O, lambda lib: O.run_grid(**a, array_forcing=array_forcing, lib=lib), key)[:2]


def snowmodel(O, margs, array_forcing=False, key=None):
    """(want, bars) of oracle.run_snowmodel(**margs, array_forcing=...)"""
    return bars_for(O, lambda lib: O.run_snowmodel(**margs, array_forcing=array_forcing, lib=lib), key)[:2]


def microsnow(O, args, array_forcing=False, key=None):
    """(want, bars) of oracle.run_microsnow(*args, array_forcing=...)"""
    return bars_for(O, lambda lib: O.run_microsnow(*args, array_forcing=array_forcing, lib=lib), key)[:2]


def compare(got, want, bars=None, *, tol=None):
    """Same variables in the reference's order, same shapes, identical NaN / inf patterns, R's NA payload where the oracle
    has it, and every finite value within bars[variable] * (1 + |x|).  A comparison that has no derived bars says so:
    `tol=` spelled out, one number for every variable — there is no default to fall back to by omission."""
    if (bars is None) == (tol is None):
        raise TypeError("compare() takes either per-variable bars or an explicit tol=")
    assert list(got) == list(want)            # same variables, same (reference) order
    worst = {}
    for k, w in want.items():
        g = got[k]
        bar = tol if bars is None else bars[k]
        assert bar <= CAP, (k, bar)
        assert g.shape == w.shape, k
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{k}: NA pattern differs"
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), fin), f"{k}: inf pattern differs"
        err = np.abs(g[fin] - w[fin]) / (1.0 + np.abs(w[fin]))
        worst[k] = float(err.max()) if err.size else 0.0
        assert worst[k] <= bar, f"{k}: max scaled error {worst[k]:.3e} > bar {bar:.3e}"
        na = np.isnan(w) & (w.view(np.uint64) == NA_BITS)
        if na.any():                          # NA cells / steps carry R's NA_real_ payload, not just any NaN
            assert (g[na].view(np.uint64) == NA_BITS).all(), k
    return worst


def slips_for(O, run, want):
    """S[slip][variable]: distance of each slip variant from the oracle; inf where the slip changes the NaN / inf pattern
    (the comparator refuses that outright)"""
    _, var = run_variants(O, run, O.SLIP_VARIANTS)
    return {v: {k: (distance(res[k], w) if same_pattern(res[k], w) else float("inf")) for k, w in want.items()}
            for v, res in var.items()}


def case_sets(O, sets=("cases", "random", "snowmodel", "microsnow")):
    """The workloads whose bars are certified on the CPU (tests/test_parity_bars_cpu.py) and recorded
    (tools/parity_margins.py): yields (set, label, run, inputs) with run(lib) -> {variable: array}; `inputs` is what the
    device entry needs to solve the same thing.  `snowfast1` / `snowfast2` (the oracle chains of tests/snowfast_cases.py, on
    terrain_oracle's terrain; certified by tests/test_snowfast_bars_cpu.py) are not in the default tuple."""
    from microclimf_amd import synthetic
    import parity_cases as PC
    import snow_cases as SC
    if "cases" in sets:
        for name in sorted(PC.CASES):
            a, af = PC.build(name)
            yield ("cases", name, (lambda lib, a=a, af=af: O.run_grid(**a, array_forcing=af, lib=lib)),
                   dict(kind="grid", a=a, af=af, extra={}))
    if "random" in sets:
        for i in range(96):
            rows, cols, T, kw, extra = PC.draw(i)
            a = synthetic.workload(rows, cols, T, **kw)
            af = kw["array_forcing"]
            yield ("random", f"draw{i:02d}", (lambda lib, a=a, af=af: O.run_grid(**a, array_forcing=af, lib=lib)),
                   dict(kind="grid", a=a, af=af, extra=extra))
    if "snowmodel" in sets or "microsnow" in sets:
        for name in sorted(SC.SNOW_CASES):
            sw, af = SC.build_snow(name)
            margs = SC.model_args(sw)
            if "snowmodel" in sets:
                yield ("snowmodel", name, (lambda lib, m=margs, af=af: O.run_snowmodel(**m, array_forcing=af, lib=lib)),
                       dict(kind="snowmodel", sw=sw, af=af))
            if "microsnow" in sets:
                smod = O.run_snowmodel(**margs, array_forcing=af)
                snowm, micro = SC.microsnow_state(sw, smod)
                for h in SC.MICRO_HEIGHTS:
                    args = (h, sw["obstime"], sw["climdata"], snowm, micro, sw["vegp"], sw["other"], 3.0, [1] * 10)
                    yield ("microsnow", f"{name}@{h:g}",
                           (lambda lib, args=args, af=af: O.run_microsnow(*args, array_forcing=af, lib=lib)),
                           dict(kind="microsnow", args=args, af=af))
    for kind, n in (("snowfast1", "q1"), ("snowfast2", "q2")):
        if kind in sets:
            import snowfast_cases as FC
            for i in range(len(FC.Q1_CASES if n == "q1" else FC.Q2_CASES)):
                c = (FC.q1_case if n == "q1" else FC.q2_case)(i)
                yield (kind, f"case{i}", FC.run(O, c), dict(kind=kind, index=i, case=c))
