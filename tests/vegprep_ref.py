"""Yardstick of the vegetation pre-compute tests: a plain numpy / Python restatement of leafrcpp, solve_lref, solve_gref,
find_lref, find_gref, fill_naCpp (reference src/microclimfCpp.cpp:5594-5777) and of the loop of leafrfromalb()
(R/dataprep.R:1007-1049), written from the equations in the reference's operation order.  Nothing is hoisted: f_lower is
evaluated again at every step and all 100 steps run; the fill is a literal FIFO queue.

Beside the values it returns what the parity bar needs (tests/test_vegprep_*.py):
  * per cell the smallest | |f_mid| - tol | over the steps the cell was still searching, and the step it occurred at: how far
    the nearest root test was from flipping (the initial f_lower's distance from zero counts as well);
  * the largest |residual in float64 - residual in np.longdouble| over every evaluation made, and the evaluation points, so
    that the library's own residual can be measured on the same points.
Cells are vectorised; the steps are not."""
from collections import deque

import numpy as np

TOL = 1e-6
MAX_ITER = 100
LREF = (0.0001, 0.6665)
GREF = (0.0001, 0.9999)
PI = 3.14159265358979323846
NA_BITS = 0x7FF00000000007A2


def leafr(lref, pai, gref, x, albin, ltrr, t=np.float64):
    """leafrcpp (cpp:5594-5626) elementwise in number type `t`"""
    lref, pai, gref, x, albin = (np.asarray(v, dtype=np.float64).astype(t) for v in (lref, pai, gref, x, albin))
    ltrr = t(ltrr)
    with np.errstate(all="ignore"):
        ltra = ltrr * lref
        om = lref + ltra
        a = 1 - om
        de = lref - ltra
        mla = t(9.65) * np.power(3 + x, t(-1.65))
        mla = np.where(mla > t(PI) / 2, t(PI) / t(2.0), mla)
        J = np.where(x != 1.0, np.cos(mla) * np.cos(mla), t(1.0 / 3.0)).astype(t)
        gma = t(0.5) * (om + J * de)
        h = np.sqrt(a * a + 2 * a * gma)
        S1 = np.exp(-h * pai)
        u1 = a + gma * (1 - 1 / gref)
        D1 = (a + gma + h) * (u1 - h) * 1 / S1 - (a + gma - h) * (u1 + h) * S1
        p1 = (gma / (D1 * S1)) * (u1 - h)
        p2 = (-gma * S1 / D1) * (u1 + h)
        albd = p1 + p2
        return albd - albin


class Trace:
    """what the parity bar is made of, collected over every bisection run with it"""

    def __init__(self, keep_points=True):
        self.E = 0.0                    # max |float64 - longdouble| of the residual
        self.points = []                # (lref, pai, gref, x, albin) arrays of every evaluation, when kept
        self.keep_points = keep_points

    def see(self, f64, args, ltrr, act):
        """the evaluations of the cells still searching (`act`)"""
        if not act.any():
            return
        args = tuple(np.array(a[act], dtype=np.float64) for a in args)
        ld = leafr(*args, ltrr, t=np.longdouble)
        err = np.abs(f64[act].astype(np.longdouble) - ld)
        ok = np.isfinite(err)
        if ok.any():
            self.E = max(self.E, float(err[ok].max()))
        if self.keep_points:
            self.points.append(args + (ld,))

    def stacked(self):
        """(lref, pai, gref, x, albin, residual in longdouble) over everything seen"""
        return tuple(np.concatenate([p[k] for p in self.points]) for k in range(6))


def _bisect(f, bracket, n, na_on_fail, flip=None):
    """the loop of solve_lref (cpp:5629-5648) / solve_gref (cpp:5652-5672) over n cells; `flip`: per cell the step whose root
    test is taken the other way, -1 for none.  -> result, margin, step of the margin"""
    lower = np.full(n, bracket[0])
    upper = np.full(n, bracket[1])
    mid = np.zeros(n)
    res = np.full(n, np.nan)
    done = np.zeros(n, dtype=bool)
    margin = np.full(n, np.inf)
    mstep = np.full(n, -1)
    with np.errstate(all="ignore"):
        for it in range(MAX_ITER):
            act = ~done
            if not act.any():
                break
            mid = np.where(act, (lower + upper) / 2.0, mid)
            f_lower = f(lower, act if it == 0 else None)
            f_mid = f(mid, act)
            mg = np.abs(np.abs(f_mid) - TOL)
            if it == 0:                       # the sign of the first f_lower matters once the first root test has failed
                mg = np.where(np.abs(f_mid) < TOL, mg, np.fmin(mg, np.abs(f_lower)))
            mg = np.where(np.isnan(mg), np.inf, mg)
            closer = act & (mg < margin)
            margin[closer] = mg[closer]
            mstep[closer] = it
            root = np.abs(f_mid) < TOL
            if flip is not None:
                root = np.where(flip == it, ~root, root)
            root &= act
            res[root] = mid[root]
            done |= root
            act = ~done
            neg = f_lower * f_mid < 0
            upper = np.where(act & neg, mid, upper)
            lower = np.where(act & ~neg, mid, lower)
    if not na_on_fail:
        res[~done] = mid[~done]
    return res, margin, mstep


def _solve(which, first, second, x, albin, ltrr, trace=None, flip=None):
    """which = "lref": first = pai, second = gref; "gref": first = lref, second = pai.  Rasters of one shape."""
    shape = np.shape(first)
    first, second, x, albin = (np.asarray(v, dtype=np.float64).ravel() for v in (first, second, x, albin))
    ok = ~(np.isnan(first) | np.isnan(second) | np.isnan(x) | np.isnan(albin))
    a, b, xx, al = first[ok], second[ok], x[ok], albin[ok]

    def f(u, act):
        args = (u, a, b, xx, al) if which == "lref" else (a, b, u, xx, al)
        v = leafr(*args, ltrr)
        if trace is not None and act is not None:
            trace.see(v, args, ltrr, act)
        return v

    r, mg, st = _bisect(f, LREF if which == "lref" else GREF, int(ok.sum()), which == "gref",
                        None if flip is None else np.asarray(flip).ravel()[ok])
    out = np.full(first.shape, np.nan)
    margin = np.full(first.shape, np.inf)
    step = np.full(first.shape, -1)
    out[ok], margin[ok], step[ok] = r, mg, st
    return out.reshape(shape), margin.reshape(shape), step.reshape(shape)


def find_lref(pai, gref, x, albin, ltrr, trace=None, flip=None):
    return _solve("lref", pai, gref, x, albin, ltrr, trace, flip)


def find_gref(lref, pai, x, albin, ltrr, trace=None, flip=None):
    return _solve("gref", lref, pai, x, albin, ltrr, trace, flip)


def fill_na(m, mask):
    """fill_naCpp (cpp:5727-5777), the queue included"""
    m = np.array(m, dtype=np.float64, order="F")
    mask = np.asarray(mask, dtype=np.float64)
    nrow, ncol = m.shape
    src = -np.ones(nrow * ncol, dtype=np.int64)
    q = deque()
    for j in range(ncol):
        for i in range(nrow):
            if np.isnan(mask[i, j]):
                continue
            if not np.isnan(m[i, j]):
                src[i + nrow * j] = i + nrow * j
                q.append(i + nrow * j)
    dr, dc = (-1, 1, 0, 0), (0, 0, -1, 1)
    while q:
        cur = q.popleft()
        r, c = cur % nrow, cur // nrow
        for k in range(4):
            rr, cc = r + dr[k], c + dc[k]
            if rr < 0 or rr >= nrow or cc < 0 or cc >= ncol or np.isnan(mask[rr, cc]):
                continue
            nb = rr + nrow * cc
            if src[nb] == -1:
                src[nb] = src[cur]
                q.append(nb)
    for j in range(ncol):
        for i in range(nrow):
            if np.isnan(mask[i, j]) or not np.isnan(m[i, j]):
                continue
            s = src[i + nrow * j]
            if s != -1:
                m[i, j] = m[s % nrow, s // nrow]
    return m


def leafrfromalb(pai, x, alb, ltrr=0.5, trace=None):
    """the loop of R/dataprep.R:1005-1049 -> the three rasters, the bookkeeping, and per pass the smallest margin of its two
    solves and how many cells its two fills filled"""
    pai, x, alb = (np.asarray(v, dtype=np.float64) for v in (pai, x, alb))
    with np.errstate(all="ignore"):
        tst = float(np.exp(-np.nanmean(pai)))
        lref = (x * 0 + 0.5) * (1 - 0.5) + 0.5 * alb
        gref = x * 0 + 0.15
    tol, maxiter = 0.001, 50
    mxdif = tol * 10
    itr, passes = 1, 0
    margins, filled, history = [], [], []
    while mxdif > tol:
        if tst < 0.5:
            l0, m1, _ = find_lref(pai, gref, x, alb, ltrr, trace)
            lref2 = fill_na(l0, x)
            g0, m2, _ = find_gref(lref2, pai, x, alb, ltrr, trace)
            gref2 = fill_na(g0, x)
        else:
            g0, m1, _ = find_gref(lref, pai, x, alb, ltrr, trace)
            gref2 = fill_na(g0, x)
            l0, m2, _ = find_lref(pai, gref2, x, alb, ltrr, trace)
            lref2 = fill_na(l0, x)
        filled.append(int((np.isnan(l0) & ~np.isnan(lref2)).sum() + (np.isnan(g0) & ~np.isnan(gref2)).sum()))
        margins.append(float(min(m1.min(), m2.min())))
        gref = 0.5 * gref + 0.5 * gref2
        lref = 0.5 * lref + 0.5 * lref2
        with np.errstate(all="ignore"):
            mxdif1 = float(np.nanmean(np.abs(gref - gref2)))
            mxdif2 = float(np.nanmean(np.abs(lref - lref2)))
        mxdif = max(mxdif1, mxdif2)
        history.append(mxdif)
        passes += 1
        itr += 1
        if itr > maxiter:
            mxdif = 0
    return {"leafr": lref, "leaft": ltrr * lref, "gref": gref, "iterations": passes, "mxdif_gref": mxdif1,
            "mxdif_leaf": mxdif2, "lref_first": tst < 0.5, "tst": tst, "margins": margins, "filled": filled, "history": history}


def synthetic(rows, cols, mean_pai, seed, na=0.05, zero_pai=0.05):
    """the issue's settings: gamma-distributed pai, x in 0.3..3 with 10 % exact ones, alb in 0.05..0.4, about 5 % NA in each,
    5 % pai = 0"""
    rng = np.random.default_rng(seed)
    pai = rng.gamma(2.0, mean_pai / 2.0, (rows, cols))
    pai[rng.random((rows, cols)) < zero_pai] = 0.0
    x = rng.uniform(0.3, 3.0, (rows, cols))
    x[rng.random((rows, cols)) < 0.10] = 1.0
    alb = rng.uniform(0.05, 0.4, (rows, cols))
    for a in (pai, x, alb):
        a[rng.random((rows, cols)) < na] = np.nan
    return pai, x, alb
