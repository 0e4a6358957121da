"""Restatement of evaluateModelFit's measures (R/evaluateModelFit.R:53-169) in np.longdouble and
the error bounds a float64 implementation is held to.  Independent of hmsc_amd.predict: ranks come
from counting, correlations from two passes, every sum in longdouble.

Definitions (Y the data with NaN = NA, m the per-cell mean or -- Poisson -- median, pO the share of
positive draws; per species):

  RMSE (Y, m), O.RMSE (1[Y > 0], pO), C.RMSE (Yc, m / pO)   sqrt of the mean of (a - b)^2 over the
      rows where that term is not NaN; NaN without such a row; an infinite term gives inf.
  R2 (normal), SR2, C.SR2 (Poisson)   sign(co) co^2, co the Pearson correlation (of the average
      ranks for the two Spearman measures) over the pairwise-complete rows, +-inf being complete;
      NaN below 2 rows or at zero variance.
  AUC (probit), O.AUC (Poisson)   (R1 - n1 (n1 + 1) / 2) / (n1 n0) over the rows with Y not NaN,
      classes 1[Y > 0], R1 the positives' average ranks; NaN unless both classes occur, and NaN if
      a selected prediction is NaN.
  TjurR2 (probit: Y == 1 against Y == 0), O.TjurR2 (Y > 0 against the other rows with Y not NaN)
      mean prediction of the first class minus that of the second; NaN for an empty class.
  Yc is Y with 0 -> NaN.

Bounds, u = 2^-53, n the rows used:
  RMSE family   relative (n + 4) u
  Tjur family   per class (n_c - 1) u mean|p| + u |mean|, the two summed, plus u |result| (the
                any-order bound of a sum)
  R2 family     |co - co_ref| <= d = 2 (n + 6) u, so the measure is within 2 |co_ref| d + d^2
                (inputs with |mean| / sd <= 1e3: the second-order term n^2 u^2 kx ky is below it)
  AUC family    none: every intermediate is a half-integer below 2^53, the one division is
                correctly rounded, so float64 results are equal
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
KEYS = ("RMSE", "R2", "AUC", "TjurR2", "SR2", "O.AUC", "O.TjurR2", "O.RMSE", "C.SR2", "C.RMSE")
FAMILY_KEYS = {1: ("R2",), 2: ("AUC", "TjurR2"), 3: ("SR2", "O.AUC", "O.TjurR2", "O.RMSE", "C.SR2", "C.RMSE")}
BOUND_FAMILY = {"RMSE": "rmse", "O.RMSE": "rmse", "C.RMSE": "rmse", "R2": "corr", "SR2": "corr", "C.SR2": "corr",
                "TjurR2": "tjur", "O.TjurR2": "tjur", "AUC": "auc", "O.AUC": "auc"}


def average_ranks(x):
    """(#values < x_i) + (#values == x_i + 1) / 2 by counting (-0.0 == +0.0, +-inf are values); all
    NaN if any value is NaN.  Up to 512 values the counts are taken pair by pair as well."""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any():
        return np.full(x.shape, np.nan)
    s = np.sort(x)
    less = np.searchsorted(s, x, side="left")
    equal = np.searchsorted(s, x, side="right") - less
    if x.size <= 512:
        assert np.array_equal(less, (x[None, :] < x[:, None]).sum(axis=1))
        assert np.array_equal(equal, (x[None, :] == x[:, None]).sum(axis=1))
    return less + (equal + 1) / 2.0


def _rmse(a, b):
    """value, bound"""
    with np.errstate(all="ignore"):
        q = (np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)) ** 2
    q = q[~np.isnan(q)]
    if q.size == 0:
        return LD(np.nan), 0.0
    val = np.sqrt(np.sum(q) / LD(q.size))
    return val, (q.size + 4) * U * float(val) if np.isfinite(val) else 0.0


def _corr(x, y):
    """sign(co) co^2 of the two-pass correlation over the pairwise-complete rows, and its bound"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ok = ~np.isnan(x) & ~np.isnan(y)
    n = int(ok.sum())
    if n < 2:
        return LD(np.nan), 0.0
    with np.errstate(all="ignore"):
        a, b = x[ok].astype(LD), y[ok].astype(LD)
        da, db = a - np.sum(a) / LD(n), b - np.sum(b) / LD(n)
        co = np.sum(da * db) / np.sqrt(np.sum(da * da) * np.sum(db * db))
    if np.isnan(co):
        return LD(np.nan), 0.0
    d = 2.0 * (n + 6) * U
    return np.sign(co) * co * co, 2.0 * abs(float(co)) * d + d * d


def _spearman(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ok = ~np.isnan(x) & ~np.isnan(y)
    if ok.sum() < 2:
        return LD(np.nan), 0.0
    return _corr(average_ranks(x[ok]), average_ranks(y[ok]))


def _auc(y, p):
    y, p = np.asarray(y, dtype=np.float64), np.asarray(p, dtype=np.float64)
    sel = ~np.isnan(y)
    pos = y[sel] > 0
    n1, n0 = int(pos.sum()), int((~pos).sum())
    if n1 == 0 or n0 == 0 or np.isnan(p[sel]).any():
        return LD(np.nan), 0.0
    r1 = np.sum(average_ranks(p[sel])[pos].astype(LD))     # half-integers: exact
    num = np.float64(r1 - LD(n1) * LD(n1 + 1) / LD(2))     # exact in float64 as well
    return LD(num / np.float64(n1 * n0)), 0.0              # one correctly rounded float64 division


def _tjur(one, zero, p):
    p = np.asarray(p, dtype=np.float64)
    means, bound = [], 0.0
    for cls in (one, zero):
        v = p[cls].astype(LD)
        if v.size == 0:
            return LD(np.nan), 0.0
        with np.errstate(all="ignore"):
            mean = np.sum(v) / LD(v.size)
            bound += (v.size - 1) * U * float(np.sum(np.abs(v)) / LD(v.size)) + U * abs(float(mean))
        means.append(mean)
    with np.errstate(all="ignore"):
        val = means[0] - means[1]
    if not np.isfinite(val):
        return val, 0.0
    return val, bound + U * abs(float(val))


def reference(Y, m, pO, family):
    """The 10 x ns measures in the order of KEYS (np.longdouble, NaN outside each measure's family)
    and their 10 x ns float64 bounds (0: equality)."""
    Y, m = np.asarray(Y, dtype=np.float64), np.asarray(m, dtype=np.float64)
    ns = Y.shape[1]
    val = np.full((len(KEYS), ns), np.nan, dtype=LD)
    bnd = np.zeros((len(KEYS), ns))

    def put(key, j, vb):
        val[KEYS.index(key), j], bnd[KEYS.index(key), j] = vb

    for j in range(ns):
        y, p = Y[:, j], m[:, j]
        put("RMSE", j, _rmse(y, p))
        if family[j] == 1:
            put("R2", j, _corr(y, p))
        elif family[j] == 2:
            put("AUC", j, _auc(y, p))
            put("TjurR2", j, _tjur(y == 1, y == 0, p))
        elif family[j] == 3:
            o = np.asarray(pO, dtype=np.float64)[:, j]
            put("SR2", j, _spearman(y, p))
            put("O.AUC", j, _auc(y, o))
            put("O.TjurR2", j, _tjur(y > 0, ~np.isnan(y) & ~(y > 0), o))
            put("O.RMSE", j, _rmse(np.where(np.isnan(y), np.nan, (y > 0).astype(np.float64)), o))
            yc = np.where(y == 0, np.nan, y)
            with np.errstate(all="ignore"):
                mc = p / o
            put("C.SR2", j, _spearman(yc, mc))
            put("C.RMSE", j, _rmse(yc, mc))
        else:
            raise ValueError(f"family {family[j]} of species {j} is outside 1..3")
    return val, bnd


def as_dict(out, family):
    """A 10 x ns result as evaluateModelFit's dict: the keys of the families that occur."""
    family = np.asarray(family)
    keys = ("RMSE",) + tuple(k for f in (1, 2, 3) if (family == f).any() for k in FAMILY_KEYS[f])
    return {k: np.asarray(out[KEYS.index(k)], dtype=np.float64) for k in keys}


def assert_within(got, val, bnd, what=""):
    """got (dict of ns-vectors, or 10 x ns) against the restatement: the same NaN and inf pattern,
    equality where the bound is 0, |got - val| <= bound elsewhere.  Returns the worst error / bound
    per bound family (rmse, tjur, corr) over the finite cells."""
    worst = dict(rmse=0.0, tjur=0.0, corr=0.0)
    for k, key in enumerate(KEYS):
        if isinstance(got, dict) and key not in got:
            assert np.all(np.isnan(val[k])), (what, key)
            continue
        g = np.asarray(got[key] if isinstance(got, dict) else got[k], dtype=np.float64)
        ref = val[k]
        assert np.array_equal(np.isnan(g), np.isnan(ref)), (what, key, g, ref.astype(np.float64))
        inf = np.isinf(ref)
        assert np.array_equal(g[inf], ref[inf].astype(np.float64)) and not np.isinf(g[~inf]).any(), (what, key, g)
        fin = np.isfinite(ref)
        err = np.abs(g[fin].astype(LD) - ref[fin]).astype(np.float64)
        if BOUND_FAMILY[key] == "auc":
            assert np.array_equal(g[fin], ref[fin].astype(np.float64)), (what, key, g, ref.astype(np.float64))
            continue
        assert np.all(err <= bnd[k][fin]), (what, key, err, bnd[k][fin])
        if err.size:
            with np.errstate(all="ignore"):
                ratio = np.where(bnd[k][fin] > 0, err / bnd[k][fin], 0.0)
            worst[BOUND_FAMILY[key]] = max(worst[BOUND_FAMILY[key]], float(ratio.max()))
    return worst


def assert_close_to_host(got, host, tol=1e-10, what=""):
    """Two evaluateModelFit dicts: the same keys, NaN and inf pattern, AUC and O.AUC bit-equal,
    every other finite value within tol."""
    assert set(got) == set(host), (what, sorted(got), sorted(host))
    for key in host:
        g, h = np.asarray(got[key]), np.asarray(host[key])
        assert np.array_equal(np.isnan(g), np.isnan(h)), (what, key, g, h)
        inf = np.isinf(h)
        assert np.array_equal(g[inf], h[inf]) and not np.isinf(g[~inf]).any(), (what, key, g, h)
        fin = np.isfinite(h)
        if BOUND_FAMILY[key] == "auc":
            assert np.array_equal(g[fin], h[fin]), (what, key, g, h)
        else:
            assert np.all(np.abs(g[fin] - h[fin]) <= tol), (what, key, g, h)


class Stub:
    """What evaluateModelFit reads of a model: Y, distr[:, 0], ny, ns."""

    def __init__(self, Y, family):
        self.Y = np.asarray(Y, dtype=np.float64)
        self.ny, self.ns = self.Y.shape
        self.distr = np.column_stack([np.asarray(family, dtype=np.int64), np.ones(self.ns, dtype=np.int64)])


def as_summary(m, pO):
    """The summary dict evaluateModelFit(summary=) reads: mean for the other columns, median and
    occ for the Poisson ones (m serves as both)."""
    return dict(mean=m, median=m, occ=pO)


MIXED_FAMILY = np.array([1, 1, 1, 2, 2, 2, 3, 3, 3], dtype=np.int32)


def mixed_case(ny, family=MIXED_FAMILY, seed=0, na_frac=0.05):
    """Y, m, pO (ny x ns) with heavy ties: probit m a mean over 4 draws (values in {0, 1/4, .., 1}),
    pO in {1/4, .., 1}, Poisson Y with many zeros and repeated counts, the Poisson m a median of 3
    counts; a few NA in Y.  The first (up to) four rows of every column are fixed so that both
    classes and two distinct values on each side of every correlation exist once ny >= 4."""
    family = np.asarray(family)
    ns = len(family)
    rng = np.random.default_rng([seed, ny, ns])
    Y, m, pO = np.zeros((ny, ns)), np.zeros((ny, ns)), np.full((ny, ns), np.nan)
    for j, f in enumerate(family):
        if f == 1:
            Y[:, j] = 3.0 + 2.0 * rng.standard_normal(ny)
            m[:, j] = 3.0 + 0.7 * (Y[:, j] - 3.0) + rng.standard_normal(ny)
        elif f == 2:
            p = rng.random(ny)
            Y[:, j] = (rng.random(ny) < p).astype(float)
            m[:, j] = (rng.random((ny, 4)) < (0.25 + 0.5 * p)[:, None]).mean(axis=1)
        else:
            lam = np.exp(rng.normal(-0.3, 1.0, ny))
            Y[:, j] = rng.poisson(lam)
            m[:, j] = np.median(rng.poisson(lam[:, None], (ny, 3)), axis=1)
            pO[:, j] = (1 + rng.binomial(3, 1.0 - np.exp(-lam))) / 4.0
    na = rng.random((ny, ns)) < na_frac
    na[:4] = False
    Y[na] = np.nan
    k = min(ny, 4)
    for j, f in enumerate(family):
        if f == 2:
            Y[:k, j], m[:k, j] = [1.0, 0.0, 1.0, 0.0][:k], [0.75, 0.25, 0.5, 0.5][:k]
        elif f == 3:
            Y[:k, j], m[:k, j], pO[:k, j] = [0.0, 2.0, 5.0, 1.0][:k], [0.0, 2.0, 4.0, 1.0][:k], [0.25, 1.0, 0.75, 0.5][:k]
    return Y, m, pO


EDGE_NY = 65


def edge_case():
    """Y, m, pO, family at ny = 65: NA in Y, NaN in m (cells no CV fold filled), both; a single-class
    probit column, a constant m, -0.0 beside +0.0 in m, a real +inf in m, a probit Y holding a 2;
    pO = 0 where m > 0 (m / pO = +inf) and where m = 0 (NaN); a Poisson column of zeros only."""
    ny = EDGE_NY
    rng = np.random.default_rng(65)
    cols = []

    def probit():
        p = rng.random(ny)
        y = (rng.random(ny) < p).astype(float)
        y[:2] = [1.0, 0.0]
        return y, (rng.random((ny, 4)) < (0.25 + 0.5 * p)[:, None]).mean(axis=1)

    def normal():
        y = 1.0 + rng.standard_normal(ny)
        return y, 1.0 + 0.5 * (y - 1.0) + 0.5 * rng.standard_normal(ny)

    def poisson():
        lam = np.exp(rng.normal(0.0, 1.0, ny))
        y = rng.poisson(lam).astype(float)
        y[:4] = [0.0, 2.0, 5.0, 1.0]
        mm = np.median(rng.poisson(lam[:, None], (ny, 3)), axis=1)
        o = (1 + rng.binomial(3, 1.0 - np.exp(-lam))) / 4.0
        mm[:4], o[:4] = [0.0, 2.0, 4.0, 1.0], [0.25, 1.0, 0.75, 0.5]
        return y, mm, o

    nan_o = np.full(ny, np.nan)
    # probit
    y, p = probit(); y[[5, 17, 40]] = np.nan; cols.append((2, y, p, nan_o))                   # NA in Y
    y, p = probit(); p[[6, 18]] = np.nan; cols.append((2, y, p, nan_o))                       # NaN in m
    y, p = probit(); y[[5, 17]] = np.nan; p[[17, 30]] = np.nan; cols.append((2, y, p, nan_o))  # both, one row shared
    y, p = probit(); y[[5, 17]] = np.nan; p[[5, 17]] = np.nan; cols.append((2, y, p, nan_o))   # NaN in m only where Y is NA
    y, p = probit(); y[:] = 1.0; cols.append((2, y, p, nan_o))                                # single class
    y, p = probit(); p[:] = 0.5; cols.append((2, y, p, nan_o))                                # constant m
    y, p = probit(); p[p < 0.5] = 0.0; p[::3][p[::3] == 0.0] = -0.0; cols.append((2, y, p, nan_o))  # -0.0 beside +0.0
    y, p = probit(); p[9] = np.inf; cols.append((2, y, p, nan_o))                             # +inf in m
    y, p = probit(); y[[7, 8]] = 2.0; cols.append((2, y, p, nan_o))                           # a Y outside {0, 1}
    # normal
    y, p = normal(); y[[3, 4]] = np.nan; p[[4, 50]] = np.nan; cols.append((1, y, p, nan_o))
    y, p = normal(); p[:] = 0.25; cols.append((1, y, p, nan_o))
    y, p = normal(); p[11] = np.inf; cols.append((1, y, p, nan_o))
    y, p = normal(); p[p < 1.0] = 0.0; p[::2][p[::2] == 0.0] = -0.0; cols.append((1, y, p, nan_o))
    # Poisson
    y, p, o = poisson(); o[[10, 11, 12, 13]] = 0.0; p[[10, 11]] = [3.0, 1.0]; p[[12, 13]] = 0.0
    y[[10, 12]] = [2.0, 4.0]; cols.append((3, y, p, o))                                       # m / pO = +inf and NaN
    y, p, o = poisson(); y[[20, 21]] = np.nan; p[[21, 22]] = np.nan; o[[22, 23]] = np.nan; cols.append((3, y, p, o))
    y, p, o = poisson(); p[p < 1.0] = 0.0; p[::2][p[::2] == 0.0] = -0.0; cols.append((3, y, p, o))
    y, p, o = poisson(); y[:] = 0.0; cols.append((3, y, p, o))                                # zeros only
    y, p, o = poisson(); p[14] = np.inf; cols.append((3, y, p, o))                            # +inf in m
    y, p, o = poisson(); o[:] = 0.5; cols.append((3, y, p, o))                                # constant pO
    family = np.array([c[0] for c in cols], dtype=np.int32)
    return (np.column_stack([c[1] for c in cols]), np.column_stack([c[2] for c in cols]),
            np.column_stack([c[3] for c in cols]), family)
