"""Reference of predict's kernel (hmsc_amd/csrc/predict.hip), cell by cell, and the inputs the
predict tests feed it (tests/test_host_predict_reference.py, tests/test_gpu_predict_cells.py).
Test infrastructure only.

call_predict fills hmsc_predict_args from plain arrays, as hmsc_amd/predict.py does from a
posterior, so a case is one small launch with no Hmsc object and no chain.  reference is the same
operation in extended precision: the linear predictor

    L_ref = X Beta_s + sum_r Eta_r,s[Pi_r,] Lambda_r,s

in np.longdouble (64-bit mantissa) or, where longdouble is no wider than double, mpmath's fdot,
together with A = sum_k |a_k| |b_k| per cell, the scale of the dot product's forward error:
a K-term fma chain in double is within gamma_K A, gamma_K = K u / (1 - K u), u = 2^-53, of the
exact sum.  pnorm and exp come from mpmath at draw_reference.DPS digits, the normal deviates are
the oracle's AS241 of the cell's first uniform (pinned by tests/test_oracle_rng.py) and the
Poisson counts are the oracle's _rpois_ptrs on the reference's own exp(z).
"""
import ctypes as C
import functools

import mpmath as mp
import numpy as np

import draw_reference as D
from helpers import H, O  # noqa: F401  (puts the repository root on sys.path)
from hmsc_amd import _lib as L
from oracle.rng import Rng

U = 2.0 ** -53
S_PREDICT = 30
PT_I, PT_J = 64, 32          # predict.hip: a workgroup's site x species tile
LONGDOUBLE_OK = np.finfo(np.longdouble).eps <= 2.0 ** -63

# the fixed-rate Poisson columns (lambda = 10 itself stays out: exp(log 10) may round to either
# side of the lam < 10 switch, and the device's exp and the host's may then disagree about the
# whole column)
POIS_LAMBDAS = (0.05, 1.0, 9.999, 10.001, 30.0, 1e3, 1e6, 1e9, 1e12)
POIS_NY, POIS_SEED = 20000, 977


# ---------------------------------------------------------------------------------------------
# the C ABI, from arrays
# ---------------------------------------------------------------------------------------------
def call_raw(ny, ns, nc, nr, nsamples, expected, seed, X, Beta, sigma, family, yscale, Pi, nps, nfs, Eta, Lambda,
             out, device=0):
    """hmsc_predict on flat arrays already in the ABI's layout; returns the return code (the
    message is hmsc_last_error).  The sizes are passed as given, so a refusal can be provoked with
    sizes the arrays do not have."""
    keep = [L.f64(X), L.f64(Beta), L.f64(sigma), L.i32(family), L.f64(yscale),
            L.i32(Pi if Pi is not None else [0]), L.i32(nps if len(nps) else [0]), L.i32(nfs if len(nfs) else [0])]
    a = L.hmsc_predict_args()
    a.ny, a.ns, a.nc, a.nr, a.nsamples = int(ny), int(ns), int(nc), int(nr), int(nsamples)
    a.expected, a.seed, a.device = int(expected), int(seed), int(device)
    a.X, a.Beta, a.sigma = L.fptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2])
    a.family, a.YScalePar = L.iptr(keep[3]), L.fptr(keep[4])
    a.Pi, a.np, a.nf = L.iptr(keep[5]), L.iptr(keep[6]), L.iptr(keep[7])
    for r in range(min(int(nr), L.MAX_LEVELS)):
        e, lm = L.f64(Eta[r]), L.f64(Lambda[r])
        keep += [e, lm]
        a.Eta[r], a.Lambda[r] = L.fptr(e), L.fptr(lm)
    return L.lib().hmsc_predict(C.byref(a), L.fptr(out))


def last_error():
    return L.lib().hmsc_last_error().decode()


def live_resources():
    out = (C.c_int64 * 4)()
    L.check(L.lib().hmsc_debug_live_resources(out))
    return list(out)


def call_predict(X, Beta, sigma, family, YScalePar, Pi, nps, nfs, Eta, Lambda, expected, seed, device=0):
    """X ny x nc; Beta S x nc x ns; sigma S x ns; family ns; YScalePar 2 x ns; Pi ny x nr, 1-based;
    nps, nfs the levels' unit and factor counts; Eta[r] S x np_r x nf_r; Lambda[r] S x nf_r x ns.
    Returns (out S x ny x ns, return code)."""
    X = np.asarray(X, dtype=np.float64)
    Beta = np.asarray(Beta, dtype=np.float64)
    S, nc, ns = Beta.shape
    ny, nr = X.shape[0], len(nfs)
    cm = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).transpose(0, 2, 1)).ravel()  # noqa: E731
    out = np.full(S * ny * ns, np.nan)
    rc = call_raw(ny, ns, nc, nr, S, expected, seed, X.ravel(order="F"), cm(Beta), np.asarray(sigma).ravel(),
                  family, np.asarray(YScalePar, dtype=np.float64).ravel(order="F"),
                  None if nr == 0 else np.asarray(Pi).reshape(ny, nr).ravel(order="F"), list(nps), list(nfs),
                  [cm(e) for e in Eta], [cm(lm) for lm in Lambda], out, device)
    return out.reshape(S, ns, ny).transpose(0, 2, 1), rc


def predict_inputs(inp, expected, seed):
    """call_predict on a dict of build_inputs."""
    return call_predict(inp["X"], inp["Beta"], inp["sigma"], inp["family"], inp["YScalePar"], inp["Pi"], inp["np"],
                        inp["nf"], inp["Eta"], inp["Lambda"], expected, seed)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def random_pi(rng, ny, npr):
    """ny units of 1..npr drawn at random: not monotone, with repeats, units 1 and npr present."""
    for _ in range(100):
        pi = rng.integers(1, npr + 1, ny)
        if ny >= 2:
            a, b = rng.choice(ny, 2, replace=False)
            pi[a], pi[b] = 1, npr
        d = np.diff(pi)
        if ny < 4 or (np.any(d > 0) and np.any(d < 0) and len(np.unique(pi)) < ny):
            return pi.astype(np.int32)
    raise RuntimeError("random_pi: no admissible draw")


def build_inputs(ny, ns, nc, nfs=(), S=3, seed=0, np_mode="lt", family=1, sigma=1.0, yscale=None):
    """iid N(0, 1) values, distinct in every (sample, k, species) and (sample, unit, factor), so an
    index or stride mix-up moves a cell by O(1).  np_mode "lt": np_r = ceil(ny / 3) + r units (< ny
    from ny = 4 on); "eq": np_r = ny; or one of the two per level.  family: a scalar or one value
    per species; sigma: anything that broadcasts to S x ns; yscale 2 x ns (None: no
    back-transform)."""
    nfs = [int(f) for f in nfs]
    modes = [np_mode] * len(nfs) if isinstance(np_mode, str) else list(np_mode)
    rng = np.random.default_rng([seed, ny, ns, nc, len(nfs)] + [1 if m == "eq" else 0 for m in modes])
    nps = [ny if m == "eq" else min(ny, (ny + 2) // 3 + r) for r, m in enumerate(modes)]
    inp = dict(X=rng.standard_normal((ny, nc)), Beta=rng.standard_normal((S, nc, ns)),
               sigma=np.broadcast_to(np.asarray(sigma, dtype=np.float64), (S, ns)).copy(),
               family=np.broadcast_to(np.asarray(family, dtype=np.int32), (ns,)).copy(),
               YScalePar=np.vstack([np.zeros(ns), np.ones(ns)]) if yscale is None else np.asarray(yscale, float),
               Pi=np.column_stack([random_pi(rng, ny, n) for n in nps]) if nfs else np.zeros((ny, 0), np.int32),
               np=nps, nf=nfs,
               Eta=[rng.standard_normal((S, n, f)) for n, f in zip(nps, nfs)],
               Lambda=[rng.standard_normal((S, f, ns)) for f in nfs])
    inp["K"] = nc + sum(nfs)
    return inp


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
def _design(inp, s):
    """[X | Eta_1,s[Pi_1,] | ...] (ny x K) and [Beta_s; Lambda_1,s; ...] (K x ns) of sample s."""
    a = [np.asarray(inp["X"], dtype=np.float64)]
    b = [np.asarray(inp["Beta"][s], dtype=np.float64)]
    for r in range(len(inp["nf"])):
        a.append(np.asarray(inp["Eta"][r][s])[np.asarray(inp["Pi"])[:, r] - 1])
        b.append(np.asarray(inp["Lambda"][r][s]))
    return np.hstack(a), np.vstack(b)


def linear_predictor(inp):
    """(L_ref S x ny x ns in longdouble, A S x ny x ns in double)."""
    S = len(inp["Beta"])
    Ls, As = [], []
    for s in range(S):
        a, b = _design(inp, s)
        As.append(np.abs(a) @ np.abs(b))
        if LONGDOUBLE_OK:
            Ls.append(a.astype(np.longdouble) @ b.astype(np.longdouble))
        else:   # (exact to DPS digits, rounded to the widest float there is)
            with mp.workdps(D.DPS):
                Ls.append(np.array([[np.longdouble(mp.fdot(map(float, a[i]), map(float, b[:, j])))
                                     for j in range(b.shape[1])] for i in range(a.shape[0])]))
    return np.stack(Ls), np.stack(As)


def l_bound(inp, A):
    """1.01 gamma_K A: the forward error of the kernel's K-term fma chain (1 % over K u A for the
    1 / (1 - K u) of gamma_K, the rounding of A itself and the reference's own 2^-64)."""
    return 1.01 * inp["K"] * U * A


def to_mpf(x):
    """A longdouble (or double), exactly."""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi))) if np.isfinite(hi) else mp.mpf(hi)


def mp_pnorm(x):
    return mp.erfc(-to_mpf(x) / mp.sqrt(2)) / 2


def mp_exp(x):
    return mp.exp(to_mpf(x))


def mp_map(f, x):
    """f over an array, as an object array of mpf."""
    x = np.asarray(x)
    out = np.empty(x.shape, dtype=object)
    with mp.workdps(D.DPS):
        for k, v in enumerate(x.ravel()):
            out.reshape(-1)[k] = f(v)
    return out


def mp_to_double(ref):
    """Object array of mpf -> double (inf beyond the range, as a correctly rounded exp gives)."""
    return np.array([float(r) for r in np.asarray(ref, dtype=object).ravel()]).reshape(np.shape(ref))


def mp_to_wide(ref):
    """Object array of mpf -> the widest float there is, over its whole exponent range (values
    below the doubles' subnormals keep their size in a longdouble)."""
    out = np.empty(np.shape(ref), dtype=np.longdouble)
    with mp.workdps(D.DPS):
        for k, r in enumerate(np.asarray(ref, dtype=object).ravel()):
            m, e = mp.frexp(r)
            hi = float(m)
            out.reshape(-1)[k] = np.ldexp(np.longdouble(hi) + np.longdouble(float(m - mp.mpf(hi))), int(e))
    return out


def abs_err(y, ref):
    """|y - ref| per cell as longdouble (errors below the doubles' subnormals keep their size), ref
    an object array of mpf or its mp_to_wide, broadcast against y: taken in longdouble where that
    has a 64-bit mantissa (the difference of neighbours is then exact to 2^-11 of a double's
    spacing), in mpmath otherwise; inf where y is not finite."""
    y = np.asarray(y, dtype=np.float64)
    ref = np.asarray(ref)
    if LONGDOUBLE_OK or ref.dtype != object:
        wide = mp_to_wide(ref) if ref.dtype == object else ref
        with np.errstate(invalid="ignore"):
            e = np.abs(y.astype(np.longdouble) - np.broadcast_to(wide, y.shape))
    else:
        e = np.empty(y.shape, dtype=np.longdouble)
        with mp.workdps(D.DPS):
            for k, (v, r) in enumerate(zip(y.ravel(), np.broadcast_to(ref, y.shape).ravel())):
                e.reshape(-1)[k] = float(abs(mp.mpf(float(v)) - r)) if np.isfinite(v) else np.inf
    return np.where(np.isfinite(y), e, np.inf)


def cells(ny, ns):
    return (np.arange(ny)[:, None] + ny * np.arange(ns)[None, :]).astype(np.uint64)


def normal_deviates(seed, ny, ns, S):
    """The N(0, 1) of every cell: AS241 of the first uniform of (cell, 0, S_PREDICT, s)."""
    rng = Rng(seed)
    return np.stack([rng.normal(cells(ny, ns), 0, S_PREDICT, s) for s in range(S)])


def reference(inp, expected, seed, poisson=True):
    """dict(L, A: linear_predictor; q: the normal deviates and z = L + sqrt(sigma) q in longdouble
    (draws only); out: what predict returns, S x ny x ns, rounded to double; mp: the mpf values of
    the pnorm / exp cells (expected only; None elsewhere)).  poisson=False leaves the Poisson draws
    NaN (a count per cell costs a Python call)."""
    Lr, A = linear_predictor(inp)
    S, ny, ns = Lr.shape
    fam = np.asarray(inp["family"])
    sg = np.asarray(inp["sigma"], dtype=np.float64)
    res = dict(L=Lr, A=A, q=None, z=None, mp=None)
    out = np.empty((S, ny, ns), dtype=np.longdouble)
    if expected:
        ref = np.full((S, ny, ns), None, dtype=object)
        for j in range(ns):
            if fam[j] == 2:
                ref[:, :, j] = mp_map(mp_pnorm, Lr[:, :, j])
            elif fam[j] == 3:
                ref[:, :, j] = mp_map(mp_exp, Lr[:, :, j] + (sg[:, j].astype(np.longdouble) / 2)[:, None])
        res["mp"] = ref
        out[:] = Lr
        sel = fam != 1
        out[:, :, sel] = mp_to_double(ref[:, :, sel])
    else:
        q = normal_deviates(seed, ny, ns, S)
        z = Lr + np.sqrt(sg.astype(np.longdouble))[:, None, :] * q
        res["q"], res["z"] = q, z
        out[:] = z
        out[:, :, fam == 2] = (z[:, :, fam == 2] > 0)
        rng, cl = Rng(seed), cells(ny, ns)
        for j in np.nonzero(fam == 3)[0]:
            if not poisson:
                out[:, :, j] = np.nan
                continue
            lam = mp_to_double(mp_map(mp_exp, z[:, :, j]))
            for s in range(S):
                out[s, :, j] = [O._rpois_ptrs(float(lam[s, i]), rng, int(cl[i, j]), s) for i in range(ny)]
    m, sd = np.asarray(inp["YScalePar"], dtype=np.float64)
    tr = (m != 0) | (sd != 1)
    out[:, :, tr] = out[:, :, tr] * sd[tr].astype(np.longdouble) + m[tr].astype(np.longdouble)
    res["out"] = out.astype(np.float64)
    return res


def tile_of(i, j):
    """Where cell (i, j) sits: (site tile, row in it, species tile, column in it)."""
    return f"tile ({i // PT_I}, {j // PT_J}) at ({i % PT_I}, {j % PT_J})"


# ---------------------------------------------------------------------------------------------
# Poisson columns at fixed rates
# ---------------------------------------------------------------------------------------------
def poisson_rates():
    """The rates the samplers see: exp(log lambda) in double, as predict forms exp(Z)."""
    return np.exp(np.log(np.array(POIS_LAMBDAS)))


@functools.lru_cache(maxsize=None)
def oracle_poisson_counts():
    """POIS_NY x len(POIS_LAMBDAS) counts of oracle._rpois_ptrs under Rng(POIS_SEED): cell
    i + POIS_NY j, sample 0 -- the cells predict gives a POIS_NY x 9 prediction.  Computed once per
    process (about 10 s) and shared; read-only."""
    rng = Rng(POIS_SEED)
    lam = poisson_rates()
    out = np.empty((POIS_NY, len(lam)))
    for j, lj in enumerate(lam):
        out[:, j] = [O._rpois_ptrs(float(lj), rng, i + POIS_NY * j, 0) for i in range(POIS_NY)]
    out.setflags(write=False)
    return out


def _pool(edges_hi, prob, n):
    """Pool neighbouring bins (given by their inclusive upper edges and probabilities) from the
    left until every expected count n p is >= 5; a short remainder joins the last bin."""
    hi, pr, acc = [], [], 0.0
    for e, p in zip(edges_hi, prob):
        acc += p
        if n * acc >= 5.0:
            hi.append(e)
            pr.append(acc)
            acc = 0.0
    if acc > 0.0 or hi[-1] != edges_hi[-1]:
        pr[-1] += acc
        hi[-1] = edges_hi[-1]
    return np.array(hi), np.array(pr)


def poisson_gof_pvalue(counts, lam):
    """Chi-square goodness of fit of `counts` to Poisson(lam) (scipy.stats.poisson): integer bins
    for lam < 100, 42 bins at normal-quantile edges lam + sqrt(lam) Phi^-1(i / 42) above, pooled
    until every expected count is >= 5.  Returns (p, statistic, number of bins)."""
    from scipy import stats
    from scipy.special import ndtri
    counts = np.asarray(counts, dtype=np.float64)
    n = counts.size
    if lam < 100:
        top = int(stats.poisson.ppf(1.0 - 1e-12, lam)) + 1
        hi = np.arange(top + 1, dtype=np.float64)
    else:
        hi = np.unique(np.floor(lam + np.sqrt(lam) * ndtri(np.arange(1, 42) / 42.0)))
    cdf = np.concatenate([stats.poisson.cdf(hi, lam), [1.0]])
    hi = np.concatenate([hi, [np.inf]])              # the last bin is open above
    prob = np.diff(np.concatenate([[0.0], cdf]))
    hi, prob = _pool(hi, prob, n)
    obs = np.bincount(np.searchsorted(hi, counts, side="left"), minlength=len(hi)).astype(np.float64)
    stat = float(np.sum((obs - n * prob) ** 2 / (n * prob)))
    return float(stats.chi2.sf(stat, len(hi) - 1)), stat, len(hi)
