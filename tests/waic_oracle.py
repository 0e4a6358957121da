"""References for computeWAIC (tests only).

* ``literal`` -- R/computeWAIC.R:124-129 as written: Bl = -log(colMeans(exp(val))), V = the
  ddof = 1 column variance, WAIC = mean(Bl + V).
* ``shifted`` -- the same quantities with the max-shifted log-mean-exp the device uses
  (waic.hip): Bl = -(m + log mean exp(val - m)), m = max over samples.
* ``mp_*`` -- 50-digit mpmath evaluations of the cell terms of hmsc_amd/post.py::computeWAIC at
  the given doubles.
* ``duck_model`` / ``random_post`` -- a posterior written down directly on the attributes
  computeWAIC reads, for shapes no fitted fixture has.
"""
from types import SimpleNamespace

import mpmath as mp
import numpy as np

mp.mp.dps = 50


def literal(val):
    val = np.asarray(val, dtype=np.float64)
    with np.errstate(divide="ignore"):
        Bl = -np.log(np.mean(np.exp(val), axis=0))
    V = val.var(axis=0, ddof=1)
    return Bl, V, float(np.mean(Bl + V))


def shifted(val):
    val = np.asarray(val, dtype=np.float64)
    m = val.max(axis=0)
    Bl = -(m + np.log(np.mean(np.exp(val - m), axis=0)))
    mean = val.mean(axis=0)
    V = ((val - mean) ** 2).sum(axis=0) / (val.shape[0] - 1)
    return Bl, V, float(np.mean(Bl + V))


def mp_site(val):
    """(Bl, V) of one site's column of val, in mpmath."""
    v = [mp.mpf(float(x)) for x in val]
    n = len(v)
    Bl = -mp.log(mp.fsum(mp.exp(x) for x in v) / n)
    mean = mp.fsum(v) / n
    V = mp.fsum((x - mean) ** 2 for x in v) / (n - 1)
    return Bl, V


def mp_log_pnorm(x):
    """log Phi(x) at the double x (an mpf; -inf where x = -inf)."""
    x = mp.mpf(float(x))
    if x > 0:
        return mp.log1p(-mp.exp(mp_log_pnorm(-x)))
    if x < -100:   # the asymptotic series of erfc: its terms fall below 1e-60 within 40 of them here
        s, t = mp.mpf(1), mp.mpf(1)
        for k in range(1, 41):
            t *= -(2 * k - 1) / (x * x)
            s += t
        return -x * x / 2 - mp.log(-x * mp.sqrt(2 * mp.pi)) + mp.log(s)
    return mp.log(mp.ncdf(x))


def mp_normal_terms(y, E, sigma):
    """The three terms dnorm(y, E, sigma^(-1/2), log = TRUE) is summed from."""
    y, E, sigma = mp.mpf(float(y)), mp.mpf(float(E)), mp.mpf(float(sigma))
    return -(y - E) ** 2 * sigma / 2, mp.log(sigma) / 2, -mp.log(2 * mp.pi) / 2


def mp_poisson_cell(y, E, sigma, gx, gw):
    """log(pi^(-1/2) sum_g w_g dpois(y, exp(E + sqrt(2) x_g sigma^(-1/2)))) and the scale
    max(1, y |eta|_max, e^eta_max, lgamma(y + 1)) its error is measured against."""
    y, E, sd = mp.mpf(float(y)), mp.mpf(float(E)), 1 / mp.sqrt(mp.mpf(float(sigma)))
    etas = [E + mp.sqrt(2) * mp.mpf(float(x)) * sd for x in gx]
    lg = mp.loggamma(y + 1)
    tot = mp.fsum(mp.mpf(float(w)) * mp.exp(y * eta - mp.exp(eta) - lg) for eta, w in zip(etas, gw))
    scale = max(mp.mpf(1), max(y * abs(eta) for eta in etas), max(mp.exp(eta) for eta in etas), lg)
    return mp.log(tot / mp.sqrt(mp.pi)), scale


def duck_model(Y, X, family, Pi=None, nps=(), xs=None):
    """The attributes computeWAIC and its argument builder read, without a model object: family
    codes 1 / 2 / 3 per species, Pi 1-based (ny, nr), xs[r] the unit covariates of a
    covariate-dependent level (unit order) or None."""
    import pandas as pd
    Y = np.asarray(Y, dtype=np.float64)
    ny, ns = Y.shape
    nr = 0 if Pi is None else Pi.shape[1]
    distr = np.zeros((ns, 4), dtype=np.int64)
    distr[:, 0] = family
    xs = list(xs) if xs is not None else [None] * nr
    rL = [SimpleNamespace(xDim=0 if xs[r] is None else xs[r].shape[1], x=xs[r], sDim=0) for r in range(nr)]
    names = [f"lev{r}" for r in range(nr)]
    # unit k of level r is named so that levels(dfPi[, r]) keeps the numeric order
    dfPi = pd.DataFrame({names[r]: [f"u{int(k):06d}" for k in Pi[:, r]] for r in range(nr)}) if nr else None
    return SimpleNamespace(Y=Y, X=np.asarray(X, dtype=np.float64), Pi=Pi, distr=distr, ny=ny, ns=ns,
                           nc=X.shape[1], nr=nr, np=np.asarray(nps, dtype=np.int64), rL=rL, rLNames=names,
                           dfPi=dfPi, ncRRR=0, postList=None)


def random_post(hM, S, nfs, seed, beta_scale=0.3, nf_jitter=False):
    """S samples written down directly: Beta ~ beta_scale N(0, 1), Eta ~ N(0, 1), Lambda ~
    N(0, 1) / (2 sqrt nf), sigma ~ U(0.5, 2).  nf_jitter: odd samples of level 0 drop a factor."""
    rng = np.random.default_rng(seed)
    post = []
    for s in range(S):
        etas, lams = [], []
        for r in range(hM.nr):
            nf = nfs[r] - (1 if nf_jitter and r == 0 and s % 2 and nfs[r] > 1 else 0)
            xd = hM.rL[r].xDim
            etas.append(rng.standard_normal((int(hM.np[r]), nf)))
            lams.append(rng.standard_normal((nf, hM.ns) + ((xd,) if xd else ())) / (2 * np.sqrt(nf)))
        post.append(dict(Beta=beta_scale * rng.standard_normal((hM.nc, hM.ns)), sigma=rng.uniform(0.5, 2.0, hM.ns),
                         Eta=etas, Lambda=lams))
    return post
