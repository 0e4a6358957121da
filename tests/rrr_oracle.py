"""Numpy restatement of the reference's reduced-rank regression blocks, for the tests.

The reference carries no test or fixture for XRRR models, so the restatement of
R/computeInitialParameters.R:20-27, R/updatewRRR.R, R/updatewRRRPriors.R and the sweep order of
R/sampleMcmc.R:219-306 lives here, next to the tests that use it, and calls the existing oracle
(oracle/hmsc_oracle.py) for every other block.  Randomness follows the oracle's Philox contract
(oracle/rng.py) on the streams hmsc_amd/csrc/rng.h reserves for these blocks: element
e = k + ncRRR c of vec(wRRR) draws normal(e, 0, S_WRRR, it); PsiRRR uses the same e, DeltaRRR the
component h.

One deliberate difference from Hmsc 3.0-4: R/updatewRRR.R:43 subtracts LRan from Z only when
nr > 1, so with a single random level the reference samples wRRR from the wrong conditional;
here (and on the device) LRan is subtracted for every nr >= 1.  tests/test_host_rrr.py checks
the moments against brute-force Gaussian conditioning at nr = 0, 1, 2.
"""
import numpy as np

from helpers import O, oracle_model

S_WRRR = 14
S_PSI_RRR = 28
S_DELTA_RRR = 29
S_INIT_DELTA_RRR = 54
S_INIT_PSI_RRR = 55
S_INIT_WRRR = 56


def rrr_model(hM):
    """oracle_model(hM) plus the RRR fields; m["X"] is the design matrix the other blocks read,
    [XScaled, XRRRScaled wRRR^T], refreshed by set_design whenever wRRR changes."""
    m = oracle_model(hM)
    m["XA"] = np.asarray(hM.XScaled, dtype=np.float64)
    m["XRRR"] = np.asarray(hM.XRRRScaled, dtype=np.float64)
    m["ncRRR"] = int(hM.ncRRR)
    for f in ("nuRRR", "a1RRR", "b1RRR", "a2RRR", "b2RRR"):
        m[f] = float(hM[f])
    m["X"] = np.hstack([m["XA"], np.zeros((hM.ny, hM.ncRRR))])
    return m


def set_design(m, wRRR):
    """X = cbind(X1A, XRRR %*% t(wRRR))   (R/sampleMcmc.R:196-205, R/updatewRRR.R:62-73)."""
    m["X"] = np.hstack([m["XA"], m["XRRR"] @ np.asarray(wRRR).T])
    return m["X"]


def init_rrr(m, rng):
    """R/computeInitialParameters.R:20-27."""
    nk, nco = m["ncRRR"], m["XRRR"].shape[1]
    delta = np.empty(nk)
    delta[0] = rng.gamma(0, S_INIT_DELTA_RRR, 0, m["a1RRR"], m["b1RRR"])                       # :21
    if nk > 1:
        delta[1:] = rng.gamma(np.arange(1, nk), S_INIT_DELTA_RRR, 0, m["a2RRR"], m["b2RRR"])
    kk, cc = np.meshgrid(np.arange(nk), np.arange(nco), indexing="ij")
    e = kk + nk * cc
    psi = rng.gamma(e, S_INIT_PSI_RRR, 0, m["nuRRR"] / 2, m["nuRRR"] / 2)                      # :22
    tau = np.cumprod(delta)                                                                    # :23
    mult = np.sqrt(psi * tau[:, None]) ** -1                                                   # :24-25
    w = rng.normal(e, 0, S_INIT_WRRR, 0) * mult                                                # :26
    return dict(wRRR=w, PsiRRR=psi, DeltaRRR=delta)


def compute_initial_parameters(m, rng, nf=None):
    """computeInitialParameters with ncRRR > 0: the RRR draws first, then everything else on
    XScaled = cbind(XScaled, XB) (:27-50)."""
    rrr = init_rrr(m, rng)
    set_design(m, rrr["wRRR"])
    st = O.compute_initial_parameters(m, rng, nf=nf)
    st.update(rrr)
    return st


def wrrr_moments(st, m):
    """(iU, RiU, mu) of the wRRR conditional, R/updatewRRR.R:20-58 (LRan subtracted for nr >= 1)."""
    XA, XRRR, Z = m["XA"], m["XRRR"], st["Z"]
    ncN = XA.shape[1]
    nk, nco = m["ncRRR"], XRRR.shape[1]
    BetaN, BetaR = st["Beta"][:ncN], st["Beta"][ncN:].reshape(nk, -1)                          # :20-21
    S = Z - XA @ BetaN                                                                         # :25,46
    for r in range(m["Pi"].shape[1]):                                                          # :33-44
        S = S - O.l_ran(st, m, r)
    iS = st["iSigma"]
    A1 = (BetaR * iS[None, :]) @ BetaR.T                                                       # :49
    A2 = XRRR.T @ XRRR                                                                         # :50
    tau = np.cumprod(st["DeltaRRR"])                                                           # :52
    iU = np.diag((st["PsiRRR"] * tau[:, None]).reshape(-1, order="F")) + np.kron(A2, A1)       # :51-54
    RiU = O.chol_upper(iU)                                                                     # :55
    U = O.chol2inv(RiU)                                                                        # :56
    mu1 = ((BetaR * iS[None, :]) @ S.T @ XRRR).reshape(-1, order="F")                          # :57
    return iU, RiU, U @ mu1                                                                    # :58


def update_wrrr(st, m, rng, it, zero_noise=False):
    """R/updatewRRR.R: returns wRRR (ncRRR x ncORRR); the caller refreshes the design."""
    nk, nco = m["ncRRR"], m["XRRR"].shape[1]
    _, RiU, mu = wrrr_moments(st, m)
    xi = np.zeros(nk * nco) if zero_noise else rng.normal(np.arange(nk * nco), 0, S_WRRR, it)
    we = mu + O.backsolve(RiU, xi)                                                             # :59
    return we.reshape(nk, nco, order="F")                                                      # :60


def update_wrrr_priors(st, m, rng, it):
    """R/updatewRRRPriors.R:3-27 (its ns is ncORRR, its nf ncRRR)."""
    nu, a1, b1, a2, b2 = (m[f] for f in ("nuRRR", "a1RRR", "b1RRR", "a2RRR", "b2RRR"))
    delta = np.array(st["DeltaRRR"], dtype=np.float64).reshape(-1)
    lam = st["wRRR"]
    nf, ns = lam.shape
    tau = np.cumprod(delta)                                                                    # :8
    lam2 = lam ** 2
    aPsi = nu / 2 + 0.5                                                                        # :10
    bPsi = nu / 2 + 0.5 * lam2 * tau[:, None]                                                  # :12
    hh, jj = np.meshgrid(np.arange(nf), np.arange(ns), indexing="ij")
    psi = rng.gamma(hh + nf * jj, S_PSI_RRR, it, aPsi, bPsi)                                   # :13
    M = psi * lam2
    rs = M.sum(axis=1)
    ad = a1 + 0.5 * ns * nf                                                                    # :15
    bd = b1 + 0.5 * np.sum(tau * rs) / delta[0]                                                # :16
    delta[0] = rng.gamma(0, S_DELTA_RRR, it, ad, bd)                                           # :17
    for h in range(1, nf):                                                                     # :18-23
        tau = np.cumprod(delta)
        ad = a2 + 0.5 * ns * (nf - h)
        bd = b2 + 0.5 * np.sum(tau[h:] * rs[h:]) / delta[h]
        delta[h] = rng.gamma(h, S_DELTA_RRR, it, ad, bd)
    return psi, delta


def sweep_rrr(st, m, rng, it, updater=None):
    """One sweep in the order of R/sampleMcmc.R:219-306 for a model with ncRRR > 0 (no
    phylogeny, no spatial level, GammaEta off): wRRR after BetaLambda (:241-247), wRRRPriors
    after LambdaPriors (:273-279); m["X"] follows wRRR."""
    up = updater or {}
    on = lambda name: up.get(name, True) is not False                  # noqa: E731
    st = dict(st)
    set_design(m, st["wRRR"])
    if on("Gamma2"):
        st["Gamma"] = O.update_gamma2(st, m, rng, it)
    if on("BetaLambda"):
        st["Beta"], st["Lambda"] = O.update_beta_lambda(st, m, rng, it)
    if on("wRRR"):
        st["wRRR"] = update_wrrr(st, m, rng, it)
        set_design(m, st["wRRR"])
    if on("GammaV"):
        st["Gamma"], st["iV"] = O.update_gamma_v(st, m, rng, it)
    if on("LambdaPriors"):
        st["Psi"], st["Delta"] = O.update_lambda_priors(st, m, rng, it)
    if on("wRRRPriors"):
        st["PsiRRR"], st["DeltaRRR"] = update_wrrr_priors(st, m, rng, it)
    if on("Eta"):
        st["Eta"] = O.update_eta(st, m, rng, it)
    if on("InvSigma"):
        st["iSigma"] = O.update_inv_sigma(st, m, rng, it)
    if on("Z"):
        st["Z"] = O.update_z(st, m, rng, it)
    return st


def synthetic_rrr(ny, ns, ncN, ncRRR, ncORRR, units=(), nf=2, seed=1, na_frac=0.0, n_normal=0, n_poisson=0,
                  XRRRScale=True):
    """A small JSDM with reduced-rank regression covariates: ncN plain columns (intercept first),
    ncORRR extra covariates entering through ncRRR components, one random level per entry of
    `units` (its number of units), the first n_normal species normal, the next n_poisson
    Poisson, the rest probit."""
    import pandas as pd

    from helpers import H
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, ncN - 1))])
    XRRR = rng.standard_normal((ny, ncORRR)) * rng.uniform(0.5, 3.0, ncORRR) + rng.normal(0, 1, ncORRR)
    w = rng.normal(0, 0.6, (ncRRR, ncORRR))
    B = rng.normal(0, 0.4, (ncN + ncRRR, ns))
    Lp = np.hstack([X, XRRR @ w.T]) @ B
    sd, ranLevels = {}, {}
    for r, npr in enumerate(units):
        pi = np.arange(ny) % npr
        rng.shuffle(pi)
        Lp = Lp + rng.standard_normal((npr, nf))[pi] @ (rng.standard_normal((nf, ns)) / np.arange(1, nf + 1)[:, None])
        name = f"lev{r}"
        sd[name] = np.array([f"u{k}" for k in pi])
        rl = H.HmscRandomLevel(units=sd[name])
        H.setPriors(rl, nfMin=nf, nfMax=nf)
        ranLevels[name] = rl
    Ylat = Lp + rng.standard_normal((ny, ns))
    Y = (Ylat > 0).astype(float)
    distr = ["probit"] * ns
    for j in range(n_normal):
        Y[:, j] = 2.0 * Ylat[:, j] + 1.0
        distr[j] = "normal"
    for j in range(n_normal, n_normal + n_poisson):
        Y[:, j] = rng.poisson(np.exp(np.clip(0.5 * Ylat[:, j], -20, 3))).astype(float)
        distr[j] = "poisson"
    if na_frac > 0:
        Y[rng.random((ny, ns)) < na_frac] = np.nan
    covn = ["(Intercept)"] + [f"x{k}" for k in range(1, ncN)]
    return H.Hmsc(Y=Y, X=X, covNames=covn, XRRR=XRRR, ncRRR=ncRRR, XRRRScale=XRRRScale, distr=distr,
                  studyDesign=pd.DataFrame(sd) if units else None, ranLevels=ranLevels if units else None)
