"""Numpy restatement of the reference's variable-selection blocks (Hmsc(XSelect = ...)), for the
tests.

The reference carries no test or fixture for XSelect models, so the restatement of
R/computeInitialParameters.R:105-109, R/updateBetaSel.R, the `list` branches of
R/updateBetaLambda.R:34-41,63-74,90-114 and the sweep order of R/sampleMcmc.R:219-306 lives here,
next to the tests that use it, and calls the existing oracle (oracle/hmsc_oracle.py) for every
other block, handing it m o Beta where a block only needs X Beta (R's per-species X[[j]] is
X diag(m_j), m_j the 0/1 column mask of species j).  Randomness follows the oracle's Philox
contract (oracle/rng.py) on the streams hmsc_amd/csrc/rng.h reserves: group g of selection i
draws uniforms(g, i, S_BETASEL, it).a, its initial value uniforms(g, i, S_INIT_BETASEL, 0).a.

updateBetaSel is written cell by cell from Z, E and the per-species masked X -- not through the
Grams X'X and X'Z the device uses -- so the two are independent evaluations.

One deliberate difference from Hmsc 3.0-4: R/updateBetaSel.R:53,79 evaluates
pnorm(q = Z, mean = E, sd, log.p = TRUE), a CDF where the density of Z belongs; with it the
Metropolis step does not leave the conditional of BetaSel invariant.  density="dnorm" (the
default, and what the device computes) uses the Gaussian log-density; density="pnorm" restates
the reference literally, for the test that documents the difference.
"""
import numpy as np
from scipy import stats

from helpers import H, O, oracle_model

S_BETASEL = 15
S_INIT_BETASEL = 57


def sel_model(hM):
    """oracle_model(hM) plus the selections (0-based covGroup and spGroup)."""
    m = oracle_model(hM)
    m["XSelect"] = [dict(cov=np.asarray(x["covGroup"]) - 1, spg=np.asarray(x["spGroup"]) - 1,
                         q=np.asarray(x["q"], dtype=np.float64)) for x in hM["XSelect"]]
    return m


def column_mask(m, bsel):
    """m[c, j] = 0 where a selection holding column c is off for j's group (R/sampleMcmc.R:179-195)."""
    nc, ns = m["X"].shape[1], m["Y"].shape[1]
    M = np.ones((nc, ns))
    for xs, b in zip(m["XSelect"], bsel):
        off = ~np.asarray(b, dtype=bool)[xs["spg"]]
        M[np.ix_(xs["cov"], np.nonzero(off)[0])] = 0.0
    return M


def masked(st, m):
    """The state as a block that only forms X Beta sees it: Beta[, j] replaced by m_j o Beta[, j]."""
    return dict(st, Beta=column_mask(m, st["BetaSel"]) * st["Beta"])


def init_betasel(m, rng):
    """R/computeInitialParameters.R:105-109."""
    return [rng.uniforms(np.arange(len(xs["q"])), i, S_INIT_BETASEL, 0)[0] < xs["q"]
            for i, xs in enumerate(m["XSelect"])]


def compute_initial_parameters(m, rng, nf=None):
    """computeInitialParameters with ncsel > 0: hM$X is a matrix there, so the initial Z is drawn
    from the unmasked X (:34-50,229-254); BetaSel is drawn on its own stream."""
    st = O.compute_initial_parameters(m, rng, nf=nf)
    st["BetaSel"] = init_betasel(m, rng)
    return st


def update_beta_sel(st, m, rng, it, density="dnorm"):
    """R/updateBetaSel.R.  Returns (BetaSel, info): info[i] holds, per group of selection i, the
    log ratio lldif + pridif as evaluated, the uniform it met, and the scale of the evaluation,
    the sum of the absolute values of the cell terms that entered lldif."""
    X1, Z, iS = m["X"], st["Z"], st["iSigma"]
    ny, ns = Z.shape
    std = iS ** -0.5                                                                   # :24
    bsel = [np.array(b, dtype=bool) for b in st["BetaSel"]]
    M = column_mask(m, bsel)                                                           # :30-41
    E = np.empty((ny, ns))
    for j in range(ns):
        E[:, j] = (X1 * M[:, j][None, :]) @ st["Beta"][:, j]                           # :43-44
    for r in range(m["Pi"].shape[1]):                                                  # :46-49
        E = E + O.l_ran(st, m, r)

    def ll_of(Ej, j):
        if density == "pnorm":                                                         # :53,79 as in the reference
            return stats.norm.logcdf(Z[:, j], loc=Ej, scale=std[j])
        return -0.5 * iS[j] * (Z[:, j] - Ej) ** 2                                      # (the constant cancels)

    ll = np.column_stack([ll_of(E[:, j], j) for j in range(ns)])                       # :51-54
    info = []
    for i, xs in enumerate(m["XSelect"]):                                              # :57
        ng = len(xs["q"])
        lr, uu, sc = np.empty(ng), np.empty(ng), np.empty(ng)
        for g in range(ng):                                                            # :59
            new = not bsel[i][g]                                                       # :60
            fsp = np.nonzero(xs["spg"] == g)[0]                                        # :62
            ENew, llNew = E.copy(), ll.copy()
            scale = 0.0
            for j in fsp:                                                              # :64-80
                d = X1[:, xs["cov"]] @ st["Beta"][xs["cov"], j]
                ENew[:, j] = E[:, j] + d if new else E[:, j] - d
                llNew[:, j] = ll_of(ENew[:, j], j)
                rj = Z[:, j] - E[:, j]
                scale += iS[j] * np.sum(0.5 * d * d + np.abs(rj * d))
            lldif = np.sum(llNew[:, fsp]) - np.sum(ll[:, fsp])                         # :81
            q = xs["q"][g]
            with np.errstate(divide="ignore"):
                pridif = np.log(q) - np.log(1 - q) if new else np.log(1 - q) - np.log(q)   # :82-87
            u = float(rng.uniforms(g, i, S_BETASEL, it)[0])
            lr[g], uu[g], sc[g] = lldif + pridif, u, scale
            with np.errstate(over="ignore"):
                if np.exp(lldif + pridif) > u:                                         # :89-93
                    bsel[i][g] = new
                    E, ll = ENew, llNew
        info.append(dict(logratio=lr, u=uu, scale=sc))
    return bsel, info


def beta_lambda_moments(st, m):
    """Per-species precision and mean of updateBetaLambda's `list` branch, C = NULL
    (R/updateBetaLambda.R:34-41,63-74,90-114): XEta[[j]] = [X[[j]], Eta_1[Pi_1,], ...]."""
    Y, Z = m["Y"], st["Z"]
    nc = m["X"].shape[1]
    ns = Y.shape[1]
    XEta, priorLambda = O._xeta_and_prior(st, m)
    K = XEta.shape[1]
    M = column_mask(m, st["BetaSel"])
    Mu = np.concatenate([st["Gamma"] @ m["Tr"].T, np.zeros((K - nc, ns))])
    iS = st["iSigma"]
    Yx = ~np.isnan(Y)
    precs, means = np.empty((ns, K, K)), np.empty((K, ns))
    for j in range(ns):
        Xj = XEta.copy()
        Xj[:, :nc] = Xj[:, :nc] * M[:, j][None, :]                                     # :34-41
        P = np.zeros((K, K))
        P[:nc, :nc] = st["iV"]
        P[np.diag_indices(K)] = np.concatenate([np.diag(st["iV"]), priorLambda[:, j]])
        o = Yx[:, j]
        iU = P + (Xj[o].T @ Xj[o]) * iS[j]                                             # :90-114
        precs[j] = iU
        means[:, j] = np.linalg.solve(iU, P @ Mu[:, j] + (Xj[o].T @ Z[o, j]) * iS[j])
    return precs, means


def update_beta_lambda(st, m, rng, it, zero_noise=False):
    nc, ns, nr = m["X"].shape[1], m["Y"].shape[1], m["Pi"].shape[1]
    precs, means = beta_lambda_moments(st, m)
    K = means.shape[0]
    BL = np.empty((K, ns))
    for j in range(ns):
        RiU = O.chol_upper(precs[j])
        xi = np.zeros(K) if zero_noise else rng.normal(j, np.arange(K), O.R.S_BETALAMBDA, it)
        BL[:, j] = means[:, j] + O.backsolve(RiU, xi)
    Lambda, off = [], nc
    for r in range(nr):
        nf = st["Lambda"][r].shape[0]
        Lambda.append(BL[off:off + nf].copy())
        off += nf
    return BL[:nc].copy(), Lambda


def sweep_sel(st, m, rng, it, updater=None, adapt_nf=None, info_out=None):
    """One sweep in the order of R/sampleMcmc.R:219-306 for a model with ncsel > 0 (Gamma2 and
    GammaEta off, :207-216; no phylogeny, no spatial level): BetaSel after BetaLambda (:249-254).
    info_out: a list that receives update_beta_sel's info of this sweep."""
    up = updater or {}
    on = lambda name: up.get(name, True) is not False                  # noqa: E731
    st = dict(st)
    if on("BetaLambda"):
        st["Beta"], st["Lambda"] = update_beta_lambda(st, m, rng, it)
    if on("BetaSel"):
        st["BetaSel"], info = update_beta_sel(st, m, rng, it)
        if info_out is not None:
            info_out.append(info)
    if on("GammaV"):
        st["Gamma"], st["iV"] = O.update_gamma_v(st, m, rng, it)       # the raw Beta
    if on("LambdaPriors"):
        st["Psi"], st["Delta"] = O.update_lambda_priors(st, m, rng, it)
    if on("Eta"):
        st["Eta"] = O.update_eta(masked(st, m), m, rng, it)
    if on("InvSigma"):
        st["iSigma"] = O.update_inv_sigma(masked(st, m), m, rng, it)
    if on("Z"):
        st["Z"] = O.update_z(masked(st, m), m, rng, it)
    for r in range(m["Pi"].shape[1]):                                  # :296-306
        if adapt_nf is not None and it <= adapt_nf[r]:
            e, l, a, p, d = O.update_nf(st, m, r, rng, it)
            for k, v in (("Eta", e), ("Lambda", l), ("Alpha", a), ("Psi", p), ("Delta", d)):
                st[k] = list(st[k])
                st[k][r] = v
    return st


def synthetic_sel(ny, ns, nc, selections, units=(), nf=2, seed=1, na_frac=0.0, n_normal=0, effects=None,
                  nf_max=None):
    """A small JSDM with variable selection: nc columns (intercept first), one random level per
    entry of `units` (its number of units), the first n_normal species normal, the rest probit.
    selections: dicts(covGroup (1-based), spGroup (1-based, length ns), q).  effects: an nc x ns
    matrix of true coefficients (default: random).  nf_max: the levels adapt between nf and it."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, nc - 1))])
    B = rng.normal(0, 0.4, (nc, ns)) if effects is None else np.asarray(effects, dtype=np.float64)
    Lp = X @ B
    sd, ranLevels = {}, {}
    for r, npr in enumerate(units):
        pi = np.arange(ny) % npr
        rng.shuffle(pi)
        Lp = Lp + rng.standard_normal((npr, nf))[pi] @ (rng.standard_normal((nf, ns)) / np.arange(1, nf + 1)[:, None])
        name = f"lev{r}"
        sd[name] = np.array([f"u{k}" for k in pi])
        rl = H.HmscRandomLevel(units=sd[name])
        H.setPriors(rl, nfMin=nf, nfMax=nf if nf_max is None else nf_max)
        ranLevels[name] = rl
    Ylat = Lp + rng.standard_normal((ny, ns))
    Y = (Ylat > 0).astype(float)
    distr = ["probit"] * ns
    for j in range(n_normal):
        Y[:, j] = 2.0 * Ylat[:, j] + 1.0
        distr[j] = "normal"
    if na_frac > 0:
        Y[rng.random((ny, ns)) < na_frac] = np.nan
    covn = ["(Intercept)"] + [f"x{k}" for k in range(1, nc)]
    return H.Hmsc(Y=Y, X=X, covNames=covn, XSelect=selections, distr=distr,
                  studyDesign=pd.DataFrame(sd) if units else None, ranLevels=ranLevels if units else None)
