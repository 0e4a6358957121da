"""Posterior output layout and diagnostics (host side).

* ``convertToCodaObject`` — R/convertToCodaObject.r:36-290: the parameter naming
  and vectorisation order of the reference's coda objects ("B[cov (C1), sp (S1)]",
  Beta as.vector covariate-fastest, Lambda as.vector(t(.)) species-fastest,
  Omega = crossprod(Lambda)), returned as ``{name: [chain arrays (samples, p)]}``
  plus ``{name: column names}``.
* ``effectiveSize`` — coda::effectiveSize (spectrum0.ar: AR order by AIC via Yule-Walker,
  R's ar.yw.default) on the device (post.hip), used for the Beta ESS/sec metric;
  ``gelman_diag`` — coda::gelman.diag(multivariate=FALSE) on the host (m x p numbers).
* ``computeVariancePartitioning``, ``computeAssociations``, ``getPostEstimate(.., "Omega")``
  — their loops over posterior samples on the device (post.hip); checkers in
  oracle/post_oracle.py.
* ``poolMcmcChains``, ``getPostEstimate``, ``computeWAIC`` — R/poolMcmcChains.R,
  R/getPostEstimate.R, R/computeWAIC.R:25-131 (host loop, or the whole pass on the device:
  hmsc_waic, waic.hip).
"""
import numpy as np
from scipy import special, stats
from scipy.special import log_ndtr

from . import _lib as L


def poolMcmcChains(postList, start=1, thin=1):
    out = []
    for chain in postList:
        out.extend(chain[start - 1::thin])
    return out


def convertToCodaObject(hM, start=1, spNamesNumbers=(True, True), covNamesNumbers=(True, True),
                        trNamesNumbers=(True, True), Beta=True, Gamma=True, V=True, Sigma=True, Rho=True,
                        Eta=True, Lambda=True, Alpha=True, Omega=True, Psi=True, Delta=True):
    """R/convertToCodaObject.r:36-290: per chain, one (samples, P) matrix per parameter and
    its column names (the coda mcmc.list layout)."""
    def nm(names, numbers, prefix):                                        # :54-92
        res = []
        for k, n in enumerate(names):
            parts = []
            if numbers[0]:
                parts.append(str(n))
            if numbers[1]:
                parts.append(f"({prefix}{k + 1})")
            res.append(" ".join(parts))
        return res

    sp = nm(hM.spNames, spNamesNumbers, "S")
    cov = nm(hM.covNames, covNamesNumbers, "C")
    tr = nm(hM.trNames, trNamesNumbers, "T")
    out, cols = {}, {}
    chains = [c[start - 1:] for c in hM.postList]
    if Beta:                                                                # :131-135
        out["Beta"] = [np.stack([s["Beta"].reshape(-1, order="F") for s in c]) for c in chains]
        cols["Beta"] = [f"B[{cv}, {s}]" for s in sp for cv in cov]
    if Gamma:
        out["Gamma"] = [np.stack([s["Gamma"].reshape(-1, order="F") for s in c]) for c in chains]
        cols["Gamma"] = [f"G[{cv}, {t}]" for t in tr for cv in cov]
    if V:
        out["V"] = [np.stack([s["V"].reshape(-1, order="F") for s in c]) for c in chains]
        cols["V"] = [f"V[{c1}, {c2}]" for c2 in cov for c1 in cov]
    if Sigma:
        out["Sigma"] = [np.stack([np.asarray(s["sigma"]) for s in c]) for c in chains]
        cols["Sigma"] = [f"Sig[{s}]" for s in sp]
    if Rho and hM.C is not None:
        out["Rho"] = [np.array([[s["rho"]] for s in c]) for c in chains]
        cols["Rho"] = ["Rho"]
    for r in range(hM.nr):
        nfMax = max(c[0]["Lambda"][r].shape[0] for c in chains)
        if Eta:                                                             # :171-176
            units = list(_levels(hM.dfPi[hM.rLNames[r]])) if hM.dfPi is not None else \
                [str(q + 1) for q in range(int(hM.np[r]))]
            out.setdefault("Eta", []).append(
                [np.stack([_pad_cols(s["Eta"][r], nfMax).reshape(-1, order="F") for s in c]) for c in chains])
            cols.setdefault("Eta", []).append(
                [f"Eta{r + 1}[{u}, factor{h + 1}]" for h in range(nfMax) for u in units])
        if Lambda:                                                          # :178-183 as.vector(t(Lambda))
            out.setdefault("Lambda", []).append(
                [np.stack([_pad_rows(s["Lambda"][r], nfMax).T.reshape(-1, order="F") for s in c]) for c in chains])
            cols.setdefault("Lambda", []).append(
                [f"Lambda{r + 1}[{s}, factor{h + 1}]" for h in range(nfMax) for s in sp])
        if Omega:                                                           # :184-188 crossprod(Lambda)
            out.setdefault("Omega", []).append(
                [np.stack([(s["Lambda"][r].T @ s["Lambda"][r]).reshape(-1, order="F") for s in c]) for c in chains])
            cols.setdefault("Omega", []).append([f"Omega{r + 1}[{a}, {b}]" for b in sp for a in sp])
        if Alpha:                                                           # :189-195 alphapw[Alpha, 1], 0-padded
            apw = np.asarray(hM.rL[r].alphapw)[:, 0] if hM.rL[r].sDim else None
            rows = []
            for c in chains:
                m = np.zeros((len(c), nfMax))
                for k, smp in enumerate(c):
                    a = np.asarray(smp["Alpha"][r], dtype=np.int64).ravel()
                    m[k, :len(a)] = apw[a - 1] if apw is not None else 0.0
                rows.append(m)
            out.setdefault("Alpha", []).append(rows)
            cols.setdefault("Alpha", []).append([f"Alpha{r + 1}[factor{h + 1}]" for h in range(nfMax)])
        if Psi:                                                             # :197-203
            out.setdefault("Psi", []).append(
                [np.stack([_pad_rows(s["Psi"][r], nfMax).T.reshape(-1, order="F") for s in c]) for c in chains])
            cols.setdefault("Psi", []).append([f"Psi{r + 1}[{s}, factor{h + 1}]" for h in range(nfMax) for s in sp])
        if Delta:                                                           # :205-210 0-padded
            out.setdefault("Delta", []).append(
                [np.stack([_pad_rows(s["Delta"][r], nfMax, fill=0.0).reshape(-1) for s in c]) for c in chains])
            cols.setdefault("Delta", []).append([f"Delta{r + 1}[factor{h + 1}]" for h in range(nfMax)])
    return out, cols


def _levels(col):
    """levels(hM$dfPi[, r]): the rule hM$Pi was built with (model._factor_levels)."""
    from .model import _factor_levels
    return [str(v) for v in _factor_levels(col)]


def _pad_rows(a, n, fill=0.0):
    a = np.atleast_2d(a)
    if a.shape[0] >= n:
        return a
    return np.vstack([a, np.full((n - a.shape[0], a.shape[1]), fill)])


def _pad_cols(a, n):
    if a.shape[1] >= n:
        return a
    return np.hstack([a, np.zeros((a.shape[0], n - a.shape[1]))])


# ---------------------------------------------------------------------------
# coda::effectiveSize on the device (hmsc_effective_size, post.hip; the numpy restatement
# of spectrum0.ar with R's ar.yw.default is the checker in oracle/post_oracle.py)
# ---------------------------------------------------------------------------
def _device():
    """The device post-processing runs on: HMSC_POST_DEVICE, else 0."""
    import os
    return int(os.environ.get("HMSC_POST_DEVICE", "0"))


def spectrum0_ar(x, device=None):
    """coda::spectrum0.ar for every column of x (n, p): (spec, AR order), on the device.
    spec follows from the ESS: spec = n var / ESS (0 for a constant column)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    ess, order = _ess_device(x, device)
    var = x.var(axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        spec = np.where(ess == 0, 0.0, x.shape[0] * var / ess)
    return spec, order


def _ess_device(x, device=None):
    n, p = x.shape
    xf = np.asfortranarray(x)
    ess = np.zeros(p)
    order = np.zeros(p, dtype=np.int32)
    L.check(L.lib().hmsc_effective_size(_device() if device is None else int(device), n, p,
                                        xf.ctypes.data_as(L.dp), L.fptr(ess), L.iptr(order)))
    return ess, order


def effectiveSize(chains, device=None):
    """coda::effectiveSize for an mcmc.list: per-chain n var / spec0 (device), summed over chains."""
    if isinstance(chains, np.ndarray):
        chains = [chains]
    total = 0.0
    for x in chains:
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x[:, None]
        total = total + _ess_device(x, device)[0]
    return total


def gelman_diag(chains, confidence=0.95):
    """coda::gelman.diag(multivariate=FALSE): point estimate and upper CI of the PSRF."""
    X = np.stack([np.asarray(c, dtype=np.float64) for c in chains])      # (m, n, p)
    return gelman_from_moments(X.mean(axis=1), X.var(axis=1, ddof=1), X.shape[1], confidence)


def gelman_from_moments(xbar, s2, n, confidence=0.95):
    """gelman_diag from the chains' moments: xbar, s2 (m, ...) the per-chain means and ddof = 1
    variances of n samples each.  The PSRF needs nothing else of the chains."""
    xbar = np.asarray(xbar, dtype=np.float64)
    s2 = np.asarray(s2, dtype=np.float64)
    m = xbar.shape[0]
    W = s2.mean(axis=0)
    B = n * xbar.var(axis=0, ddof=1)
    muhat = xbar.mean(axis=0)
    var_w = s2.var(axis=0, ddof=1) / m
    var_b = (2 * B ** 2) / (m - 1)
    cov = lambda a, b: ((a - a.mean(0)) * (b - b.mean(0))).sum(0) / (m - 1)   # noqa: E731
    cov_wb = (n / m) * (cov(s2, xbar ** 2) - 2 * muhat * cov(s2, xbar))
    V = (n - 1) * W / n + (1 + 1 / m) * B / n
    var_V = ((n - 1) ** 2 * var_w + (1 + 1 / m) ** 2 * var_b + 2 * (n - 1) * (1 + 1 / m) * cov_wb) / n ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        df_V = 2 * V ** 2 / var_V
        df_adj = (df_V + 3) / (df_V + 1)
        W_df = 2 * W ** 2 / var_w
        R2_fixed = (n - 1) / n
        R2_random = (1 + 1 / m) * (1 / n) * (B / W)
        point = np.sqrt(df_adj * (R2_fixed + R2_random))
        upper = np.sqrt(df_adj * (R2_fixed + _f_upper_quantile((1 - confidence) / 2, m - 1, W_df) * R2_random))
    return point, upper


def _f_upper_quantile(tail, d1, d2):
    """R's qf(1 - tail, d1, d2) through the inverse incomplete beta function: with X ~ F(d1, d2),
    Z = d1 X / (d1 X + d2) ~ Beta(d1 / 2, d2 / 2).  The odds are taken from whichever of z and
    1 - z is the small one, so nothing cancels.  scipy's stats.f.ppf loses about d2 * 1e-16 of the
    quantile (3e-7 at d2 = 2e10, the W_df of two chains whose variances nearly agree, and
    per cent at 1e14) and jumps by as much from one ulp of d2 to the next; this form stays within
    1e-15 of a 40-digit evaluation from d2 = 0.5 to 1e14 (tests/test_host_omega_diag.py), tends to
    qchisq(., d1) / d1, and differs from stats.f.ppf by at most 5e-12 for d2 <= 1e4."""
    d2 = np.asarray(d2, dtype=np.float64)
    z = special.betaincinv(d1 / 2, d2 / 2, 1 - tail)
    w = special.betaincinv(d2 / 2, d1 / 2, tail)          # = 1 - z, formed from the other tail
    return np.where(z <= 0.5, d2 * z / (d1 * (1 - z)), d2 * (1 - w) / (d1 * w))


def getPostEstimate(hM, parName, r=1, x=None, q=(), chainIndex=None, start=1):
    """R/getPostEstimate.R: posterior mean and support (P(>0)) of Beta/Gamma/V/Sigma/Omega."""
    postList = hM.postList if chainIndex is None else [hM.postList[i] for i in chainIndex]
    post = poolMcmcChains(postList, start=start)
    if parName == "Omega" and not q:   # mean and supports summed on the device (hmsc_post_omega)
        o = _omega_device(post, r - 1, hM.ns)
        return dict(mean=o["mean_omega"], support=o["support"], supportNeg=o["support_neg"])
    if parName == "Omega":
        vals = np.stack([s["Lambda"][r - 1].T @ s["Lambda"][r - 1] for s in post])
    elif parName == "Sigma":
        vals = np.stack([np.asarray(s["sigma"]) for s in post])
    else:
        vals = np.stack([np.asarray(s[parName]) for s in post])
    res = dict(mean=vals.mean(axis=0), support=(vals > 0).mean(axis=0), supportNeg=(vals < 0).mean(axis=0))
    if q:
        res["q"] = np.quantile(vals, q, axis=0)
    return res


def computeWAIC(hM, ghN=11, device=None, byUnit=False):
    """R/computeWAIC.R:25-131.  Poisson columns integrate the lognormal intensity with
    ghN-point Gauss-Hermite quadrature (:108-118); ``dpois(Y, exp(gX))`` there recycles the
    whole ny x ns Y column-major against the ny x cN x ghN node array, which is reproduced
    as written (it only equals the per-cell likelihood when every species is Poisson).

    ``device=None`` is the host loop below, the reference's literal form.  An integer runs the
    whole pass on that device (hmsc_waic, waic.hip): the same cell terms, with the sums over
    quadrature nodes and over samples max-shifted, so it stays finite where ``exp`` of a site's
    log-likelihood underflows (ns in the hundreds) and equals the host value to rounding
    elsewhere.  ``byUnit=True`` returns dict(WAIC=, Bl=, V=) with the per-site pieces."""
    post = poolMcmcChains(hM.postList)
    if device is not None:
        res = _waic_device(hM, post, ghN, int(device))
        return dict(WAIC=res["WAIC"], Bl=res["Bl"], V=res["V"]) if byUnit else res["WAIC"]
    val = _waic_val_host(hM, post, ghN)
    Bl = -np.log(np.mean(np.exp(val), axis=0))
    Vv = val.var(axis=0, ddof=1)
    if byUnit:
        return dict(WAIC=float(np.mean(Bl + Vv)), Bl=Bl, V=Vv)
    return float(np.mean(Bl + Vv))


def _waic_val_host(hM, post, ghN=11):
    """val (samples, ny) of R/computeWAIC.R:55-122: every sample's log-likelihood of each site,
    summed over species."""
    Y, X, Pi = hM.Y, hM.X, hM.Pi
    fam = hM.distr[:, 0]
    normal, probit, pois = fam == 1, fam == 2, fam == 3
    if pois.any():
        gx, gw = np.polynomial.hermite.hermgauss(ghN)   # statmod::gauss.quad(kind="hermite")
        cN = int(pois.sum())
        ii, cc, gg = np.meshgrid(np.arange(hM.ny), np.arange(cN), np.arange(ghN), indexing="ij")
        Yrec = Y.ravel(order="F")[(ii + hM.ny * cc + hM.ny * cN * gg) % Y.size]
    na = np.isnan(Y)
    vals = []
    from .sampler import level_lran, x_unit_order
    xs = [x_unit_order(hM, r, rl) if rl.xDim else None for r, rl in enumerate(hM.rL or [])]
    for s in post:
        E = X @ s["Beta"]
        for r in range(hM.nr):
            E = E + level_lran(s["Eta"][r], s["Lambda"][r], Pi[:, r] - 1, xs[r])
        std = np.asarray(s["sigma"]) ** -0.5
        Lr = np.zeros(hM.ny)
        if normal.any():
            t = stats.norm.logpdf(Y[:, normal], loc=E[:, normal], scale=std[normal][None, :])
            t[na[:, normal]] = 0
            Lr += t.sum(axis=1)
        if probit.any():
            pz0 = log_ndtr(-E[:, probit])
            pz1 = log_ndtr(E[:, probit])
            Yp = Y[:, probit]
            t = pz1 * Yp + pz0 * (1 - Yp)
            t[na[:, probit]] = 0
            Lr += t.sum(axis=1)
        if pois.any():
            gX = E[:, pois][:, :, None] + np.sqrt(2.0) * gx[None, None, :] * std[pois][None, :, None]
            like = stats.poisson.pmf(Yrec, np.exp(gX))
            t = np.log(np.sum(like * gw[None, None, :], axis=2) / np.sqrt(np.pi))
            t[na[:, pois]] = 0
            Lr += t.sum(axis=1)
        vals.append(Lr)
    return np.stack(vals)


def _waic_args(hM, post, ghN=11, device=0, sample_chunk=0):
    """hmsc_waic_args for the pooled samples ``post`` (include/hmsc_amd.h): sample-major stacks
    of column-major matrices, every level's nf padded to its maximum over the samples (zero
    factors), a covariate-dependent level as one device level per column of rL$x with
    Eta * x[, k] and Lambda[, , k] (as predict marshals its levels).  Returns (args, keep,
    dims): keep holds the arrays the pointers refer to, dims = dict(S, nr, np, nf)."""
    if int(getattr(hM, "ncRRR", 0) or 0) > 0:
        raise ValueError("computeWAIC: a model with reduced-rank covariates (ncRRR > 0) is not supported: the "
                         "recorded Beta has nc rows and hM$X only ncNRRR columns")
    S = len(post)
    if S < 2:
        raise ValueError(f"computeWAIC: at least 2 posterior samples are needed (nsamples = {S}): the variance "
                         "over samples has ddof = 1")
    from .sampler import x_unit_order
    keep = []
    a = L.hmsc_waic_args()
    X = np.asarray(hM.X, dtype=np.float64)
    a.ny, a.ns, a.nc, a.nsamples = hM.ny, hM.ns, X.shape[1], S
    a.ghN, a.device, a.sample_chunk = int(ghN), int(device), int(sample_chunk)
    a.Y = L.colmajor_ptr(hM.Y, keep)
    a.X = L.colmajor_ptr(X, keep)
    a.Beta = L.fptr(_flat(keep, [np.asarray(s_["Beta"], dtype=np.float64) for s_ in post]))
    a.sigma = L.fptr(_flat(keep, [np.asarray(s_["sigma"], dtype=np.float64) for s_ in post]))
    a.family = L.colmajor_ptr(hM.distr[:, 0], keep, np.int32)
    gx, gw = np.polynomial.hermite.hermgauss(int(ghN))   # statmod::gauss.quad(kind="hermite")
    a.gx = L.fptr(_keep(keep, np.ascontiguousarray(gx)))
    a.gw = L.fptr(_keep(keep, np.ascontiguousarray(gw)))
    nps, nfs, pis = [], [], []
    for r, rl in enumerate(hM.rL or []):
        xu = x_unit_order(hM, r, rl) if int(rl.xDim or 0) else None
        nf, stacks = stack_device_levels(keep, [s_["Eta"][r] for s_ in post], [s_["Lambda"][r] for s_ in post], xu)
        for eta_k, lam_k in stacks:
            d = len(nps)
            if d >= L.MAX_LEVELS:
                raise ValueError(f"computeWAIC: at most {L.MAX_LEVELS} device levels")
            a.Eta[d] = L.fptr(eta_k)
            a.Lambda[d] = L.fptr(lam_k)
            nps.append(np.asarray(post[0]["Eta"][r]).shape[0])
            nfs.append(nf)
            pis.append(np.asarray(hM.Pi)[:, r])
    a.nr = len(nps)
    if nps:
        a.Pi = L.colmajor_ptr(np.column_stack(pis), keep, np.int32)
        a.np = L.colmajor_ptr(nps, keep, np.int32)
        a.nf = L.colmajor_ptr(nfs, keep, np.int32)
    return a, keep, dict(S=S, nr=len(nps), np=nps, nf=nfs)


def stack_device_levels(keep, etas, lams, x=None):
    """One random level's samples as device levels of the C ABI (hmsc_predict_args,
    hmsc_waic_args): etas (units x nf_s) and lams (nf_s x ns, or nf_s x ns x xDim) per sample, nf
    zero-padded to its maximum over the samples (updateNf may change it), each stacked
    sample-major as column-major matrices.  x (units x xDim, the units' rows of rL$x) marks a
    covariate-dependent level: one device level per column k, with Eta * x[, k] and Lambda[, , k]
    (R/predict.R:171-176, R/computeWAIC.R:66-70).  Returns (nf, [(Eta stack, Lambda stack), ...]);
    keep holds the stacks."""
    etas = [np.asarray(e, dtype=np.float64) for e in etas]
    lams = [np.asarray(lm, dtype=np.float64) for lm in lams]
    nf = max(e.shape[1] for e in etas)
    etas = [_pad_cols(e, nf) for e in etas]
    lams = [np.pad(lm, ((0, nf - lm.shape[0]),) + ((0, 0),) * (lm.ndim - 1)) for lm in lams]
    out = []
    for k in range(1 if x is None else x.shape[1]):
        ek = etas if x is None else [e * x[:, k:k + 1] for e in etas]
        lk = lams if x is None else [lm[:, :, k] for lm in lams]
        out.append((_flat(keep, ek), _flat(keep, lk)))
    return nf, out


def _waic_device(hM, post, ghN, device, sample_chunk=0):
    """computeWAIC on the device: dict(WAIC, Bl (ny), V (ny), val (S, ny))."""
    a, keep, dims = _waic_args(hM, post, ghN, device, sample_chunk)
    waic = np.zeros(1)
    site = np.zeros(2 * hM.ny)
    val = np.zeros((dims["S"], hM.ny))
    L.check(L.lib().hmsc_waic(L.C.byref(a), L.fptr(waic), L.fptr(site), L.fptr(val)))
    return dict(WAIC=float(waic[0]), Bl=site[:hM.ny].copy(), V=site[hM.ny:].copy(), val=val)


def computeVariancePartitioning(hM, group=None, groupnames=None, start=1, device=None):
    """R/computeVariancePartitioning.R:37-204 (X a matrix, na.ignore=FALSE), the loop over
    samples on the device (hmsc_variance_partitioning, post.hip).

    Reproduces the reference's loop ``for (i in 1:hM$samples)`` over the *pooled* list
    (:125), i.e. with nChains > 1 only the first chain's samples enter (SURVEY.md
    Appendix B quirk 4).  Returns dict(vals (ngroups+nr, ns), R2T=dict(Beta, Y), group,
    groupnames, rownames).
    """
    ns, nc, nr = hM.ns, hM.nc, hM.nr
    if group is None:                                                      # :42-51
        if nc > 1:
            group = np.r_[1, np.arange(1, nc)]
            groupnames = list(hM.covNames[1:nc])
        else:
            group = np.array([1])
            groupnames = [hM.covNames[0]]
    group = np.asarray(group)
    ngroups = int(group.max())
    X = np.asarray(hM.X, dtype=np.float64)
    Tr = np.asarray(hM.Tr, dtype=np.float64)
    cM = np.cov(X, rowvar=False).reshape(nc, nc)                           # :66
    post = poolMcmcChains(hM.postList, start=start)[:hM.samples]            # :125 (quirk above)
    S = len(post)
    keep = []
    a = L.hmsc_vp_args()
    a.device = _default_device_of(device)
    a.ny, a.ns, a.nc, a.nt, a.S, a.ngroups, a.nr = hM.ny, ns, nc, Tr.shape[1], S, ngroups, nr
    a.group = L.colmajor_ptr(group.astype(np.int32), keep, np.int32)
    a.X = L.colmajor_ptr(X, keep)
    a.Tr = L.colmajor_ptr(Tr, keep)
    a.cM = L.colmajor_ptr(cM, keep)
    a.Beta = L.fptr(_flat(keep, [np.asarray(s_["Beta"], dtype=np.float64) for s_ in post]))
    a.Gamma = L.fptr(_flat(keep, [np.asarray(s_["Gamma"], dtype=np.float64) for s_ in post]))
    nfs = np.zeros((max(1, nr), S), dtype=np.int32)
    for r in range(nr):
        nfm = max(int(np.asarray(s_["Lambda"][r]).shape[0]) for s_ in post)
        lam = np.zeros((S, nfm, ns))
        for k, s_ in enumerate(post):
            l_ = np.asarray(s_["Lambda"][r], dtype=np.float64)
            nfs[r, k] = l_.shape[0]
            lam[k, :l_.shape[0]] = l_
        a.nfmax[r] = nfm
        a.Lambda[r] = L.fptr(_flat(keep, list(lam)))
    a.nf = L.iptr(_keep(keep, np.ascontiguousarray(nfs.ravel())))
    slot = nc + 1 + ns * (1 + nr + ngroups)
    out = np.zeros(slot)
    L.check(L.lib().hmsc_variance_partitioning(L.C.byref(a), L.fptr(out)))
    R2T_Beta, R2T_Y = out[:nc], float(out[nc])
    fixed = out[nc + 1:nc + 1 + ns]
    random = out[nc + 1 + ns:nc + 1 + ns * (1 + nr)].reshape(nr, ns).T
    fixedsplit = out[nc + 1 + ns * (1 + nr):].reshape(ngroups, ns).T
    vals = np.zeros((ngroups + nr, ns))                                    # :180-187
    for g in range(ngroups):
        vals[g] = fixed * fixedsplit[:, g]
    for r in range(nr):
        vals[ngroups + r] = random[:, r]
    rl = list(getattr(hM, "rLNames", None) or [f"level{r + 1}" for r in range(nr)])
    return dict(vals=vals, R2T=dict(Beta=R2T_Beta, Y=R2T_Y), group=group, groupnames=groupnames,
                rownames=list(groupnames) + [f"Random: {n}" for n in rl])


def _keep(keep, arr):
    keep.append(arr)
    return arr


def _flat(keep, mats):
    """Samples stacked as consecutive column-major matrices (the C side's S x (m x n))."""
    return _keep(keep, np.ascontiguousarray(np.concatenate([np.asarray(m_).ravel(order="F") for m_ in mats])))


def _default_device_of(device):
    return _device() if device is None else int(device)


def computeAssociations(hM, start=1, thin=1, device=None):
    """R/computeAssociations.R: per random level, dict(mean, support) of
    cov2cor(crossprod(Lambda)) over the pooled samples, on the device (hmsc_post_omega)."""
    post = poolMcmcChains(hM.postList, start=start, thin=thin)
    out = []
    for r in range(hM.nr):
        res = _omega_device(post, r, hM.ns, device)
        out.append(dict(mean=res["mean_cor"], support=res["support"]))
    return out


def _omega_device(post, r, ns, device=None):
    S = len(post)
    nfm = max(int(np.asarray(s_["Lambda"][r]).shape[0]) for s_ in post)
    lam = np.zeros((S, ns, nfm))   # C order (S, ns, nfm) = each sample nfm x ns column-major
    nf = np.zeros(S, dtype=np.int32)
    for k, s_ in enumerate(post):
        l_ = np.asarray(s_["Lambda"][r], dtype=np.float64)
        nf[k] = l_.shape[0]
        lam[k, :, :l_.shape[0]] = l_.T
    outs = {k: np.zeros((ns, ns), order="F") for k in ("mean_cor", "support", "support_neg", "mean_omega")}
    L.check(L.lib().hmsc_post_omega(_default_device_of(device), S, ns, nfm, L.iptr(nf), L.fptr(lam),
                                    *[outs[k].ctypes.data_as(L.dp) for k in ("mean_cor", "support", "support_neg",
                                                                             "mean_omega")]))
    return outs


# ---------------------------------------------------------------------------
# Convergence diagnostics (vignette_3_multivariate_high.Rmd:160-181: effectiveSize and
# gelman.diag of the coda object's blocks).  Omega's ns^2 series of every chain are formed and
# diagnosed on the device from the chains' Lambda (hmsc_omega_diagnostics, post.hip); only the
# per-pair moments, ESS and AR orders come back.
# ---------------------------------------------------------------------------
def _omega_chain_stacks(hM, r, start, thin):
    """The chains' Lambda of level r (0-based) after start / thin, checked: (chains, n, nfmax)."""
    chains = [list(c[start - 1::thin]) for c in hM.postList]
    lens = [len(c) for c in chains]
    if len(set(lens)) != 1:
        raise ValueError(f"omegaDiagnostics: the chains have unequal lengths after start = {start}, thin = {thin} "
                         f"({lens}): gelman.diag and the device call need equal ones")
    n = lens[0]
    if n < 3:
        raise ValueError(f"omegaDiagnostics: {n} samples per chain after start = {start}, thin = {thin}: at least 3 "
                         "are needed (spectrum0.ar fits an AR model to the series)")
    nfm = max(int(np.asarray(s_["Lambda"][r]).shape[0]) for c in chains for s_ in c)
    return chains, n, nfm


def _omega_diag_device(lam, nf, device=None, scratch_bytes=0, series=False):
    """hmsc_omega_diagnostics on lam (m, n, ns, nfmax) -- C order, i.e. each sample nfmax x ns
    column-major -- and nf (m, n): per chain (ess, mean, var, order) as (m, ns, ns), and with
    series=True the series themselves (m, npairs, n), pair i <= j at i + j (j + 1) / 2, else None."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    nf = np.ascontiguousarray(nf, dtype=np.int32)
    m, n, ns, nfm = lam.shape
    ess, mean, var = (np.zeros((m, ns, ns)) for _ in range(3))
    order = np.zeros((m, ns, ns), dtype=np.int32)
    ser = np.zeros((m, ns * (ns + 1) // 2, n)) if series else None
    L.check(L.lib().hmsc_omega_diagnostics(_default_device_of(device), m, n, ns, nfm, L.iptr(nf), L.fptr(lam),
                                           int(scratch_bytes), L.fptr(ess), L.fptr(mean), L.fptr(var), L.iptr(order),
                                           L.fptr(ser)))
    return ess, mean, var, order, ser


def omegaDiagnostics(hM, r=1, start=1, thin=1, device=None, scratch_bytes=0):
    """coda::effectiveSize and gelman.diag(multivariate=FALSE) of convertToCodaObject(hM)$Omega[[r]]
    for every species pair, on the device (hmsc_omega_diagnostics): Omega_s = crossprod(Lambda_s)
    is formed there from the chains' Lambda and no ns^2 x samples matrix exists on the host.

    start and thin apply per chain (poolMcmcChains' rule).  Returns dict(ess (ns, ns) summed over
    the chains, psrf, psrf_upper (ns, ns; None with one chain), mean, var, order (m, ns, ns) per
    chain).  scratch_bytes bounds the device slab of series (0 = 1 GiB); no result depends on it."""
    ns = int(hM.ns)
    chains, n, nfm = _omega_chain_stacks(hM, r - 1, start, thin)
    m = len(chains)
    lam = np.zeros((m, n, ns, nfm))   # C order = each sample nfm x ns column-major (as _omega_device's)
    nf = np.zeros((m, n), dtype=np.int32)
    for c, chain in enumerate(chains):
        for k, s_ in enumerate(chain):
            l_ = np.asarray(s_["Lambda"][r - 1], dtype=np.float64)
            nf[c, k] = l_.shape[0]
            lam[c, k, :, :l_.shape[0]] = l_.T
    ess, mean, var, order, _ = _omega_diag_device(lam, nf, device, scratch_bytes)
    psrf = psrf_upper = None
    if m > 1:
        psrf, psrf_upper = gelman_from_moments(mean, var, n)
    total = ess[0].copy()               # summed in chain order, as effectiveSize sums
    for c in range(1, m):
        total = total + ess[c]
    return dict(ess=total, psrf=psrf, psrf_upper=psrf_upper, mean=mean, var=var, order=order)


def convergenceDiagnostics(hM, parameters=("Beta", "Gamma", "V", "Sigma", "Rho", "Omega"), start=1, thin=1,
                           device=None):
    """The convergence chunk of the vignettes as one call: per parameter dict(ess, psrf, psrf_upper)
    shaped like the parameter (Beta nc x ns, Gamma nc x nt, V nc x nc, Sigma ns, Rho 1; psrf None
    with one chain), for Omega a list of such dicts, one per random level (ns x ns).  The
    materialised blocks go through convertToCodaObject, effectiveSize and gelman_diag; Omega goes
    through omegaDiagnostics.  Rho is reported only for a model with phylogeny (hM.C)."""
    known = ("Beta", "Gamma", "V", "Sigma", "Rho", "Omega")
    bad = [p for p in parameters if p not in known]
    if bad:
        raise ValueError(f"convergenceDiagnostics: unknown parameters {bad}; known: {list(known)}")
    want = {p: p in parameters for p in known}
    coda, _ = convertToCodaObject(hM, start=start, Beta=want["Beta"], Gamma=want["Gamma"], V=want["V"],
                                  Sigma=want["Sigma"], Rho=want["Rho"], Eta=False, Lambda=False, Alpha=False,
                                  Omega=False, Psi=False, Delta=False)
    nc, ns = int(hM.nc), int(hM.ns)
    shapes = dict(Beta=(nc, ns), Gamma=(nc, -1), V=(nc, nc), Sigma=(ns,), Rho=(1,))
    out = {}
    for p in parameters:
        if p == "Omega":
            out[p] = []
            for r in range(hM.nr):
                o = omegaDiagnostics(hM, r=r + 1, start=start, thin=thin, device=device)
                out[p].append(dict(ess=o["ess"], psrf=o["psrf"], psrf_upper=o["psrf_upper"]))
            continue
        if p not in coda:               # Rho without hM.C
            continue
        chains = [c[::thin] for c in coda[p]]
        shape = lambda a: None if a is None else a.reshape(shapes[p], order="F")   # noqa: E731
        psrf, upper = gelman_diag(chains) if len(chains) > 1 else (None, None)
        out[p] = dict(ess=shape(effectiveSize(chains, device)), psrf=shape(psrf), psrf_upper=shape(upper))
    return out
