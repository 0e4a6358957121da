"""Post-sampling callers of the hot path, host side of the R wrapper.

predict (R/predict.R:1-231) keeps R's host logic -- argument checks, predictLatentFactor for
the prediction units (R/predictLatentFactor.R), the Pi of the new study design -- and hands
the per-sample loop (linear predictor, expected values or draws, Y back-scaling) to the HIP
kernel behind ``hmsc_predict`` (hmsc_amd/csrc/predict.hip).  computePredictedValues
(R/computePredictedValues.R:66-142) and evaluateModelFit (R/evaluateModelFit.R) sit on top.
There is no CPU fallback: without the HIP library predict raises HmscNativeError.
"""
import ctypes as C

import numpy as np
from scipy import stats

from . import _lib as L
from .model import _factor_levels
from .post import poolMcmcChains, stack_device_levels


def _levels(values):
    """levels(as.factor(x)) by the same rule hM$Pi was built with (model._as_factor_codes)."""
    return [str(v) for v in _factor_levels(values)]


def _coords(rL, names, units):
    """Rows of rL$s for the given unit names (R indexes rL$s by rownames)."""
    sn = rL["sNames"] if "sNames" in rL.names() else None
    s = np.asarray(rL.s, dtype=np.float64)
    if sn is None:            # unnamed coordinates: row k is the k-th level of the fitted units
        pos = {u: k for k, u in enumerate(units)}
        if any(n not in pos for n in names) or s.shape[0] != len(units):
            raise ValueError("predictLatentFactor: coordinates of new spatial units are needed: give sData "
                             "as a DataFrame whose index names every unit (rownames of rL$s)")
    else:
        pos = {str(u): k for k, u in enumerate(sn)}
    return s[[pos[str(n)] for n in names]]


def _dist_rows(rL, names, units):
    """Row / column indices of rL$distMat for the given unit names (R indexes it by
    rownames, R/predictLatentFactor.R:69-70,100)."""
    dn = rL["distNames"] if "distNames" in rL.names() else None
    if dn is None:            # unnamed: row k is the k-th level of the fitted units
        pos = {u: k for k, u in enumerate(units)}
        if any(n not in pos for n in names) or rL.distMat.shape[0] != len(units):
            raise ValueError("predictLatentFactor: distances to new spatial units are needed: give distMat "
                             "as a DataFrame whose index names every unit (rownames of rL$distMat)")
    else:
        pos = {str(u): k for k, u in enumerate(dn)}
        missing = [n for n in names if str(n) not in pos]
        if missing:
            raise ValueError(f"predictLatentFactor: units {missing[:5]} are not rows of rL$distMat")
    return np.array([pos[str(n)] for n in names], dtype=np.int64)


def _pdist(a, b):
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def predictLatentFactor(unitsPred, units, postEta, rL, predictMean=False, rng=None, postAlpha=None,
                        predictMeanField=False, device=None, seed=None, level=0, gppDevice=False):
    """R/predictLatentFactor.R:35-210 (host side of predict, as in R): known units keep their
    posterior Eta rows; new units of a non-spatial level get N(0, 1) draws (0 with
    predictMean); new units of a spatial level are kriged from the sample's Eta with its
    alphapw grid scale alpha_h (:59-204): predictMean / predictMeanField (:62-92), or the
    method's joint conditional -- Full (:95-117), NNGP over the nNeighbours nearest fitted
    units (:118-160), GPP through the knots (:161-203; R uses alpha[nf] for every factor
    there, and so does this restatement).

    device=None is the host path above, with its draws from ``rng``.  With a device index the
    new units of all samples go to the device in one ``hmsc_krige`` call (krige.hip): the unit
    bookkeeping stays here, the kernels are factored once per alphapw grid point in use, and
    every N(0, 1) draw -- a non-spatial level's included -- is the Philox normal of (new unit,
    factor, stream 31 + 256 * level, sample) under the key ``seed``; nothing is taken from ``rng``.
    GPP's joint conditional stays on the host (NotImplementedError with a device) unless
    gppDevice=True: then it is hmsc_krige's mode 4 (gpp.hip), with the knot innovation of (knot,
    factor, stream 32 + 256 * level, sample); a fitted unit on a knot is refused there, and a new
    unit on a knot gets no residual draw."""
    if predictMean and predictMeanField:
        raise ValueError("Hmsc.predictLatentFactor: predictMean and predictMeanField arguments cannot be simultaneously TRUE")
    if device is not None:
        return _predict_latent_factor_device(unitsPred, units, postEta, rL, predictMean, postAlpha, predictMeanField,
                                             int(device), seed, int(level), bool(gppDevice))
    units = [str(u) for u in units]
    unitsPred = [str(u) for u in unitsPred]
    pos = {u: k for k, u in enumerate(units)}
    old = np.array([u in pos for u in unitsPred], dtype=bool)
    new = ~old
    nn = int(new.sum())
    rng = rng or np.random.default_rng()
    spatial = bool(rL.sDim) and nn > 0
    if spatial:
        if postAlpha is None:
            raise ValueError("predictLatentFactor: postAlpha is needed for new units of a spatial level")
        newu = [u for u, o in zip(unitsPred, old) if not o]
        if rL.distMat is not None:
            # a level given by distances (R/predictLatentFactor.R:69-70,100): D from rL$distMat;
            # 'NNGP' and 'GPP' need coordinates in R too (rL$s, :120,163)
            if not (predictMean or predictMeanField) and rL.spatialMethod != "Full":
                raise ValueError(f"predictLatentFactor: spatialMethod '{rL.spatialMethod}' needs coordinates "
                                 f"(sData); a distMat level predicts with 'Full'")
            s1 = _dist_rows(rL, units, units)
            s2 = _dist_rows(rL, newu, units)
        else:
            s1 = _coords(rL, units, units)
            s2 = _coords(rL, newu, units)
        alphapw = np.asarray(rL.alphapw, dtype=np.float64)
    out = []
    for k, eta in enumerate(postEta):
        nf = eta.shape[1]
        e = np.empty((len(unitsPred), nf))
        if old.any():
            e[old] = eta[[pos[u] for u, o in zip(unitsPred, old) if o]]
        if nn and not spatial:
            e[new] = 0.0 if predictMean else rng.standard_normal((nn, nf))
        elif nn:
            e[new] = _krige(rL, eta, np.asarray(postAlpha[k]), alphapw, s1, s2, predictMean, predictMeanField, rng)
        out.append(e)
    return out


def _predict_latent_factor_device(unitsPred, units, postEta, rL, predictMean, postAlpha, predictMeanField, device,
                                  seed, level, gppDevice=False):
    """predictLatentFactor with the new units' rows from hmsc_krige (include/hmsc_amd.h)."""
    units = [str(u) for u in units]
    unitsPred = [str(u) for u in unitsPred]
    pos = {u: k for k, u in enumerate(units)}
    old = np.array([u in pos for u in unitsPred], dtype=bool)
    new = ~old
    nn, S = int(new.sum()), len(postEta)
    oldrows = [pos[u] for u, o in zip(unitsPred, old) if o]
    res = None
    if nn and S and not (predictMean and not rL.sDim):
        if seed is None and not predictMean:
            raise ValueError("predictLatentFactor: device kriging draws from a Philox key: give seed")
        npo = len(units)
        nfs = [int(np.asarray(e).shape[1]) for e in postEta]
        nfmax = max(nfs)
        a = L.hmsc_krige_args()
        keep = []
        if rL.sDim:
            if postAlpha is None:
                raise ValueError("predictLatentFactor: postAlpha is needed for new units of a spatial level")
            newu = [u for u, o in zip(unitsPred, old) if not o]
            d = krige_description(rL, units, newu, predictMean, predictMeanField, gppDevice, nfs, lambda k: postAlpha[k])
            mode, alphas, idx, a.sDim = d["mode"], d["alphas"], d["alpha"], d["sDim"]
            if d["dist"] is not None:
                a.dist = L.colmajor_ptr(d["dist"], keep)
            else:
                a.coords = L.colmajor_ptr(d["coords"], keep)
            if mode == 4:
                a.knots, a.nK = L.colmajor_ptr(d["knots"], keep), int(d["knots"].shape[0])
            a.nNeighbours = int(rL.nNeighbours) if rL.nNeighbours is not None else 10
        else:
            # a non-spatial level's new units are N(0, 1): the same call on a one-point grid at
            # alpha = 0, whose output is z of the counter contract
            mode, alphas = 2, np.zeros(1)
            a.coords = L.colmajor_ptr(np.zeros((npo + nn, 1)), keep)
            a.sDim = 1
            idx = np.zeros((S, nfmax), dtype=np.int32)
            for k in range(S):
                idx[k, :nfs[k]] = 1
        eta = np.zeros((S, nfmax, npo))
        for k, e in enumerate(postEta):
            eta[k, :nfs[k]] = np.asarray(e, dtype=np.float64).T
        keep += [alphas, idx, eta]
        a.device, a.np, a.nn, a.G, a.S, a.nfmax, a.mode, a.level = device, npo, nn, len(alphas), S, nfmax, mode, level
        a.seed = int(seed or 0)
        a.alphas, a.Eta, a.alpha = L.fptr(alphas), L.fptr(eta), L.iptr(idx)
        res = np.empty((S, nfmax, nn))
        L.check(L.lib().hmsc_krige(C.byref(a), L.fptr(res)))
    out = []
    for k, eta_k in enumerate(postEta):
        nf = eta_k.shape[1]
        e = np.empty((len(unitsPred), nf))
        if old.any():
            e[old] = eta_k[oldrows]
        if nn:
            e[new] = 0.0 if res is None else res[k, :nf].T
        out.append(e)
    return out


def gpp_knots(rL, sDim):
    """rL$sKnot (nK x sDim) of a GPP level."""
    sK = np.asarray(rL["sKnot"], dtype=np.float64) if "sKnot" in rL.names() else None
    if sK is None or sK.ndim != 2 or sK.shape[0] == 0 or sK.shape[1] != sDim:
        raise ValueError("predictLatentFactor: a GPP level needs knots (sKnot) of the coordinates' dimension")
    return sK


def krige_description(rL, units, newu, predictMean, predictMeanField, gppDevice, nfs, alpha):
    """What hmsc_krige and hmsc_predict_map take of a spatial level with the new units newu: dict(mode,
    coords or dist with sDim (fitted units, then new), knots (mode 4), alphas, alpha: the S x max(nfs)
    table of 1-based grid indices, alpha(k) being sample k's, 0 for a factor the sample lacks)."""
    method = rL.spatialMethod
    if predictMean or predictMeanField:
        mode = 0 if predictMean else 1
    elif method == "Full":
        mode = 2
    elif method == "NNGP":
        mode = 3
    elif method == "GPP" and gppDevice:
        mode = 4
    elif method == "GPP":
        raise NotImplementedError("predictLatentFactor: GPP kriging on the device is not implemented (its cost "
                                  "is in the knots, not in np): predict this level with device=None")
    else:
        raise ValueError(f"unknown spatialMethod {method!r}")
    d = dict(mode=mode, coords=None, dist=None, sDim=0, knots=None)
    if rL.distMat is not None:
        if mode in (3, 4):
            raise ValueError(f"predictLatentFactor: spatialMethod '{method}' needs coordinates "
                             f"(sData); a distMat level predicts with 'Full'")
        ua = np.concatenate([_dist_rows(rL, units, units), _dist_rows(rL, newu, units)])
        d["dist"] = np.asarray(rL.distMat, dtype=np.float64)[np.ix_(ua, ua)]
    else:
        d["coords"] = np.vstack([_coords(rL, units, units), _coords(rL, newu, units)])
        d["sDim"] = d["coords"].shape[1]
    if mode == 4:
        d["knots"] = gpp_knots(rL, d["sDim"])
    d["alphas"] = np.ascontiguousarray(np.asarray(rL.alphapw, dtype=np.float64)[:, 0])
    d["alpha"] = np.zeros((len(nfs), max(nfs)), dtype=np.int32)
    for k, nf in enumerate(nfs):
        d["alpha"][k, :nf] = np.asarray(alpha(k), dtype=np.int64).ravel()[:nf]
    return d


def _krige(rL, eta, alpha, alphapw, s1, s2, predictMean, predictMeanField, rng):
    npo, nf, nn = s1.shape[0], eta.shape[1], s2.shape[0]
    res = np.empty((nn, nf))
    dm = rL.distMat
    if predictMean or predictMeanField:                                       # :62-92
        # (with distMat R's :69-70 index rL$distMat by s1 / s2, which that branch never sets --
        # an error in R; the fitted and new units' rows are what it evidently means)
        if dm is not None:
            D11, D12 = dm[np.ix_(s1, s1)], dm[np.ix_(s1, s2)]
        else:
            D11, D12 = _pdist(s1, s1), _pdist(s1, s2)
        for h in range(nf):
            a = alphapw[alpha[h] - 1, 0]
            if a > 0:
                K11, K12 = np.exp(-D11 / a), np.exp(-D12 / a)
                m = K12.T @ np.linalg.solve(K11, eta[:, h])
                if predictMean:
                    res[:, h] = m
                else:
                    iLK = np.linalg.solve(np.linalg.cholesky(K11), K12)
                    res[:, h] = m + rng.standard_normal(nn) * np.sqrt(1 - (iLK ** 2).sum(axis=0))
            else:
                res[:, h] = 0.0 if predictMean else rng.standard_normal(nn)
        return res
    method = rL.spatialMethod
    if method == "Full":                                                      # :95-117
        if dm is not None:
            ua = np.concatenate([s1, s2])
            D = dm[np.ix_(ua, ua)]
        else:
            D = _pdist(np.vstack([s1, s2]), np.vstack([s1, s2]))
        for h in range(nf):
            a = alphapw[alpha[h] - 1, 0]
            if a > 0:
                K = np.exp(-D / a)
                K11, K12, K22 = K[:npo, :npo], K[:npo, npo:], K[npo:, npo:]
                m = K12.T @ np.linalg.solve(K11, eta[:, h])
                W = K22 - K12.T @ np.linalg.solve(K11, K12)
                res[:, h] = m + np.linalg.cholesky(W) @ rng.standard_normal(nn)
            else:
                res[:, h] = rng.standard_normal(nn)
    elif method == "NNGP":                                                    # :118-160
        k = int(rL.nNeighbours) if rL.nNeighbours is not None else 10
        d = _pdist(s2, s1)
        ind = np.argsort(d, axis=1, kind="stable")[:, :k]                     # FNN::knnx.index
        for h in range(nf):
            a = alphapw[alpha[h] - 1, 0]
            if a > 0:
                m = np.empty(nn)
                F = np.empty(nn)
                for i in range(nn):
                    K11 = np.exp(-_pdist(s1[ind[i]], s1[ind[i]]) / a)
                    K12 = np.exp(-d[i, ind[i]] / a)
                    w = np.linalg.solve(K11, K12)
                    m[i] = w @ eta[ind[i], h]
                    F[i] = 1 - w @ K12
                res[:, h] = m + np.sqrt(F) * rng.standard_normal(nn)
            else:
                res[:, h] = rng.standard_normal(nn)
    elif method == "GPP":                                                     # :161-203
        sK = np.asarray(rL["sKnot"], dtype=np.float64)
        dss, dns, dnsOld = _pdist(sK, sK), _pdist(s2, sK), _pdist(s1, sK)
        for h in range(nf):
            a = alphapw[alpha[nf - 1] - 1, 0]                                  # R: ag = alpha[nf]
            if a > 0:
                Wns, W12, Wss = np.exp(-dns / a), np.exp(-dnsOld / a), np.exp(-dss / a)
                iWss = np.linalg.inv(Wss)
                dDn = 1 - ((Wns @ iWss) * Wns).sum(axis=1)
                idD = 1 / (1 - np.einsum("ik,kl,il->i", W12, iWss, W12))
                idDW12 = idD[:, None] * W12
                iF = np.linalg.inv(Wss + W12.T @ idDW12)
                LiF = np.linalg.cholesky(iF).T                                 # chol(): upper
                mu = iF @ idDW12.T @ eta[:, h] + LiF @ rng.standard_normal(sK.shape[0])
                res[:, h] = Wns @ mu + np.sqrt(dDn) * rng.standard_normal(nn)
            else:
                res[:, h] = rng.standard_normal(nn)
    else:
        raise ValueError(f"unknown spatialMethod {method!r}")
    return res


def predict(hM, post=None, X=None, studyDesign=None, Yc=None, mcmcStep=1, expected=False, predictEtaMean=False,
            seed=None, device=0, predictEtaMeanField=False, XRRRData=None, XRRR=None, krigeDevice=False,
            condBatch=False, XData=None, ranLevels=None, Gradient=None, gppDevice=False, condSpatial=False):
    """predict.Hmsc (R/predict.R): a list of ny x ns arrays, one per posterior sample.  With Yc
    (conditional prediction, :191-202) each sample's latent factors are first updated given the
    observed part of Yc by updateZ / (updateEta, updateZ) x mcmcStep on the device.
    A reduced-rank regression model appends XRRR %*% t(sam$wRRR) to X per sample (:91-97,144-152);
    the kernel takes one X for all samples, so it is given [X, XRRR] and each sample's
    rbind(BetaNRRR, t(wRRR) %*% BetaRRR): the same LFix = cbind(X, XB) %*% Beta.
    krigeDevice=True: predictLatentFactor's new units come from the device (hmsc_krige) under the
    key `seed`, or one key drawn from the seeded generator; the default keeps them on the host.
    gppDevice=True (with krigeDevice=True; no effect without it): a GPP level's joint conditional is
    kriged on the device too (hmsc_krige mode 4) instead of being refused.
    condBatch=True (experimental): Yc conditions all samples in one device call
    (hmsc_predict_conditional, samples as a grid axis) instead of sample by sample; same key, same
    starting Eta and same draws for a given seed, results equal to rounding.  It serves non-spatial
    levels without xData and nf <= 32 (NotImplementedError otherwise), and reduced-rank regression
    models, which the per-sample path refuses.
    condSpatial=True (with condBatch=True; no effect without it): the batched call also serves
    spatial 'Full' levels, given by sData or distMat, grouped units allowed, and 'GPP' levels with
    one row per unit (hmsc_predict_conditional_spatial): each sample's system is factored once
    instead of 1 + mcmcStep times, and only the alphapw values the posterior uses are built.
    'NNGP' levels are refused by name.
    XData (a data frame of the fitted model's covariates, :76-86: its model matrix with the fitted
    factor levels), ranLevels (the prediction units' levels by name, :119-127: the coordinates of
    new spatial units come from them) and Gradient (constructGradient's or prepareGradient's dict,
    which sets XData, studyDesign and ranLevels, :62-66) are R's arguments of those names."""
    a, keep, S, nyN = _predict_args(hM, post, X, studyDesign, Yc, mcmcStep, expected, predictEtaMean, seed, device,
                                    predictEtaMeanField, XRRRData, XRRR, krigeDevice, condBatch, XData, ranLevels,
                                    Gradient, gppDevice, condSpatial)
    out = np.empty(S * nyN * hM.ns)
    L.check(L.lib().hmsc_predict(C.byref(a), L.fptr(out)))
    del keep
    out = out.reshape(S, hM.ns, nyN).transpose(0, 2, 1)
    return [out[k] for k in range(S)]


def _xlev(XData):
    """The factor columns' levels of a fitted data frame (R/predict.R:83: lapply(XData, levels) of
    the factors), as model_matrix's xlev."""
    import pandas as pd
    df = pd.DataFrame(XData)
    return {c: _levels(df[c]) for c in df.columns
            if not pd.api.types.is_numeric_dtype(df[c]) or pd.api.types.is_bool_dtype(df[c])}


def _new_design(hM, X, studyDesign, XData, ranLevels, Gradient):
    """R/predict.R:62-90,116-127: Gradient sets XData, studyDesign and ranLevels; XData becomes the
    model matrix under the fitted formula and factor levels; ranLevels replaces the model's levels
    (a copy of hM carries them, so every later step reads the prediction units' levels)."""
    if Gradient is not None:
        XData, studyDesign, ranLevels = Gradient["XDataNew"], Gradient["studyDesignNew"], Gradient["rLNew"]
    if XData is not None and X is not None:
        raise ValueError("Hmsc.predict: only one of XData and X arguments can be specified")
    if XData is not None:
        if isinstance(XData, list):
            raise NotImplementedError("predict: species-specific XData lists are out of scope")
        if hM.XData is None:
            raise ValueError("Hmsc.predict: XData needs a model that was defined with XData and XFormula")
        from .model import model_matrix
        X = model_matrix(hM.XFormula, XData, xlev=_xlev(hM.XData))[0]
    if hM.nr and studyDesign is not None and not all(n in studyDesign for n in hM.rLNames):
        raise ValueError("hMsc.predict: dfPiNew does not contain all the necessary named columns")
    if ranLevels is not None:
        if not all(n in ranLevels for n in hM.rLNames):
            raise ValueError("hMsc.predict: rL does not contain all the necessary named levels")
        hM = hM.copy()
        hM.rL = [ranLevels[n] for n in hM.rLNames]
    return hM, X, studyDesign


def _predict_args(hM, post, X, studyDesign, Yc, mcmcStep, expected, predictEtaMean, seed, device,
                  predictEtaMeanField, XRRRData, XRRR, krigeDevice, condBatch, XData=None, ranLevels=None,
                  Gradient=None, gppDevice=False, condSpatial=False):
    """predict's host part up to the device call: the checks, predictLatentFactor for the prediction
    units, the conditioning on Yc and the sample-major stacks, as hmsc_predict_args.  Returns (args,
    the arrays the pointers refer to, the number of samples, the number of prediction rows); predict
    predictSummary and predictCommunity hand the same block to hmsc_predict, hmsc_predict_summary
    and hmsc_predict_community."""
    hM, X, studyDesign = _new_design(hM, X, studyDesign, XData, ranLevels, Gradient)
    post = poolMcmcChains(hM.postList) if post is None else post
    X = np.asarray(hM.X if X is None else X, dtype=np.float64)
    nyN = X.shape[0]
    if XRRRData is not None and XRRR is not None:
        raise ValueError("Hmsc.predict: only one of XRRRData and XRRR arguments can be specified")
    ncRRR = int(hM.ncRRR or 0)
    if XRRRData is not None:                                                  # :91-93
        from .model import model_matrix
        XRRR = model_matrix(hM.XRRRFormula, XRRRData)[0]
    elif XRRR is None and ncRRR > 0:                                          # :96-97
        XRRR = hM["XRRR"]
    betas = [np.asarray(s["Beta"], dtype=np.float64) for s in post]
    if ncRRR > 0:
        XRRR = np.asarray(XRRR, dtype=np.float64)
        if XRRR.shape[0] != nyN:
            raise ValueError("hMsc.predict: number of rows in XRRR and X must be equal")
        if Yc is not None and not condBatch and np.any(~np.isnan(np.asarray(Yc, dtype=np.float64))):
            raise NotImplementedError("predict: conditional prediction (Yc) is not implemented for a reduced-rank "
                                      "regression model")
        ncN = hM.ncNRRR
        betas = [np.vstack([b[:ncN], np.asarray(s["wRRR"]).T @ b[ncN:]]) for b, s in zip(betas, post)]
        X = np.hstack([X, XRRR])
    studyDesign = hM.studyDesign if studyDesign is None else studyDesign
    if Yc is not None:
        Yc = np.asarray(Yc, dtype=np.float64)
        if Yc.shape[1] != hM.ns:
            raise ValueError("hMsc.predict: number of columns in Yc must be equal to ns")
        if Yc.shape[0] != nyN:
            raise ValueError("hMsc.predict: number of rows in Yc and X must be equal")
        if condBatch and np.any(~np.isnan(Yc)):
            cond_batch_check(hM, post, spatial=bool(condSpatial))
    rng = np.random.default_rng(seed)
    S = len(post)
    keep = []
    a = L.hmsc_predict_args()
    a.ny, a.ns, a.nc, a.nr, a.nsamples = nyN, hM.ns, X.shape[1], hM.nr, S
    a.expected = 1 if expected else 0
    a.seed = int(rng.integers(1, 2 ** 62)) if seed is None else int(seed)
    a.device = device
    kkey = None
    if krigeDevice:
        kkey = int(rng.integers(1, 2 ** 62)) if seed is None else int(seed)
    kdev = dict(device=device, seed=kkey, gppDevice=bool(gppDevice)) if krigeDevice else {}
    a.X = L.colmajor_ptr(X, keep)
    a.Beta = L.fptr(_stack(keep, [b.reshape(-1, order="F") for b in betas]))
    a.sigma = L.fptr(_stack(keep, [np.asarray(s["sigma"], dtype=np.float64) for s in post]))
    a.family = L.colmajor_ptr(hM.distr[:, 0], keep, np.int32)
    a.YScalePar = L.colmajor_ptr(hM.YScalePar, keep)
    if hM.nr:
        # a covariate-dependent level goes to the kernel as one level per column of rL$x with
        # Eta[q, ] * x[q, k] of the prediction units (R/predict.R:171-176: LRan = sum_k
        # (Eta[dfPiNew,] * x[dfPiNew, k]) %*% Lambda[,,k])
        ndev = sum(max(int(rl.xDim or 0), 1) for rl in hM.rL)
        if ndev > L.MAX_LEVELS:
            raise ValueError(f"predict: at most {L.MAX_LEVELS} device levels")
        PiNew = np.zeros((nyN, ndev), dtype=np.int32)
        nps, nfs = [], []
        d = 0
        for r, name in enumerate(hM.rLNames):
            raw = studyDesign[name]
            col = np.asarray(raw).astype(str)
            unitsPred = _levels(raw)
            units = _levels(hM.dfPi[name])
            etas = predictLatentFactor(unitsPred, units, [s["Eta"][r] for s in post], hM.rL[r],
                                       predictMean=predictEtaMean, rng=rng,
                                       postAlpha=[s["Alpha"][r] for s in post] if hM.rL[r].sDim else None,
                                       predictMeanField=predictEtaMeanField, level=r, **kdev)
            if Yc is not None and np.any(~np.isnan(Yc)):
                if r == 0 and condBatch:
                    cond = _conditional_etas_batched(hM, post, X, betas, studyDesign, Yc, mcmcStep, rng, device,
                                                     krigeKey=kkey, spatial=bool(condSpatial))
                elif r == 0:
                    cond = _conditional_etas(hM, post, X, studyDesign, Yc, mcmcStep, rng, device, krigeKey=kkey)
                etas = [c[r] for c in cond]
            idx = {u: k for k, u in enumerate(unitsPred)}
            xp = _x_rows(hM, r, unitsPred) if int(hM.rL[r].xDim or 0) else None
            nf, stacks = stack_device_levels(keep, etas, [s["Lambda"][r] for s in post], xp)
            for eta_k, lam_k in stacks:
                PiNew[:, d] = [idx[v] + 1 for v in col]
                a.Eta[d] = L.fptr(eta_k)
                a.Lambda[d] = L.fptr(lam_k)
                nps.append(len(unitsPred))
                nfs.append(nf)
                d += 1
        a.nr = ndev
        a.Pi = L.colmajor_ptr(PiNew, keep, np.int32)
        a.np = L.colmajor_ptr(nps, keep, np.int32)
        a.nf = L.colmajor_ptr(nfs, keep, np.int32)
    return a, keep, S, nyN


SUMMARY_MAX_PROBS = 8


def _summary_probs(hM, probs):
    """The probabilities and flagged columns of a summary call: the caller's probs on every column,
    with 0.5 added when the model has Poisson columns (evaluateModelFit's median); without probs,
    0.5 on the Poisson columns alone.  Raises ValueError for more than 8 probabilities or one
    outside [0, 1]; touches no device library."""
    probs = [float(p) for p in np.asarray(probs, dtype=np.float64).reshape(-1)]
    if any(not (0.0 <= p <= 1.0) for p in probs):
        raise ValueError("predictSummary: every probability in probs must lie in [0, 1]")
    pois = np.asarray(hM.distr)[:, 0] == 3
    qcols = np.ones(hM.ns, dtype=np.int32) if probs else pois.astype(np.int32)
    if pois.any() and 0.5 not in probs:
        probs = probs + [0.5]
    if len(probs) > SUMMARY_MAX_PROBS:
        raise ValueError(f"predictSummary: at most {SUMMARY_MAX_PROBS} probabilities in one call (0.5 is added for "
                         f"Poisson columns); got {len(probs)}")
    return probs, qcols


def predictSummary(hM, post=None, X=None, studyDesign=None, Yc=None, mcmcStep=1, expected=False, predictEtaMean=False,
                   seed=None, device=0, predictEtaMeanField=False, XRRRData=None, XRRR=None, krigeDevice=False,
                   condBatch=False, probs=(), scratch_bytes=0, XData=None, ranLevels=None, Gradient=None,
                   gppDevice=False, condSpatial=False):
    """Per-cell summaries of predict's samples without the samples (hmsc_predict_summary): the
    arguments of predict, and for one seed the summaries of the very values predict returns.
    Returns a dict: mean, occ (share of values > 0) and n (values that are not NaN), each ny x ns;
    probs; quantiles (len(probs) x ny x ns, R's type 7); median (ny x ns, NaN where 0.5 was not
    computed).  Without probs, 0.5 is computed for the Poisson columns only; with probs every column
    gets them, and 0.5 is added if the model has Poisson columns.  scratch_bytes bounds the device
    slab of the quantile selection (0: 1 GiB); the results do not depend on it.  XData, ranLevels,
    gppDevice, condSpatial and Gradient are predict's."""
    probs, qcols = _summary_probs(hM, probs)
    a, keep, S, nyN = _predict_args(hM, post, X, studyDesign, Yc, mcmcStep, expected, predictEtaMean, seed, device,
                                    predictEtaMeanField, XRRRData, XRRR, krigeDevice, condBatch, XData, ranLevels,
                                    Gradient, gppDevice, condSpatial)
    ns, nq = hM.ns, len(probs)
    q = L.hmsc_summary_args()
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    q.nq, q.scratch_bytes = nq, int(scratch_bytes)
    q.probs, q.qcols = (L.fptr(pr), L.iptr(qcols)) if nq else (None, None)
    mean, occ = np.empty(ns * nyN), np.empty(ns * nyN)
    n = np.empty(ns * nyN, dtype=np.int32)
    quant = np.empty(max(nq, 1) * ns * nyN)
    L.check(L.lib().hmsc_predict_summary(C.byref(a), C.byref(q), L.fptr(mean), L.fptr(occ), L.iptr(n),
                                         L.fptr(quant) if nq else None))
    del keep
    return _unpack_cells(mean, occ, n, quant, probs, ns, nyN)


def _unpack_cells(mean, occ, n, quant, probs, ns, nyN):
    """predictSummary's dict from a filled cell block (column-major ny x ns planes)."""
    nq = len(probs)
    quant = quant.reshape(max(nq, 1), ns, nyN).transpose(0, 2, 1)[:nq]
    median = quant[probs.index(0.5)].copy() if 0.5 in probs else np.full((nyN, ns), np.nan)
    return dict(mean=mean.reshape(ns, nyN).T, occ=occ.reshape(ns, nyN).T, n=n.reshape(ns, nyN).T,
                probs=np.array(probs), quantiles=quant, median=median)


def _x_rows(hM, r, units):
    """rL$x rows of the given unit names (R indexes rL$x by unit name, R/predict.R:174); unnamed
    rows are the fitted units in order."""
    rl = hM.rL[r]
    x = np.asarray(rl.x, dtype=np.float64)
    names = [str(i) for i in rl.x.index] if hasattr(rl.x, "index") else None
    if names is None:
        fitted = _levels(hM.dfPi[hM.rLNames[r]])
        pos = {u: k for k, u in enumerate(fitted)}
        if any(u not in pos for u in units) or x.shape[0] != len(fitted):
            raise ValueError(f"predict: covariates of new units of level {hM.rLNames[r]} are needed: give xData "
                             f"as a DataFrame whose index names every unit")
    else:
        pos = {n: k for k, n in enumerate(names)}
        missing = [u for u in units if str(u) not in pos]
        if missing:
            raise ValueError(f"predict: no xData rows for units {missing[:5]} of level {hM.rLNames[r]}")
    return x[[pos[str(u)] for u in units]]


def _conditional_etas(hM, post, X, studyDesign, Yc, mcmcStep, rng, device, krigeKey=None):
    """R/predict.R:191-202: per sample, Z = L; Z = updateZ(Yc); then mcmcStep x (updateEta,
    updateZ), all with the sample's Beta, sigma, Lambda fixed -- the device updaters of a chain
    built on (Yc, X) in R's unscaled space (X and Beta as `post` holds them)."""
    from .model import Hmsc
    from .sampler import Chain, level_lran
    rl = {name: hM.rL[r] for r, name in enumerate(hM.rLNames)}
    sd = studyDesign.reset_index(drop=True) if hasattr(studyDesign, "reset_index") else studyDesign
    hMc = Hmsc(Y=Yc, X=X, XScale=False, YScale=False, distr=hM.distr, studyDesign=sd, ranLevels=rl,
               covNames=list(hM.covNames), spNames=list(hM.spNames))
    ch = Chain(hMc, int(rng.integers(1, 2 ** 62)), device=device, updater={"GammaEta": False})
    out = []
    try:
        ch.init()
        units = [_levels(hM.dfPi[name]) for name in hM.rLNames]
        dev_etas = None
        if krigeKey is not None:   # all samples of a level in one device call (sample = Philox counter)
            dev_etas = [predictLatentFactor(_levels(sd[name]), units[r], [sam["Eta"][r] for sam in post], hM.rL[r],
                                            postAlpha=[sam["Alpha"][r] for sam in post] if hM.rL[r].sDim else None,
                                            device=device, seed=krigeKey, level=r)
                        for r, name in enumerate(hM.rLNames)]
        for k, sam in enumerate(post):
            if dev_etas is not None:
                etas = [de[k] for de in dev_etas]
            else:
                etas = []
                for r, name in enumerate(hM.rLNames):
                    etas.append(predictLatentFactor(_levels(sd[name]), units[r], [sam["Eta"][r]], hM.rL[r], rng=rng,
                                                    postAlpha=[sam["Alpha"][r]] if hM.rL[r].sDim else None)[0])
            L = X @ sam["Beta"]
            for r in range(hM.nr):
                xr = _x_rows(hM, r, _levels(sd[hM.rLNames[r]])) if hM.rL[r].xDim else None
                L = L + level_lran(etas[r], sam["Lambda"][r], hMc.Pi[:, r] - 1, xr)
            # the sample's spatial scales condition the spatial levels' updateEta prior
            # (R/predict.R:185 passes Alpha = sam$Alpha)
            ch.set_state(dict(Beta=sam["Beta"], sigma=np.asarray(sam["sigma"]), Eta=etas,
                              Lambda=[np.asarray(lm) for lm in sam["Lambda"]], Z=L,
                              Alpha=[np.asarray(a, dtype=np.int64).ravel() for a in sam["Alpha"]]))
            it = 1 + k * (2 * mcmcStep + 1)
            ch.update("Z", it)
            for m in range(mcmcStep):
                ch.update("Eta", it + 1 + 2 * m)
                ch.update("Z", it + 2 + 2 * m)
            out.append(ch.get_state(with_z=False)["Eta"])
    finally:
        ch.close()
    return out


def cond_batch_check(hM, post, spatial=False):
    """What the batched conditional path (hmsc_predict_conditional) serves: non-spatial levels
    without unit covariates and at most 32 factors; with spatial=True (condSpatial,
    hmsc_predict_conditional_spatial) spatial 'Full' levels and 'GPP' levels with one row per unit,
    at most 16 factors and nK nf <= 1024 as well.  Raises NotImplementedError naming the level and
    the reason; touches no device library."""
    for r, name in enumerate(hM.rLNames):
        rl = hM.rL[r]
        if rl.sDim and spatial:
            nf = max(int(np.asarray(s["Eta"][r]).shape[1]) for s in post) if len(post) else 0
            if rl.spatialMethod == "NNGP":
                raise NotImplementedError(f"predict: condSpatial does not serve level {name}: spatial method 'NNGP' "
                                          f"(its factor lives in the chain's band order); use condBatch=False")
            if rl.spatialMethod == "GPP":
                _cond_gpp_check(name, int(hM.np[r]), int(hM.ny), nf, np.asarray(rl["sKnot"]).shape[0])
        elif rl.sDim:
            raise NotImplementedError(f"predict: condBatch does not serve level {name}: spatial (its updateEta prior "
                                      f"couples the units); use condBatch=False")
        if int(rl.xDim or 0):
            raise NotImplementedError(f"predict: condBatch does not serve level {name}: xData (covariate-dependent "
                                      f"loadings); use condBatch=False")
        nf = max(int(np.asarray(s["Eta"][r]).shape[1]) for s in post) if len(post) else 0
        if nf > 32:
            raise NotImplementedError(f"predict: condBatch does not serve level {name}: nf > 32 (nf = {nf}); use "
                                      f"condBatch=False")


def _cond_gpp_check(name, npr, ny, nf, nK):
    """The batched call's limits for a 'GPP' level (those of the chain's GPP updater)."""
    if npr != ny:
        raise NotImplementedError(f"predict: condSpatial does not serve level {name}: 'GPP' with grouped units (np = "
                                  f"{npr}, ny = {ny}; the low-rank form takes one row per unit); use condBatch=False")
    if nf > 16:
        raise NotImplementedError(f"predict: condSpatial does not serve level {name}: 'GPP' with nf > 16 (nf = {nf}); "
                                  f"use condBatch=False")
    if nK * nf > 1024:
        raise NotImplementedError(f"predict: condSpatial does not serve level {name}: 'GPP' with nK * nf > 1024 (nK = "
                                  f"{nK}, nf = {nf}); use condBatch=False")


def cond_grid_in_use(alphapw, alphas, nf=None, name="?"):
    """The part of a level's alphapw grid a posterior uses.  alphapw: the level's grid (G x 2, the
    values in column 0); alphas: per sample the 1-based grid index of every factor (sam$Alpha[[r]]);
    nf: the width of the index table (default: the most factors of a sample).  Returns (values: the
    grid values of the distinct indices in use, in the grid's order; idx: nsamples x nf int32, the
    0-based position in `values` of every factor's value).  A sample with fewer than nf factors is
    padded with 0, the first value in use, as stack_device_levels pads its Eta and Lambda with
    zeros.  Raises ValueError for an index outside the grid."""
    grid = np.asarray(alphapw, dtype=np.float64).reshape(-1, 2)[:, 0]
    al = [np.asarray(a, dtype=np.int64).reshape(-1) for a in alphas]
    nf = max([a.size for a in al] + [0]) if nf is None else int(nf)
    flat = np.concatenate(al) if al else np.zeros(0, dtype=np.int64)
    if flat.size and (flat.min() < 1 or flat.max() > grid.size):
        raise ValueError(f"predict: a grid index of level {name} lies outside its alphapw (1 .. {grid.size})")
    used = np.unique(flat)
    idx = np.zeros((len(al), nf), dtype=np.int32)
    for k, a in enumerate(al):
        idx[k, :a.size] = np.searchsorted(used, a)
    return grid[used - 1], idx


def cond_classes(obs, pi0, npr):
    """The distinct count vectors of a level: obs (ny x ns, True where Yc is observed), pi0 the
    0-based unit of every row.  c[q, j] counts the rows of unit q in which species j is observed;
    returns (cnt: ncls x ns int32, the distinct rows of c in np.unique's order; unit_class: npr
    int32 with c[q] == cnt[unit_class[q]])."""
    obs = np.asarray(obs, dtype=bool)
    pi0 = np.asarray(pi0, dtype=np.int64)
    ny, ns = obs.shape
    rows = np.bincount(pi0, minlength=npr)
    so = obs[np.argsort(pi0, kind="stable")].astype(np.int32)      # rows grouped by unit
    if np.all(rows == 1):
        c = so
    else:                                                          # differences of the running sums
        cs = np.vstack([np.zeros((1, ns), dtype=np.int32), np.cumsum(so, axis=0, dtype=np.int32)])
        ends = np.cumsum(rows)
        c = cs[ends] - cs[ends - rows]
    # np.unique over whole rows sorts npr keys of ns words; a 64-bit hash per row finds the
    # candidates first, each row is then compared with its class' representative (exact), and only
    # the representatives are sorted (np.unique's order).  A hash collision takes the plain way.
    w = np.random.default_rng(0x636F6E64).integers(1, 2 ** 63, ns, dtype=np.uint64)
    h = c.astype(np.uint64) @ w                                    # (wraps: mod 2^64)
    _, first, hinv = np.unique(h, return_index=True, return_inverse=True)
    hinv = np.reshape(hinv, -1)
    reps = c[first]
    if np.array_equal(reps[hinv], c):
        cnt, rinv = np.unique(reps, axis=0, return_inverse=True)
        inv = np.reshape(rinv, -1)[hinv]
    else:
        cnt, inv = np.unique(c, axis=0, return_inverse=True)
    return np.ascontiguousarray(cnt, dtype=np.int32), np.ascontiguousarray(np.reshape(inv, -1), dtype=np.int32)


def conditional_etas_device(X, betas, sigmas, etas, lams, Pi, family, Yc, mcmcStep, seed, device=0, sample_chunk=0,
                            spatial=None):
    """One hmsc_predict_conditional call (include/hmsc_amd.h) on all samples: betas[k] (nc x ns),
    sigmas[k] (ns), etas[k][r] (np_r x nf_k, the starting Eta of the prediction units), lams[k][r]
    (nf_k x ns), Pi (ny x nr, 1-based), family (ns).  Sample k draws under the key `seed` at the
    iterations 1 + k (2 mcmcStep + 1) ...: what _conditional_etas draws sample by sample.  Returns
    the conditioned Eta as [sample][level].
    spatial (hmsc_predict_conditional_spatial): None, or per level None or a dict: alphapw (the
    level's grid), Alpha (per sample the factors' 1-based grid indices), and for a 'Full' level
    coords (np_r x sDim) or dist (np_r x np_r) of the level's units in Eta's order, for a 'GPP' level
    gpp: a function of the grid values in use that returns their (idDg, idDW12g, Fg), each with
    the grid value as its last axis (hmsc_amd/dataparams.py)."""
    X = np.asarray(X, dtype=np.float64)
    Yc = np.asarray(Yc, dtype=np.float64)
    Pi = np.asarray(Pi, dtype=np.int32).reshape(X.shape[0], -1)
    S, nr = len(betas), Pi.shape[1]
    if S == 0:
        return []
    if nr > L.MAX_LEVELS:
        raise ValueError(f"predict: at most {L.MAX_LEVELS} device levels")
    keep = []
    a = L.hmsc_cond_args()
    a.ny, a.ns, a.nc, a.nr, a.nsamples = X.shape[0], Yc.shape[1], X.shape[1], nr, S
    a.mcmcStep, a.device, a.sample_chunk, a.seed = int(mcmcStep), int(device), int(sample_chunk), int(seed)
    a.X = L.colmajor_ptr(X, keep)
    a.Yc = L.colmajor_ptr(Yc, keep)
    a.Beta = L.fptr(_stack(keep, [np.asarray(b, dtype=np.float64).reshape(-1, order="F") for b in betas]))
    a.sigma = L.fptr(_stack(keep, [np.asarray(s, dtype=np.float64).ravel() for s in sigmas]))
    a.family = L.colmajor_ptr(family, keep, np.int32)
    a.Pi = L.colmajor_ptr(Pi, keep, np.int32)
    obs = ~np.isnan(Yc)
    nps, nfs, ncls, outs = [], [], [], []
    EtaOut = (L.dp * L.MAX_LEVELS)()
    levels = (L.hmsc_cond_spatial * L.MAX_LEVELS)() if spatial is not None else None
    for r in range(nr):
        npr = int(np.asarray(etas[0][r]).shape[0])
        nf, stacks = stack_device_levels(keep, [e[r] for e in etas], [lm[r] for lm in lams])
        out = np.empty(S * npr * nf)
        keep.append(out)
        a.Eta[r], a.Lambda[r] = L.fptr(stacks[0][0]), L.fptr(stacks[0][1])
        EtaOut[r] = L.fptr(out)
        nps.append(npr)
        nfs.append(nf)
        outs.append(out)
        sp = spatial[r] if spatial is not None else None
        if sp is not None:   # a spatial level: cnt / unit_class are not read
            vals, idx = cond_grid_in_use(sp["alphapw"], sp["Alpha"], nf, name=str(r))
            keep += [vals, idx]
            q = levels[r]
            q.method, q.nalpha, q.alphas, q.AlphaIdx = 1, vals.size, L.fptr(vals), L.iptr(idx)
            if sp.get("gpp") is not None:
                idD, idDW12, F = sp["gpp"](vals)
                q.method, q.nK = 3, F.shape[0]
                q.idDg, q.idDW12g, q.Fg = (L.colmajor_ptr(np.asarray(v, dtype=np.float64), keep) for v in (idD, idDW12, F))
            elif sp.get("dist") is not None:
                q.dist = L.colmajor_ptr(np.asarray(sp["dist"], dtype=np.float64), keep)
            else:
                crd = np.asarray(sp["coords"], dtype=np.float64).reshape(npr, -1)
                q.sDim, q.coords = crd.shape[1], L.colmajor_ptr(crd, keep)
            ncls.append(0)
            continue
        cnt, ucls = cond_classes(obs, Pi[:, r] - 1, npr)
        keep += [cnt, ucls]
        a.cnt[r], a.unit_class[r] = L.iptr(cnt), L.iptr(ucls)
        ncls.append(cnt.shape[0])
    a.np = L.colmajor_ptr(nps, keep, np.int32)
    a.nf = L.colmajor_ptr(nfs, keep, np.int32)
    a.ncls = L.colmajor_ptr(ncls, keep, np.int32)
    if levels is None:
        L.check(L.lib().hmsc_predict_conditional(C.byref(a), EtaOut))
    else:
        L.check(L.lib().hmsc_predict_conditional_spatial(C.byref(a), levels, EtaOut))
    res = []
    for k in range(S):
        res.append([outs[r].reshape(S, nfs[r], nps[r])[k].T[:, :np.asarray(etas[k][r]).shape[1]].copy()
                    for r in range(nr)])
    return res


def _conditional_etas_batched(hM, post, X, betas, studyDesign, Yc, mcmcStep, rng, device, krigeKey=None,
                              spatial=False):
    """_conditional_etas with every sample in one device call (conditional_etas_device).  It takes
    from the seeded generator what _conditional_etas takes, in its order -- the chain key, then
    the starting Eta of new units sample by sample and level by level (or, with krigeKey, from the
    device under that key) -- so for a given seed both paths start from the same Eta under the same
    key.  betas: the per-sample coefficients of the columns of X (an RRR model's stacked ones).
    spatial (condSpatial): the model's 'Full' levels go to the call with the prediction units'
    coordinates or distances, its 'GPP' levels with the low-rank arrays of the grid values in use,
    both in the unit order of the conditioning model, which is built as _conditional_etas builds it."""
    sd = studyDesign.reset_index(drop=True) if hasattr(studyDesign, "reset_index") else studyDesign
    sp = None
    if spatial and any(rl.sDim for rl in hM.rL):
        from .dataparams import _level_order, gpp_grid_values
        from .model import Hmsc
        hMc = Hmsc(Y=Yc, X=X, XScale=False, YScale=False, distr=hM.distr, studyDesign=sd,
                   ranLevels={name: hM.rL[r] for r, name in enumerate(hM.rLNames)})
        sp = []
        for r, lv in enumerate(hM.rL):
            if not lv.sDim:
                sp.append(None)
                continue
            if lv.spatialMethod == "GPP":
                nf = max(int(np.asarray(s["Eta"][r]).shape[1]) for s in post)
                _cond_gpp_check(hM.rLNames[r], int(hMc.np[r]), int(hMc.ny), nf, np.asarray(lv["sKnot"]).shape[0])
                geo = dict(gpp=lambda vals, r=r, lv=lv: gpp_grid_values(hMc, r, lv, vals))
            else:
                idx = _level_order(hMc, r, lv)
                geo = (dict(coords=np.asarray(lv.s, dtype=np.float64)[idx]) if lv.distMat is None else
                       dict(dist=np.asarray(lv.distMat, dtype=np.float64)[np.ix_(idx, idx)]))
            sp.append(dict(alphapw=lv.alphapw, Alpha=[s["Alpha"][r] for s in post], **geo))
    key = int(rng.integers(1, 2 ** 62))
    units = [_levels(hM.dfPi[name]) for name in hM.rLNames]
    unitsPred = [_levels(sd[name]) for name in hM.rLNames]
    alpha = lambda r, sams: [s["Alpha"][r] for s in sams] if hM.rL[r].sDim else None  # noqa: E731
    if krigeKey is not None:
        dev_etas = [predictLatentFactor(unitsPred[r], units[r], [sam["Eta"][r] for sam in post], hM.rL[r],
                                        postAlpha=alpha(r, post), device=device, seed=krigeKey, level=r)
                    for r in range(hM.nr)]
        etas = [[de[k] for de in dev_etas] for k in range(len(post))]
    else:
        etas = [[predictLatentFactor(unitsPred[r], units[r], [sam["Eta"][r]], hM.rL[r], rng=rng,
                                     postAlpha=alpha(r, [sam]))[0]
                 for r in range(hM.nr)] for sam in post]
    Pi = np.zeros((X.shape[0], hM.nr), dtype=np.int32)
    for r, name in enumerate(hM.rLNames):
        idx = {u: k for k, u in enumerate(unitsPred[r])}
        Pi[:, r] = [idx[v] + 1 for v in np.asarray(sd[name]).astype(str)]
    return conditional_etas_device(X, betas, [np.asarray(s["sigma"], dtype=np.float64) for s in post], etas,
                                   [[np.asarray(lm, dtype=np.float64) for lm in s["Lambda"]] for s in post], Pi,
                                   hM.distr[:, 0], Yc, mcmcStep, key, device=device, spatial=sp)


def _stack(keep, arrays):
    flat = np.ascontiguousarray(np.concatenate(arrays).astype(np.float64)) if arrays else np.zeros(1)
    keep.append(flat)
    return flat


def computePredictedValues(hM, partition=None, start=1, thin=1, Yc=None, mcmcStep=1, expected=True,
                           initPar=None, nParallel=1, nChains=None, updater=None, verbose=None, seed=None,
                           krigeDevice=False, partition_sp=None, condBatch=False, summary=False, probs=(),
                           gppDevice=False, condSpatial=False):
    """R/computePredictedValues.R:66-142: ny x ns x predN.  Without a partition, the fitted
    model's own predictions; with one, K-fold cross-validation refits (sampleMcmc on the
    training rows with the fitted run's samples / transient / thin, predictions for the
    held-out rows).  krigeDevice goes to predict: the held-out units of a spatial level are kriged
    on the device (every fold of a spatially blocked partition has them); gppDevice goes with it, for
    the held-out units of a GPP level.
    partition_sp (R's partition.sp, :125-140): a length-ns vector of species folds.  Per row fold,
    after the refit, the species of each species fold are predicted conditionally on the held-out
    rows' data of all the other species (Yc = NA, Yc[, train.sp] = Y[val, train.sp]; mcmcStep
    updates); the Yc argument is not used then.  As in R it is ignored without `partition`.  A
    given seed fixes every species fold's predict seed (cv_sp_fold_seed).  condBatch and
    condSpatial go to predict.
    summary=True returns predictSummary's dict (mean, occ, n, probs, quantiles, median) in place of
    the array, never forming it: every fold fills its held-out rows, every species fold its columns,
    under the seeds of the array path, so the dict summarises the array the same call would return.
    probs goes to predictSummary."""
    if summary:
        _summary_probs(hM, probs)      # refusals before any refit or device call
    if partition_sp is not None:
        partition_sp = np.asarray(partition_sp).reshape(-1)
        if partition_sp.shape[0] != hM.ns:
            raise ValueError("HMSC.computePredictedValues: partition.sp parameter must be a vector of length ns")
    if partition is None:
        post = poolMcmcChains(hM.postList, start=start, thin=thin)
        if summary:
            return predictSummary(hM, post=post, Yc=Yc, mcmcStep=mcmcStep, expected=expected, seed=seed,
                                  krigeDevice=krigeDevice, condBatch=condBatch, probs=probs, gppDevice=gppDevice,
                                  condSpatial=condSpatial)
        pred = predict(hM, post=post, Yc=Yc, mcmcStep=mcmcStep, expected=expected, seed=seed, krigeDevice=krigeDevice,
                       condBatch=condBatch, gppDevice=gppDevice, condSpatial=condSpatial)
        return np.stack(pred, axis=2)
    partition = np.asarray(partition)
    nfolds = len(np.unique(partition))
    nChains = len(hM.postList) if nChains is None else nChains
    postN = hM.samples * nChains
    out = None if summary else np.full((hM.ny, hM.ns, postN), np.nan)
    sm = None
    for k in np.unique(partition):
        train, val = partition != k, partition == k
        hM1 = _cv_refit(hM, train, k, seed, nChains, updater, initPar, nParallel)
        post = poolMcmcChains(hM1.postList, start=start)
        sdv = None if hM.studyDesign is None else hM.studyDesign.loc[val].reset_index(drop=True)
        kw = dict(post=post, X=hM.X[val], studyDesign=sdv, mcmcStep=mcmcStep, expected=expected,
                  XRRR=hM["XRRR"][val] if hM.ncRRR else None,   # XRRRVal (:87,126)
                  krigeDevice=krigeDevice, condBatch=condBatch, gppDevice=gppDevice, condSpatial=condSpatial)
        if partition_sp is None:
            if summary:
                sm = _summary_fill(sm, hM, val, slice(None), predictSummary(
                    hM1, Yc=None if Yc is None else np.asarray(Yc)[val], seed=seed, probs=probs, **kw))
                continue
            pred = predict(hM1, Yc=None if Yc is None else np.asarray(Yc)[val], seed=seed, **kw)
            out[val] = np.stack(pred, axis=2)
            continue
        pred1 = None if summary else np.full((int(val.sum()), hM.ns, postN), np.nan)
        for i in np.unique(partition_sp):                                       # :131-139
            val_sp = partition_sp == i
            if summary:
                sm = _summary_fill(sm, hM, val, val_sp, predictSummary(
                    hM1, Yc=cv_sp_fold_yc(hM.Y[val], partition_sp, i), seed=cv_sp_fold_seed(seed, k, i), probs=probs,
                    **kw))
                continue
            pred2 = predict(hM1, Yc=cv_sp_fold_yc(hM.Y[val], partition_sp, i), seed=cv_sp_fold_seed(seed, k, i), **kw)
            pred1[:, val_sp] = np.stack(pred2, axis=2)[:, val_sp]
        if not summary:
            out[val] = pred1
    del nfolds
    return sm if summary else out


def _summary_fill(sm, hM, rows, cols, part):
    """A fold's predictSummary dict into the whole model's (made on first use): the held-out rows
    `rows` and the species `cols` of every matrix; cells no fold fills stay NaN with n = 0."""
    if sm is None:
        nq = len(part["probs"])
        sm = dict(mean=np.full((hM.ny, hM.ns), np.nan), occ=np.full((hM.ny, hM.ns), np.nan),
                  n=np.zeros((hM.ny, hM.ns), dtype=np.int32), probs=part["probs"],
                  quantiles=np.full((nq, hM.ny, hM.ns), np.nan), median=np.full((hM.ny, hM.ns), np.nan))
    ri = np.nonzero(rows)[0]
    cj = np.arange(hM.ns)[cols]
    for key in ("mean", "occ", "n", "median"):
        sm[key][np.ix_(ri, cj)] = part[key][:, cj]
    sm["quantiles"][np.ix_(np.arange(sm["quantiles"].shape[0]), ri, cj)] = part["quantiles"][:, :, cj]
    return sm


def _cv_fold_model(hM, train):
    """R/computePredictedValues.R:92-116: the model on the training rows, with the full
    model's scalings."""
    from .model import Hmsc
    sd = None if hM.studyDesign is None else hM.studyDesign.loc[train].reset_index(drop=True)
    rl = {name: hM.ranLevels[name] for name in hM.rLNames} if hM.nr else None
    rrr = dict(XRRR=hM["XRRR"][train], ncRRR=hM.ncRRR) if hM.ncRRR else {}      # XRRRTrain (:85-91)
    sel = dict(XSelect=hM["XSelect"]) if hM.ncsel else {}                       # XSelect = hM$XSelect (:92)
    hM1 = Hmsc(Y=hM.Y[train], X=hM.X[train], Tr=hM.Tr, distr=hM.distr, C=hM.C,                   # :92
               studyDesign=sd, ranLevels=rl, covNames=list(hM.covNames[:hM.ncNRRR]), spNames=list(hM.spNames), **rrr,
               **sel)
    # :93-94 calls setPriors(hM1, V0 = hM$V0, ...) without assigning its result, so the refit
    # keeps Hmsc()'s default priors (the random levels' priors travel with ranLevels); the
    # scalings are the full model's (:95-116)
    hM1.YScalePar = hM.YScalePar
    hM1.YScaled = (hM1.Y - hM1.YScalePar[0][None, :]) / hM1.YScalePar[1][None, :]
    hM1.XInterceptInd = hM.XInterceptInd
    hM1.XScalePar = hM.XScalePar
    hM1.XScaled = (np.asarray(hM1.X, dtype=np.float64) - hM1.XScalePar[0][None, :]) / hM1.XScalePar[1][None, :]
    if hM1.ncRRR:                                                               # :110-113
        hM1.XRRRScalePar = hM.XRRRScalePar
        hM1.XRRRScaled = (hM1["XRRR"] - hM1.XRRRScalePar[0][None, :]) / hM1.XRRRScalePar[1][None, :]
    hM1.TrInterceptInd = hM.TrInterceptInd
    hM1.TrScalePar = hM.TrScalePar
    hM1.TrScaled = (np.asarray(hM1.Tr, dtype=np.float64) - hM1.TrScalePar[0][None, :]) / hM1.TrScalePar[1][None, :]
    return hM1


def cv_fold_seed(seed, k):
    """Seed of fold k's refit: R draws the refit's chain seeds from its global RNG; here a given
    predict seed fixes them per fold (None: fresh seeds)."""
    return None if seed is None else int(np.random.default_rng([int(seed), int(k)]).integers(1, 2 ** 62))


def cv_sp_fold_seed(seed, k, i):
    """Seed of predict for species fold i of row fold k (None: fresh draws): one generator state
    per (seed, k, i), apart from cv_fold_seed's (seed, k)."""
    return None if seed is None else int(np.random.default_rng([int(seed), int(k), int(i), 1]).integers(1, 2 ** 62))


def cv_sp_fold_yc(Yval, partition_sp, i):
    """R/computePredictedValues.R:134-135: Yc = NA; Yc[, train.sp] = Y[val, train.sp] for species
    fold i (train.sp = partition.sp != i)."""
    Yval = np.asarray(Yval, dtype=np.float64)
    Yc = np.full(Yval.shape, np.nan)
    train_sp = np.asarray(partition_sp) != i
    Yc[:, train_sp] = Yval[:, train_sp]
    return Yc


def _cv_refit(hM, train, k, seed, nChains, updater, initPar, nParallel):
    """R/computePredictedValues.R:117: sampleMcmc of the fold model with the fitted run's
    samples / transient / thin / adaptNf."""
    from .sampler import sampleMcmc
    return sampleMcmc(_cv_fold_model(hM, train), samples=hM.samples, thin=hM.thin, transient=hM.transient,
                      nChains=nChains, adaptNf=getattr(hM, "adaptNf", None), updater=updater, initPar=initPar,
                      verbose=0, nParallel=nParallel, seed=cv_fold_seed(seed, k))


def _auc(y, p):
    """pROC::auc(levels=c(0,1), direction="<"): Mann-Whitney with average ranks for ties."""
    r = stats.rankdata(p)
    n1 = np.sum(y == 1)
    n0 = np.sum(y == 0)
    return (np.sum(r[y == 1]) - n1 * (n1 + 1) / 2) / (n1 * n0)


MODEL_FIT_KEYS = ("RMSE", "R2", "AUC", "TjurR2", "SR2", "O.AUC", "O.TjurR2", "O.RMSE", "C.SR2", "C.RMSE")
_MODEL_FIT_FAMILY = {1: ("R2",), 2: ("AUC", "TjurR2"), 3: ("SR2", "O.AUC", "O.TjurR2", "O.RMSE", "C.SR2", "C.RMSE")}


def model_fit_device(Y, m, pO, family, device=0, chunk_rows=0, scratch_bytes=0):
    """hmsc_model_fit (modelfit.hip) on ny x ns matrices: the 10 x ns measures in the order of
    MODEL_FIT_KEYS, NaN outside each measure's family.  pO is read in Poisson columns only and may
    be None when there are none."""
    Y, m = np.asarray(Y, dtype=np.float64), np.asarray(m, dtype=np.float64)
    family = L.i32(family)
    if Y.ndim != 2 or m.shape != Y.shape or family.shape != (Y.shape[1],):
        raise ValueError(f"model_fit_device: Y {Y.shape}, m {m.shape} and family {family.shape} do not agree")
    if pO is not None and np.shape(pO) != Y.shape:
        raise ValueError(f"model_fit_device: pO {np.shape(pO)} is not Y's shape {Y.shape}")
    if int(chunk_rows) < 0 or int(scratch_bytes) < 0:
        raise ValueError("model_fit_device: chunk_rows and scratch_bytes must not be negative")
    keep = []
    a = L.hmsc_model_fit_args()
    a.device, a.ny, a.ns = int(device), Y.shape[0], Y.shape[1]
    a.Y, a.m = L.colmajor_ptr(Y, keep), L.colmajor_ptr(m, keep)
    a.pO = None if pO is None else L.colmajor_ptr(pO, keep)
    a.family = L.iptr(family)
    a.chunk_rows, a.scratch_bytes = int(chunk_rows), int(scratch_bytes)
    out = np.empty((len(MODEL_FIT_KEYS), Y.shape[1]))
    L.check(L.lib().hmsc_model_fit(C.byref(a), L.fptr(out)))
    return out


def evaluateModelFit(hM, predY=None, summary=None, device=None, chunk_rows=0, scratch_bytes=0):
    """R/evaluateModelFit.R: RMSE for all species; R2 (normal); AUC and TjurR2 (probit);
    SR2, O.AUC, O.TjurR2, O.RMSE, C.SR2, C.RMSE (Poisson).  Exactly one of predY (the ny x ns x predN
    array of computePredictedValues) and summary (its summary=True dict) is given: the measures
    need the per-cell mean (the median for Poisson columns) and the share of positive values, which
    is all they take from the array.

    device=None computes the measures on the host, species by species.  device=d forms the same two
    matrices and makes one hmsc_model_fit call on device d (modelfit.hip; chunk_rows and
    scratch_bytes as in include/hmsc_amd.h, neither changes a result): the same dict, AUC and O.AUC
    bit-equal to the host's, the rest within the rounding bounds of DESIGN.md §4."""
    if (predY is None) == (summary is None):
        raise ValueError("evaluateModelFit: give exactly one of predY and summary")
    if device is not None and (isinstance(device, bool) or not isinstance(device, (int, np.integer)) or device < 0):
        raise ValueError(f"evaluateModelFit: device = {device!r} is not a device index")
    Y = np.asarray(hM.Y, dtype=np.float64)
    fam = hM.distr[:, 0]
    pois = fam == 3
    m = np.full((hM.ny, hM.ns), np.nan)
    pO = np.full((hM.ny, hM.ns), np.nan)
    if summary is not None:
        m[:, ~pois] = np.asarray(summary["mean"])[:, ~pois]
        m[:, pois] = np.asarray(summary["median"])[:, pois]
        pO[:, pois] = np.asarray(summary["occ"])[:, pois]
    else:
        with np.errstate(all="ignore"):
            if pois.any():
                m[:, pois] = np.nanmedian(predY[:, pois, :], axis=2)
                pO[:, pois] = np.nanmean((predY[:, pois, :] > 0).astype(float), axis=2)
            if (~pois).any():
                m[:, ~pois] = np.nanmean(predY[:, ~pois, :], axis=2)

    if device is not None:
        out = model_fit_device(Y, m, pO if pois.any() else None, fam, device=device, chunk_rows=chunk_rows,
                               scratch_bytes=scratch_bytes)
        keys = ("RMSE",) + tuple(k for f in (1, 2, 3) if (fam == f).any() for k in _MODEL_FIT_FAMILY[f])
        return {k: out[MODEL_FIT_KEYS.index(k)].copy() for k in keys}

    def rmse(Yc, P):
        return np.sqrt(np.nanmean((Yc - P) ** 2, axis=0))

    def r2(Yc, P, method="pearson"):
        out = np.full(Yc.shape[1], np.nan)
        for j in range(Yc.shape[1]):
            ok = ~np.isnan(Yc[:, j]) & ~np.isnan(P[:, j])
            if ok.sum() > 1:
                if method == "spearman":
                    co = stats.spearmanr(Yc[ok, j], P[ok, j])[0]
                else:
                    co = np.corrcoef(Yc[ok, j], P[ok, j])[0, 1]
                out[j] = np.sign(co) * co ** 2
        return out

    def auc(Yc, P):
        Yb = np.where(np.isnan(Yc), np.nan, (Yc > 0).astype(float))
        out = np.full(Yc.shape[1], np.nan)
        for j in range(Yc.shape[1]):
            sel = ~np.isnan(Yb[:, j])
            if len(np.unique(Yb[sel, j])) == 2:
                out[j] = _auc(Yb[sel, j], P[sel, j])
        return out

    def tjur(Yc, P):
        return np.array([np.mean(P[Yc[:, j] == 1, j]) - np.mean(P[Yc[:, j] == 0, j]) for j in range(Yc.shape[1])])

    res = dict(RMSE=rmse(Y, m))
    sel = fam == 1
    if sel.any():
        res["R2"] = np.full(hM.ns, np.nan)
        res["R2"][sel] = r2(Y[:, sel], m[:, sel])
    sel = fam == 2
    if sel.any():
        res["AUC"] = np.full(hM.ns, np.nan)
        res["TjurR2"] = np.full(hM.ns, np.nan)
        res["AUC"][sel] = auc(Y[:, sel], m[:, sel])
        res["TjurR2"][sel] = tjur(Y[:, sel], m[:, sel])
    sel = fam == 3
    if sel.any():
        Ys, ms = Y[:, sel], m[:, sel]
        res["SR2"] = np.full(hM.ns, np.nan)
        res["SR2"][sel] = r2(Ys, ms, method="spearman")
        Yo = np.where(np.isnan(Ys), np.nan, (Ys > 0).astype(float))
        pO = pO[:, sel]
        for key, val in (("O.AUC", auc(Yo, pO)), ("O.TjurR2", tjur(Yo, pO)), ("O.RMSE", rmse(Yo, pO))):
            res[key] = np.full(hM.ns, np.nan)
            res[key][sel] = val
        with np.errstate(all="ignore"):
            mc = ms / pO                                    # mPredCY = mPredY / mPredO  (:150)
        Yc = np.where(Ys == 0, np.nan, Ys)                  # CY[CY == 0] = NA  (:151-152)
        res["C.SR2"] = np.full(hM.ns, np.nan)
        res["C.RMSE"] = np.full(hM.ns, np.nan)
        res["C.SR2"][sel] = r2(Yc, mc, method="spearman")
        res["C.RMSE"][sel] = rmse(Yc, mc)
    return res
