"""Models, hand-made pooled posteriors and prediction grids for predictMap's tests
(test_gpu_predict_map.py, test_host_predict_map.py).  No device library is touched here."""
import numpy as np
import pandas as pd

from helpers import H

NP, NS, NSAMP, NSITE = 70, 37, 9, 12
GRID = np.array([0.0, 0.05, 0.1, 0.2, 0.35, 0.5, 0.8, 1.1])      # alphapw[, 1]: index 1 is a = 0
ALPHA_IDX = [1, 3, 5, 8, 3, 8, 5, 1]                               # cycled over the (sample, factor) pairs


def model(method="Full", seed=21, families=(1, 2, 3), xdim=False, distmat=False, ns=NS, **rl_kw):
    """An unfitted model of NP spatial units ("plot": one per row, named coordinates) and NSITE
    non-spatial units ("site"), ns species whose families cycle through `families` (1 normal, 2 probit,
    3 Poisson), Y scaled (a non-trivial YScalePar on the normal columns), two covariates, two traits."""
    rng = np.random.default_rng(seed)
    xy = rng.random((NP, 2))
    names = [f"p{k:03d}" for k in range(NP)]
    fam = np.array(families)[np.arange(ns) % len(families)]
    Y = np.empty((NP, ns))
    for j, f in enumerate(fam):
        z = rng.standard_normal(NP)
        Y[:, j] = 3.0 * z + 1.5 if f == 1 else (z > 0).astype(float) if f == 2 else rng.poisson(np.exp(0.5 * z))
    distr = [{1: "normal", 2: "probit", 3: "poisson"}[int(f)] for f in fam]
    XData = pd.DataFrame({"x1": rng.standard_normal(NP), "x2": rng.standard_normal(NP)})
    if rl_kw.get("sKnot") == "auto":
        from hmsc_amd.dataparams import constructKnots
        rl_kw["sKnot"] = constructKnots(xy, nKnots=3)
    if distmat:
        d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
        rl = H.HmscRandomLevel(distMat=pd.DataFrame(d, index=names, columns=names))
    else:
        rl = H.HmscRandomLevel(sData=pd.DataFrame(xy, index=names), sMethod=method, **rl_kw)
    H.setPriors(rl, nfMin=2, nfMax=3, alphapw=np.column_stack([GRID, np.full(len(GRID), 1.0 / len(GRID))]))
    site = np.array([f"u{k:02d}" for k in np.arange(NP) % NSITE])
    if xdim:
        xdf = pd.DataFrame({"c0": np.ones(NSITE), "c1": rng.standard_normal(NSITE)},
                           index=[f"u{k:02d}" for k in range(NSITE)])
        rs = H.HmscRandomLevel(xData=xdf)
    else:
        rs = H.HmscRandomLevel(units=site)
    H.setPriors(rs, nfMin=2, nfMax=3)
    Tr = np.column_stack([np.ones(ns), rng.standard_normal(ns)])
    return H.Hmsc(Y=Y, XData=XData, XFormula="~x1+x2", Tr=Tr, distr=distr, YScale=True,
                  studyDesign=pd.DataFrame({"plot": names, "site": site}), ranLevels={"plot": rl, "site": rs})


def posterior(hM, S=NSAMP, seed=22):
    """S pooled samples whose factor counts alternate between 2 and 3 in both levels; the spatial
    level's alpha indices cycle through ALPHA_IDX (the a = 0 grid point and three positive ones)."""
    rng = np.random.default_rng(seed)
    post, q = [], 0
    fam = np.asarray(hM.distr)[:, 0]
    for k in range(S):
        nf0, nf1 = 2 + k % 2, 3 - k % 2
        sigma = rng.uniform(0.3, 1.5, hM.ns)
        sigma[fam == 2] = 1.0
        sigma[fam == 3] = 0.0
        alpha = np.array([ALPHA_IDX[(q + h) % len(ALPHA_IDX)] for h in range(nf0)])
        q += nf0
        post.append(dict(Beta=0.5 * rng.standard_normal((hM.nc, hM.ns)), sigma=sigma,
                         Eta=[rng.standard_normal((NP, nf0)), rng.standard_normal((NSITE, nf1))],
                         Lambda=[0.5 * rng.standard_normal((nf0, hM.ns)), 0.5 * rng.standard_normal((nf1, hM.ns))],
                         Alpha=[alpha, np.zeros(nf1, dtype=np.int64)]))
    return post


def grid(hM, nn, seed=23):
    """prepareGradient over nn new sites: every row its own new spatial unit, all rows the
    non-spatial "new_unit"."""
    rng = np.random.default_rng(seed)
    XDataNew = pd.DataFrame({"x1": rng.standard_normal(nn), "x2": rng.standard_normal(nn)})
    return H.prepareGradient(hM, XDataNew, {"plot": rng.random((nn, 2))})


def shared_units(G, pairs=((20, 120),)):
    """The Gradient with row b given row a's new spatial unit for every (a, b)."""
    sd = G["studyDesignNew"].copy()
    for a, b in pairs:
        sd.loc[b, "plot"] = sd.loc[a, "plot"]
    return dict(XDataNew=G["XDataNew"], studyDesignNew=sd, rLNew=G["rLNew"])
