"""The gradient workflow after predict: constructGradient (R/constructGradient.R),
prepareGradient (R/prepareGradient.R), community-level posterior summaries on the device
(predictCommunity -> hmsc_predict_community, hmsc_amd/csrc/community.hip) and plotGradient's
numbers without the figure (gradientSummary, R/plotGradient.R:63-138).

A Gradient is a dict with R's three fields: XDataNew (a data frame), studyDesignNew (a data frame
of unit names per random level) and rLNew (the levels by name, with the new units appended);
predict, predictSummary and predictCommunity take it as ``Gradient=``.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .model import _parse_formula
from .predict import _levels, _new_design, krige_description, _predict_args, _summary_probs, _unpack_cells

COMMUNITY_MAX_COLUMNS = 16
COMMUNITY_MAX_PROBS = 8
COMMUNITY_MAX_PAIRS = 8


def _is_factor(v):
    import pandas as pd
    return not pd.api.types.is_numeric_dtype(v) or pd.api.types.is_bool_dtype(v)


def _mode(x):
    """R/constructGradient.R:42-48: the most frequent value, the first met among ties."""
    vals = list(x)
    ux = list(dict.fromkeys(vals))
    counts = [vals.count(u) for u in ux]
    return ux[int(np.argmax(counts))]


def _focal_design(v, factor, levels=None):
    """The design matrix of `~ v.focal`: intercept and slope, or intercept and treatment dummies."""
    if not factor:
        return np.column_stack([np.ones(len(v)), np.asarray(v, dtype=np.float64)])
    sv = np.array([str(x) for x in v])
    return np.column_stack([np.ones(len(sv))] + [(sv == lv).astype(np.float64) for lv in levels[1:]])


def multinom_fit(D, y, nclass, maxit=200, tol=1e-12):
    """The multinomial-logit maximum-likelihood fit of classes y (0 .. nclass - 1) on the design D
    (n x p), baseline = class 0: Newton steps on the log-likelihood with step halving, until a step
    gains less than tol (1 + |ll|).  Returns the p x (nclass - 1) coefficients.  Under perfect
    separation the likelihood has no maximum; the iteration then stops at maxit with the classes
    already separated."""
    D = np.asarray(D, dtype=np.float64)
    n, p = D.shape
    Y = np.zeros((n, nclass))
    Y[np.arange(n), np.asarray(y, dtype=np.int64)] = 1.0
    B = np.zeros((p, nclass - 1))

    def loglik(B):
        eta = np.column_stack([np.zeros(n), D @ B])
        mx = eta.max(axis=1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(eta - mx).sum(axis=1))
        return float((Y * eta).sum() - lse.sum()), np.exp(eta - lse[:, None])

    ll, P = loglik(B)
    for _ in range(maxit):
        R = (Y - P)[:, 1:]
        grad = (D.T @ R).reshape(-1, order="F")
        q = nclass - 1
        H = np.zeros((p * q, p * q))
        for a in range(q):
            for b in range(q):
                w = P[:, a + 1] * ((1.0 if a == b else 0.0) - P[:, b + 1])
                H[a * p:(a + 1) * p, b * p:(b + 1) * p] = D.T @ (D * w[:, None])
        try:
            step = np.linalg.solve(H, grad)
        except np.linalg.LinAlgError:
            step = np.linalg.lstsq(H, grad, rcond=None)[0]
        if not np.all(np.isfinite(step)):
            break
        t, moved = 1.0, False
        while t > 1e-10:
            Bn = B + t * step.reshape(p, q, order="F")
            lln, Pn = loglik(Bn)
            if np.isfinite(lln) and lln > ll:
                moved = True
                break
            t *= 0.5
        if not moved:
            break
        gain = lln - ll
        B, ll, P = Bn, lln, Pn
        if gain < tol * (1.0 + abs(ll)):
            break
    return B


def multinom_predict(B, Dnew):
    """The most probable class at each row of Dnew (predict.multinom's type = "class"); the first
    class among exactly tied ones."""
    Dnew = np.asarray(Dnew, dtype=np.float64)
    eta = np.column_stack([np.zeros(Dnew.shape[0]), Dnew @ B])
    return np.argmax(eta, axis=1)


def constructGradient(hM, focalVariable, non_focalVariables=None, ngrid=20):
    """R/constructGradient.R for a model defined with an XData frame (nz = 1): ngrid points along the
    focal variable from its minimum to its maximum (a focal factor: its levels), every other
    variable of XFormula set by its type in non_focalVariables, a dict name -> (type,) or
    (type, value): 1 the mean (a factor: the mode), 2 its regression on the focal variable (the
    default), 3 the given value.  Returns dict(XDataNew, studyDesignNew, rLNew): "new_unit" in
    every level, whose coordinates are the column means of rL$s; for a distMat level its distances
    are the means of the two rows with the smallest row means (:198-207).

    Type 2 for a non-focal factor is nnet::multinom in R; here it is the multinomial-logit
    maximum-likelihood fit (multinom_fit: Newton with step halving, baseline = first level) and the
    most probable class.  nnet stops at its own tolerance short of the maximum, so the class can
    differ from R's where two probabilities are nearly tied."""
    import pandas as pd
    if isinstance(hM.XData, list):
        raise NotImplementedError("constructGradient: species-specific XData lists are out of scope")
    if hM.XData is None:
        raise ValueError("constructGradient: the model must be defined with XData and XFormula")
    XData = pd.DataFrame(hM.XData)
    variables = _parse_formula(hM.XFormula, list(XData.columns))[1]
    if focalVariable not in variables:
        raise ValueError(f"constructGradient: focalVariable {focalVariable!r} is not a variable of XFormula")
    spec = {}
    for name, val in (non_focalVariables or {}).items():
        val = list(val) if isinstance(val, (list, tuple)) else [val]
        spec[name] = (int(val[0]), val[1] if len(val) > 1 else None)
    v_focal = XData[focalVariable]
    f_focal = _is_factor(v_focal)
    if f_focal:
        lev_focal = _levels(v_focal)
        xx = list(lev_focal)
        ngrid = len(xx)
        D, Dnew = _focal_design(v_focal, True, lev_focal), _focal_design(xx, True, lev_focal)
    else:
        lev_focal = None
        xx = np.linspace(float(np.min(v_focal)), float(np.max(v_focal)), int(ngrid))
        ngrid = len(xx)
        D, Dnew = _focal_design(v_focal, False), _focal_design(xx, False)
    new = {focalVariable: xx}
    for name in variables:
        if name == focalVariable:
            continue
        kind, val = spec.get(name, (2, None))
        v = XData[name]
        if kind not in (1, 2, 3):
            raise ValueError(f"constructGradient: type of non-focal variable {name} must be 1, 2 or 3")
        if kind == 3:
            new[name] = [val] * ngrid
        elif _is_factor(v):
            if kind == 1:
                new[name] = [_mode(v)] * ngrid
            else:
                lev = _levels(v)
                pos = {lv: k for k, lv in enumerate(lev)}
                y = np.array([pos[str(x)] for x in v])
                cls = multinom_predict(multinom_fit(D, y, len(lev)), Dnew) if len(lev) > 1 else np.zeros(ngrid, int)
                new[name] = [lev[k] for k in cls]
        elif kind == 1:
            new[name] = np.full(ngrid, float(np.mean(v)))
        else:
            coef = np.linalg.lstsq(D, np.asarray(v, dtype=np.float64), rcond=None)[0]   # lm(v.non.focal ~ v.focal)
            new[name] = Dnew @ coef
    XDataNew = pd.DataFrame(new)
    studyDesignNew = pd.DataFrame({name: ["new_unit"] * ngrid for name in hM.rLNames})
    rLNew = {}
    for r, name in enumerate(hM.rLNames):
        rl = hM.rL[r].copy()
        units = _levels(hM.dfPi[name])
        if rl.s is not None:
            s = np.asarray(rl.s, dtype=np.float64)
            names = rl["sNames"] if "sNames" in rl.names() and rl["sNames"] is not None else units
            rl.s = np.vstack([s, s.mean(axis=0)])
            rl["sNames"] = [str(u) for u in names] + ["new_unit"]
        if rl.distMat is not None:
            dm = np.asarray(rl.distMat, dtype=np.float64)
            names = rl["distNames"] if "distNames" in rl.names() and rl["distNames"] is not None else units
            focals = np.argsort(dm.mean(axis=1), kind="stable")[:2]
            newdist = dm[focals].mean(axis=0)
            rl.distMat = np.block([[dm, newdist[:, None]], [newdist[None, :], np.zeros((1, 1))]])
            rl["distNames"] = [str(u) for u in names] + ["new_unit"]
        rl.pi = list(rl.pi if rl.pi is not None else units) + ["new_unit"]
        rl.N = int(rl.N) + 1
        rLNew[name] = rl
    return dict(XDataNew=XDataNew, studyDesignNew=studyDesignNew, rLNew=rLNew)


def prepareGradient(hM, XDataNew, sDataNew):
    """R/prepareGradient.R: a Gradient over a prediction grid.  XDataNew: the covariates of the new
    sampling units; sDataNew: a dict from a spatial level's name to the coordinates of its new
    units, one row per row of XDataNew.  A spatial level gets the units new_spatial_unit000001 ...
    with their coordinates appended to rL$s; a non-spatial level gets "new_unit" everywhere."""
    import pandas as pd
    nyNew = len(XDataNew)
    sd, rLNew = {}, {}
    for r, name in enumerate(hM.rLNames):
        rl = hM.rL[r].copy()
        units = _levels(hM.dfPi[name])
        if not rl.sDim:
            sd[name] = ["new_unit"] * nyNew
            rl.pi = list(rl.pi if rl.pi is not None else units) + ["new_unit"]
            rl.N = int(rl.N) + 1
        else:
            if rl.s is None:
                raise ValueError(f"prepareGradient: level {name} is defined by distMat; new units need coordinates")
            if sDataNew is None or name not in sDataNew:
                raise ValueError(f"prepareGradient: sDataNew holds no coordinates for the spatial level {name}")
            xyNew = np.asarray(sDataNew[name], dtype=np.float64)
            if xyNew.shape != (nyNew, int(rl.sDim)):
                raise ValueError(f"prepareGradient: sDataNew[{name!r}] must be {nyNew} x {int(rl.sDim)}")
            newu = [f"new_spatial_unit{k:06d}" for k in range(1, nyNew + 1)]
            sd[name] = newu
            names = rl["sNames"] if "sNames" in rl.names() and rl["sNames"] is not None else units
            rl.s = np.vstack([np.asarray(rl.s, dtype=np.float64), xyNew])
            rl["sNames"] = [str(u) for u in names] + newu
            rl.pi = list(rl.pi if rl.pi is not None else units) + newu
        rLNew[name] = rl
    return dict(XDataNew=XDataNew, studyDesignNew=pd.DataFrame(sd), rLNew=rLNew)


def _community_columns(hM, measures, weights):
    """The columns of a predictCommunity call: (name, weights (ns), normalise, transform) each."""
    cols = []
    all_normal = bool(np.all(np.asarray(hM.distr)[:, 0] == 1))
    for m in measures:
        if m == "S":
            cols.append(("S", np.ones(hM.ns), 0, 0))
        elif m == "T":
            Tr = np.asarray(hM.Tr, dtype=np.float64)
            for t, name in enumerate(hM.trNames):
                cols.append((str(name), Tr[:, t], 1, 1 if all_normal else 0))
        else:
            raise ValueError(f"predictCommunity: unknown measure {m!r} (\"S\" or \"T\"; species through weights)")
    if weights is not None:
        if hasattr(weights, "items"):
            named = [(str(k), np.asarray(v, dtype=np.float64).reshape(-1)) for k, v in weights.items()]
        else:
            Wu = np.asarray(weights, dtype=np.float64)
            Wu = Wu[:, None] if Wu.ndim == 1 else Wu
            named = [(f"w{k + 1}", Wu[:, k]) for k in range(Wu.shape[1])]
        for name, w in named:
            if w.shape[0] != hM.ns:
                raise ValueError(f"predictCommunity: weights column {name} must have one value per species")
            cols.append((name, w, 0, 0))
    if len(cols) > COMMUNITY_MAX_COLUMNS:
        raise ValueError(f"predictCommunity: at most {COMMUNITY_MAX_COLUMNS} community columns in one call; got "
                         f"{len(cols)}")
    if not cols:
        raise ValueError("predictCommunity: no column asked for (measures and weights are both empty)")
    return cols


def _community_checks(probs, contrast, ny=None):
    probs = [float(p) for p in np.asarray(probs, dtype=np.float64).reshape(-1)]
    if any(not (0.0 <= p <= 1.0) for p in probs):
        raise ValueError("predictCommunity: every probability in probs must lie in [0, 1]")
    if len(probs) > COMMUNITY_MAX_PROBS:
        raise ValueError(f"predictCommunity: at most {COMMUNITY_MAX_PROBS} probabilities in one call; got {len(probs)}")
    pairs = np.zeros((0, 2), dtype=np.int32)
    if contrast is not None:
        pairs = np.asarray(contrast, dtype=np.int64).reshape(-1, 2)
        if len(pairs) > COMMUNITY_MAX_PAIRS:
            raise ValueError(f"predictCommunity: at most {COMMUNITY_MAX_PAIRS} contrasts in one call; got {len(pairs)}")
        if ny is not None and (pairs.min(initial=0) < 0 or pairs.max(initial=0) >= ny):
            raise ValueError(f"predictCommunity: contrast names a row outside 0 .. {ny - 1}")
    return probs, np.ascontiguousarray(pairs, dtype=np.int32)


def predictCommunity(hM, post=None, X=None, studyDesign=None, Yc=None, mcmcStep=1, expected=False,
                     predictEtaMean=False, seed=None, device=0, predictEtaMeanField=False, XRRRData=None, XRRR=None,
                     krigeDevice=False, condBatch=False, XData=None, ranLevels=None, Gradient=None,
                     measures=("S", "T"), weights=None, probs=(0.025, 0.5, 0.975), contrast=None, returnSamples=False,
                     scratch_bytes=0, gppDevice=False, condSpatial=False):
    """Community-level summaries of predict's samples without the samples (hmsc_predict_community):
    the arguments of predict, and for one seed the summaries of the very values predict returns.
    measures: "S" is the row sum of a sample (species richness, the summed response, the total
    count); "T" the community-weighted means of the columns of hM.Tr, sum_j g(p_j) Tr[j, t] /
    sum_j g(p_j), with g = exp exactly when every family is normal (plotGradient's rule).  weights
    (ns x k, or a dict name -> ns vector) adds plain weighted sums; a zero weight leaves the species
    out (a unit vector returns that species' predictions).  contrast: a 0-based row pair (a, b) or
    up to 8 of them: Pr is the share of samples in which row b lies above row a.
    Returns dict(columns, mean, n (ny x nw), probs, quantiles (len(probs) x ny x nw, R's type 7), Pr
    (pairs x nw, None without contrast), samples (S x ny x nw with returnSamples, else None)).
    scratch_bytes bounds the device slab (0: 1 GiB); the results do not depend on it.  gppDevice and
    condSpatial are predict's."""
    cols = _community_columns(hM, measures, weights)
    probs, pairs = _community_checks(probs, contrast)
    a, keep, S, nyN = _predict_args(hM, post, X, studyDesign, Yc, mcmcStep, expected, predictEtaMean, seed, device,
                                    predictEtaMeanField, XRRRData, XRRR, krigeDevice, condBatch, XData, ranLevels,
                                    Gradient, gppDevice, condSpatial)
    _community_checks(probs, contrast, nyN)
    nw, npairs = len(cols), len(pairs)
    Pr = np.empty((npairs, nw)) if npairs else None
    samples = np.empty((S, nyN, nw)) if returnSamples else None
    blocks = _community_blocks(cols, nyN, probs)
    for b in blocks:        # one transform per device call
        c, sel, k = L.hmsc_community_args(), b.sel, len(b.sel)
        b.fill(c)
        c.npairs, c.pairs = npairs, L.iptr(pairs) if npairs else None
        c.scratch_bytes = int(scratch_bytes)
        p1 = np.empty(max(npairs, 1) * k)
        s1 = np.empty(S * k * nyN) if returnSamples else None
        L.check(L.lib().hmsc_predict_community(C.byref(a), C.byref(c), *b.out(), L.fptr(p1) if npairs else None,
                                               L.fptr(s1) if returnSamples else None))
        if npairs:
            Pr[:, sel] = p1[:npairs * k].reshape(k, npairs).T
        if returnSamples:
            samples[:, :, sel] = s1.reshape(S, k, nyN).transpose(0, 2, 1)
    del keep
    return dict(_community_gather(cols, blocks, nyN, probs), Pr=Pr, samples=samples)


class _CommunityBlock:
    """The community columns of one transform, one device block: sel, their places among the call's
    columns; the block's W, normalise and probs and its column-major result buffers n, mean and quant,
    which it owns for as long as the device call needs them."""

    def __init__(self, cols, sel, transform, nyN, probs):
        k, nq = len(sel), len(probs)
        self.sel, self.transform = sel, transform
        self.W = np.ascontiguousarray(np.column_stack([cols[j][1] for j in sel]).reshape(-1, order="F"))
        self.normalise = np.ascontiguousarray([cols[j][2] for j in sel], dtype=np.int32)
        self.probs = np.ascontiguousarray(probs, dtype=np.float64)
        self.n, self.mean, self.quant = np.empty(k * nyN, dtype=np.int32), np.empty(k * nyN), np.empty(max(nq, 1) * k * nyN)

    def fill(self, c):
        """A hmsc_community_args' nw, W, normalise, transform, nq and probs."""
        nq = len(self.probs)
        c.nw, c.W, c.normalise, c.transform = len(self.sel), L.fptr(self.W), L.iptr(self.normalise), self.transform
        c.nq, c.probs = nq, L.fptr(self.probs) if nq else None

    def out(self):
        """The output pointers (n, mean, quant or None) in the C ABI's order."""
        return L.iptr(self.n), L.fptr(self.mean), L.fptr(self.quant) if len(self.probs) else None


def _community_blocks(cols, nyN, probs):
    """One block per transform: the columns of either kind together, as the device takes them."""
    sels = [(tr, [k for k, c in enumerate(cols) if c[3] == tr]) for tr in (0, 1)]
    return [_CommunityBlock(cols, sel, tr, nyN, probs) for tr, sel in sels if sel]


def _community_gather(cols, blocks, nyN, probs):
    """predictCommunity's dict without Pr and samples from the filled blocks: columns, mean and n
    (ny x nw), probs, quantiles (nq x ny x nw)."""
    nw, nq = len(cols), len(probs)
    mean, n, quant = np.empty((nyN, nw)), np.empty((nyN, nw), dtype=np.int32), np.empty((nq, nyN, nw))
    for b in blocks:
        k = len(b.sel)
        mean[:, b.sel], n[:, b.sel] = b.mean.reshape(k, nyN).T, b.n.reshape(k, nyN).T
        if nq:
            quant[:, :, b.sel] = b.quant.reshape(nq, k, nyN).transpose(0, 2, 1)
    return dict(columns=[c[0] for c in cols], mean=mean, n=n, probs=np.array(probs), quantiles=quant)


MAP_SCRATCH_DEFAULT = 1 << 30
MAP_TILE = 64
MAP_BLOCKS_MAX = 1 << 23


def map_slab_rows(ny, nsamples, columns, slab_rows=0, scratch_bytes=0):
    """The rows of a slab of hmsc_predict_map (include/hmsc_amd.h): slab_rows as given, or the
    largest multiple of 64 whose scratch -- nsamples * 8 bytes per row and column, the columns being
    the flagged summary columns, the community columns and the factors of all levels -- fits
    scratch_bytes (0: 1 GiB); at most 2^23 / nsamples tiles of 64 rows, at most ny."""
    ny, S = int(ny), max(int(nsamples), 1)
    rows = int(slab_rows)
    if rows < 0:
        raise ValueError("predictMap: slab_rows must not be negative")
    if rows == 0:
        scratch = int(scratch_bytes) or MAP_SCRATCH_DEFAULT
        row_bytes = S * 8 * max(int(columns), 1)
        if MAP_TILE * row_bytes > scratch:
            raise ValueError(f"predictMap: one 64-row tile needs {MAP_TILE * row_bytes} bytes of scratch, scratch_bytes "
                             f"allows {scratch}")
        rows = scratch // row_bytes // MAP_TILE * MAP_TILE
    return max(1, min(rows, (MAP_BLOCKS_MAX // S) * MAP_TILE, ny))


def map_slab_plan(units, nps, slab_rows):
    """The slabs of a map, as hmsc_predict_map walks them.  units: per level the unit of every
    prediction row, 0-based: u < np a fitted unit, np + k the level's k-th new unit; nps: the fitted
    units per level; slab_rows: rows per slab (the last may be shorter).  Returns a list of dicts:
    row0, rows; units (per level the slab's distinct units in ascending order, fitted units first);
    new (per level the global indices k of its new units, the counters of their draws); Pi (rows x
    levels, the row's unit as its 0-based place in `units`).  A unit referred to from several slabs
    appears in each.  Pure: no device library."""
    units = [np.asarray(u, dtype=np.int64).reshape(-1) for u in units]
    ny = len(units[0]) if units else 0
    slab_rows = int(slab_rows)
    if slab_rows < 1:
        raise ValueError("map_slab_plan: slab_rows must be positive")
    plan = []
    for row0 in range(0, ny, slab_rows):
        rows = min(slab_rows, ny - row0)
        us, new = [], []
        Pi = np.zeros((rows, len(units)), dtype=np.int32)
        for r, u in enumerate(units):
            d, inv = np.unique(u[row0:row0 + rows], return_inverse=True)
            us.append(d.astype(np.int64))
            new.append((d[d >= nps[r]] - nps[r]).astype(np.int64))
            Pi[:, r] = np.reshape(inv, -1)
        plan.append(dict(row0=row0, rows=rows, units=us, new=new, Pi=Pi))
    return plan


def _map_level(hM, r, name, raw, post, predictEtaMean, predictEtaMeanField, gppDevice=False):
    """One level of a predictMap call, before any device call: the refusals, the row -> unit codes
    (0-based: fitted units, then the new units in the order of the prediction units' levels, which
    is hmsc_krige's index of a new unit) and the kriging description."""
    rl = hM.rL[r]
    if int(rl.xDim or 0):
        raise NotImplementedError(f"predictMap: level {name} has xData (covariate-dependent loadings, xDim > 0), "
                                  f"which maps do not serve; use predict")
    units = _levels(hM.dfPi[name])
    pos = {u: k for k, u in enumerate(units)}
    unitsPred = _levels(raw)
    newu = [u for u in unitsPred if u not in pos]
    code = dict(pos)
    code.update({u: len(units) + k for k, u in enumerate(newu)})
    unit = np.fromiter((code[v] for v in np.asarray(raw).astype(str)), dtype=np.int64, count=len(raw))
    S = len(post)
    nfs = [int(np.asarray(s["Eta"][r]).shape[1]) for s in post]
    nfmax = max(nfs)
    lev = dict(name=name, np=len(units), nn=len(newu), nf=nfmax, unit=unit, coords=None, dist=None, sDim=0,
               nNeighbours=int(rl.nNeighbours) if rl.nNeighbours is not None else 10, knots=None)
    if rl.sDim and newu:
        d = krige_description(rl, units, newu, predictEtaMean, predictEtaMeanField, gppDevice, nfs,
                              lambda k: post[k]["Alpha"][r])
        lev.update(coords=d["coords"], dist=d["dist"], sDim=d["sDim"], knots=d["knots"])
        mode, alphas, idx = d["mode"], d["alphas"], d["alpha"]
    else:
        # new units of a non-spatial level are N(0, 1): the one-point grid at alpha = 0
        mode, alphas, idx = (0 if predictEtaMean else 1), np.zeros(1), np.zeros((S, nfmax), dtype=np.int32)
        for k in range(S):
            idx[k, :nfs[k]] = 1
    lev.update(mode=mode, alphas=alphas, alpha=idx, nfs=nfs)
    return lev


def predictMap(hM, post=None, Gradient=None, X=None, XData=None, studyDesign=None, ranLevels=None, expected=True,
               predictEtaMean=False, predictEtaMeanField=False, seed=None, device=0, cells=True, probs=(), measures=(),
               weights=None, communityProbs=(0.025, 0.5, 0.975), slab_rows=0, scratch_bytes=0, factor_bytes=0,
               XRRRData=None, XRRR=None, gppDevice=False, **kw):
    """A pooled posterior mapped onto new sites in one device call (hmsc_predict_map): the reference's
    prepareGradient -> predict(Gradient =, predictEtaMean = TRUE) -> row sums and means at the size of
    a raster.  The prediction rows are walked in slabs; the latent factors of a slab's units -- the
    fitted units' posterior rows, N(0, 1) or 0 for new units of a non-spatial level, the kriging of
    new spatial units -- are made on the device and used there.  Returns dict(cells, community):
    cells is predictSummary's dict (None with cells=False, which skips the rows x species outputs),
    community predictCommunity's without Pr and samples (None without measures and weights).  For one
    seed both hold the doubles predictSummary(..., krigeDevice=True) and predictCommunity(...,
    krigeDevice=True) return, for every slab_rows.
    slab_rows: rows per slab (0: from scratch_bytes, 0 meaning 1 GiB: map_slab_rows); factor_bytes
    bounds the resident kriging factors and a slab's workspace (0: what the device has free).
    gppDevice=True serves a GPP level's joint conditional (mode 4 of hmsc_krige, gpp.hip): per grid
    value iWss and the knot-sized C = mu + eps stay resident and any slab is served, its new units
    being conditionally independent given the knot draw.
    Refused by name: a level with xData; GPP's joint conditional without gppDevice; a 'Full' joint draw (neither
    predictEtaMean nor predictEtaMeanField) whose new units do not fit one slab; Yc; draws without a
    seed."""
    if "Yc" in kw:
        raise TypeError("predictMap: Yc (conditional prediction) is not an argument of predictMap; use predict")
    if kw:
        raise TypeError(f"predictMap: unexpected arguments {sorted(kw)}")
    if predictEtaMean and predictEtaMeanField:
        raise ValueError("Hmsc.predictLatentFactor: predictMean and predictMeanField arguments cannot be simultaneously TRUE")
    from .post import poolMcmcChains
    cols = _community_columns(hM, measures, weights) if (len(measures) or weights is not None) else []
    cprobs = _community_checks(communityProbs, None)[0] if cols else []
    if not cells and not cols:
        raise ValueError("predictMap: nothing asked for (cells=False without measures or weights)")
    sprobs, qcols = _summary_probs(hM, probs) if cells else ([], None)
    hM, X, studyDesign = _new_design(hM, X, studyDesign, XData, ranLevels, Gradient)
    post = poolMcmcChains(hM.postList) if post is None else post
    X = np.asarray(hM.X if X is None else X, dtype=np.float64)
    nyN, S, ns = X.shape[0], len(post), hM.ns
    if XRRRData is not None and XRRR is not None:
        raise ValueError("Hmsc.predict: only one of XRRRData and XRRR arguments can be specified")
    ncRRR = int(hM.ncRRR or 0)
    if XRRRData is not None:
        from .model import model_matrix
        XRRR = model_matrix(hM.XRRRFormula, XRRRData)[0]
    elif XRRR is None and ncRRR > 0:
        XRRR = hM["XRRR"]
    betas = [np.asarray(s["Beta"], dtype=np.float64) for s in post]
    if ncRRR > 0:                     # folded into X and Beta as predict does
        XRRR = np.asarray(XRRR, dtype=np.float64)
        if XRRR.shape[0] != nyN:
            raise ValueError("hMsc.predict: number of rows in XRRR and X must be equal")
        ncN = hM.ncNRRR
        betas = [np.vstack([b[:ncN], np.asarray(s["wRRR"]).T @ b[ncN:]]) for b, s in zip(betas, post)]
        X = np.hstack([X, XRRR])
    studyDesign = hM.studyDesign if studyDesign is None else studyDesign
    if hM.nr > L.MAX_LEVELS:
        raise ValueError(f"predict: at most {L.MAX_LEVELS} device levels")
    levels = [_map_level(hM, r, name, studyDesign[name], post, predictEtaMean, predictEtaMeanField, gppDevice)
              for r, name in enumerate(hM.rLNames)]
    draws = (not expected) or any(lv["nn"] > 0 and lv["mode"] != 0 for lv in levels)
    if seed is None and draws:
        raise ValueError("predictMap: draws are asked for (expected=False, or new units without predictEtaMean) and "
                         "come from a Philox key: give seed")
    nslot = int(np.sum(qcols)) if (cells and sprobs) else 0
    ncol = nslot + len(cols) + sum(lv["nf"] for lv in levels)
    rows = map_slab_rows(nyN, S, ncol, slab_rows, scratch_bytes)
    for lv in levels:
        if lv["mode"] == 2 and lv["nn"] > 0:
            for sl in map_slab_plan([lv["unit"]], [lv["np"]], rows):
                if 0 < len(sl["new"][0]) < lv["nn"]:
                    raise NotImplementedError(
                        f"predictMap: the 'Full' joint draw of level {lv['name']} needs all its {lv['nn']} new units in "
                        f"one slab ({rows} rows); use predictEtaMean or predictEtaMeanField, or a larger slab_rows")
    # ---- the device call
    keep = []
    a = L.hmsc_map_args()
    a.ny, a.ns, a.nc, a.nr, a.nsamples = nyN, ns, X.shape[1], hM.nr, S
    a.expected, a.seed, a.device = (1 if expected else 0), int(seed or 0), int(device)
    a.X = L.colmajor_ptr(X, keep)
    a.Beta = L.colmajor_ptr(np.concatenate([b.reshape(-1, order="F") for b in betas]), keep)
    a.sigma = L.colmajor_ptr(np.concatenate([np.asarray(s["sigma"], dtype=np.float64).ravel() for s in post]), keep)
    a.family = L.colmajor_ptr(hM.distr[:, 0], keep, np.int32)
    a.YScalePar = L.colmajor_ptr(hM.YScalePar, keep)
    for r, lv in enumerate(levels):
        nf, npo = lv["nf"], lv["np"]
        eta = np.zeros((S, nf, npo))
        lam = np.zeros((S, ns, nf))
        for k, s in enumerate(post):
            eta[k, :lv["nfs"][k]] = np.asarray(s["Eta"][r], dtype=np.float64).T
            lam[k, :, :lv["nfs"][k]] = np.asarray(s["Lambda"][r], dtype=np.float64).T
        unit1 = np.ascontiguousarray(lv["unit"] + 1, dtype=np.int32)
        alphas, idx = np.ascontiguousarray(lv["alphas"], dtype=np.float64), np.ascontiguousarray(lv["alpha"])
        keep += [eta, lam, unit1, alphas, idx]
        m = a.level[r]
        m.np, m.nn, m.nf, m.sDim, m.G, m.mode, m.nNeighbours = npo, lv["nn"], nf, lv["sDim"], len(alphas), lv["mode"], \
            lv["nNeighbours"]
        m.unit, m.alphas, m.alpha, m.Eta, m.Lambda = L.iptr(unit1), L.fptr(alphas), L.iptr(idx), L.fptr(eta), L.fptr(lam)
        if lv["coords"] is not None:
            m.coords = L.colmajor_ptr(lv["coords"], keep)
        if lv["dist"] is not None:
            m.dist = L.colmajor_ptr(lv["dist"], keep)
        if lv["knots"] is not None:
            m.knots, m.nK = L.colmajor_ptr(lv["knots"], keep), int(lv["knots"].shape[0])
    a.cells, a.slab_rows = (1 if cells else 0), int(rows)
    a.scratch_bytes, a.factor_bytes = int(scratch_bytes), int(factor_bytes)
    o = L.hmsc_map_out()
    nq = len(sprobs)
    if cells:
        pr = np.ascontiguousarray(sprobs, dtype=np.float64)
        a.summary.nq = nq
        a.summary.probs, a.summary.qcols = (L.fptr(pr), L.iptr(qcols)) if nq else (None, None)
        mean, occ = np.empty(ns * nyN), np.empty(ns * nyN)
        n = np.empty(ns * nyN, dtype=np.int32)
        quant = np.empty(max(nq, 1) * ns * nyN)
        keep += [pr, qcols]
        o.mean, o.occ, o.n, o.quant = L.fptr(mean), L.fptr(occ), L.iptr(n), L.fptr(quant) if nq else None
    blocks = _community_blocks(cols, nyN, cprobs)       # one block per transform, as predictCommunity's calls
    for k, b in enumerate(blocks):
        b.fill(a.community[k])
        a.community[k].npairs = 0
        o.cn[k], o.cmean[k], o.cquant[k] = b.out()
    a.ncomm = len(blocks)
    L.check(L.lib().hmsc_predict_map(C.byref(a), C.byref(o)))
    del keep
    return dict(cells=_unpack_cells(mean, occ, n, quant, sprobs, ns, nyN) if cells else None,
                community=_community_gather(cols, blocks, nyN, cprobs) if cols else None)


def mapTiming():
    """hmsc_debug_map_timing of this thread's last predictMap: dict of milliseconds per phase, summed
    over the slabs."""
    t = np.zeros(9)
    L.check(L.lib().hmsc_debug_map_timing(L.fptr(t)))
    return dict(zip(("plan", "K12", "trsm", "mean", "assemble", "summary", "community", "statistics", "copy"),
                    (float(v) for v in t)))


def quantile7(x, probs):
    """R's quantile(x, probs, na.rm = TRUE) (type 7) along the last axis: h = (n - 1) p,
    lo + (h - floor h) (hi - lo) of the sorted non-NaN values.  Returns len(probs) x x.shape[:-1]."""
    x = np.asarray(x, dtype=np.float64)
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    srt = np.sort(x, axis=-1)                        # NaN last
    n = (~np.isnan(x)).sum(axis=-1)
    nn = np.maximum(n, 1)
    out = np.empty((len(probs),) + x.shape[:-1])
    for q, p in enumerate(probs):
        h = (nn - 1).astype(np.float64) * p
        fl = np.floor(h)
        g = h - fl
        k0 = fl.astype(np.int64)
        k1 = np.minimum(k0 + (g > 0), nn - 1)
        x0 = np.take_along_axis(srt, k0[..., None], axis=-1)[..., 0]
        x1 = np.take_along_axis(srt, k1[..., None], axis=-1)[..., 0]
        with np.errstate(invalid="ignore", over="ignore"):
            r = np.where(x1 != x0, x0 + g * (x1 - x0), x0)
        out[q] = np.where(n > 0, r, np.nan)
    return out


def _pr_above(last, first):
    """R's mean(last > first): NA when either holds one."""
    if np.any(np.isnan(last)) or np.any(np.isnan(first)):
        return float("nan")
    return float(np.mean(last > first))


def gradientSummary(hM, Gradient, measure, index=0, q=(0.025, 0.5, 0.975), predY=None, **kw):
    """plotGradient's numbers without the figure (R/plotGradient.R:63-138): dict(xx, lo, me, hi, Pr,
    xlabel, ylabel) for measure "S" (the summed response), "Y" (species `index`, 0-based) or "T"
    (community-weighted mean of trait `index`, 0-based).  lo, me, hi are the quantiles q[0], q[1],
    q[2] over the posterior samples at every grid point; Pr is the share of samples in which the
    last grid point lies above the first.
    With predY (the list predict(hM, Gradient=Gradient, ...) returns) it is the host restatement of
    the reference's lines.  Without it the numbers come from the device without the prediction
    array: predictCommunity(hM, Gradient=Gradient, **kw), "Y" through a unit-vector weight column;
    for one seed they are those of predict's values under that seed."""
    q = [float(p) for p in q]
    if len(q) != 3:
        raise ValueError("gradientSummary: q must hold three probabilities (lo, me, hi)")
    if measure not in ("S", "Y", "T"):
        raise ValueError(f"gradientSummary: unknown measure {measure!r}")
    xdn = Gradient["XDataNew"]
    xlabel = str(xdn.columns[0])
    xx = np.asarray(xdn.iloc[:, 0])
    ngrid = len(xx)
    fam = np.asarray(hM.distr)[:, 0]
    if measure == "S":
        ylabel = "Species richness" if np.all(fam == 2) else "Total count" if np.all(fam == 3) else "Summed response"
    elif measure == "Y":
        ylabel = str(hM.spNames[index])
    else:
        ylabel = str(hM.trNames[index])
    if predY is not None:
        A = np.stack([np.asarray(p, dtype=np.float64) for p in predY], axis=2)      # abind(predY, along = 3)
        if measure == "S":
            val = A.sum(axis=1)                                                      # lapply(predY, rowSums)
        elif measure == "Y":
            val = A[:, index, :]
        else:
            Tr = np.asarray(hM.Tr, dtype=np.float64)
            def one(a):                 # (exp(a) %*% Tr) / matrix(rep(rowSums(exp(a)), nt), ncol = nt)
                g = np.exp(a) if np.all(fam == 1) else a
                with np.errstate(invalid="ignore", divide="ignore"):
                    return (g @ Tr) / np.repeat(g.sum(axis=1)[:, None], Tr.shape[1], axis=1)
            val = np.stack([one(np.asarray(p, dtype=np.float64)) for p in predY], axis=2)[:, index, :]
        Pr = _pr_above(val[ngrid - 1], val[0])
        qp = quantile7(val, q)
    else:
        kw = dict(kw)
        kw.update(Gradient=Gradient, probs=q, contrast=(0, ngrid - 1))
        if measure == "S":
            res, col = predictCommunity(hM, measures=("S",), **kw), 0
        elif measure == "T":
            res, col = predictCommunity(hM, measures=("T",), **kw), index
        else:
            w = np.zeros(hM.ns)
            w[index] = 1.0
            res, col = predictCommunity(hM, measures=(), weights={ylabel: w}, **kw), 0
        qp = res["quantiles"][:, :, col]
        Pr = float(res["Pr"][0, col])
    return dict(xx=xx, lo=qp[0], me=qp[1], hi=qp[2], Pr=Pr, xlabel=xlabel, ylabel=ylabel)
