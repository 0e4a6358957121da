"""numpy fp64 restatement of GPP kriging of latent factors at new spatial units
(R/predictLatentFactor.R:161-203) with the draws of the device's counter contract, for
tests/test_host_gpp_krige.py (pinned to the host path hmsc_amd.predict._krige) and
tests/test_gpu_gpp_krige.py (hmsc_krige's mode 4 against it).

Per sample s with nf_s factors the grid value is that of its LAST factor, a = alphas[idx[s, nf_s - 1]
- 1], for every factor (R's ag = alpha[nf]).  a = 0: out = z_new.  a > 0, in the host path's literal
`inv` form:
    Wss, W12, Wns = exp(-d / a) between knots, fitted units and knots, new units and knots
    iWss = inv(Wss); idD = 1 / (1 - rowsums((W12 iWss) o W12)); iF = inv(Wss + W12' diag(idD) W12)
    R = chol(iF) upper;  mu = iF W12' (idD o eta) + R z_knot   (covariance R R', as in R)
    out = Wns mu + sqrt(max(1 - rowsums((Wns iWss) o Wns), 0)) z_new
The clamp at 0 is the deviation from the host path, whose sqrt of a negative rounding residue (a
new unit on a knot) is NaN.  Such a unit -- its kernel entry with the knot is exactly 1 -- gets its
exact dDn = 0: the residue is +-2e-16 with either sign depending on the fp64 route (inv or
Cholesky), and its square root, 1.5e-8, would be the output's largest error term.
z_new of new unit i, factor h, sample s is Rng(seed).normal(i, h, 31 + 256 level, s); z_knot of knot k
is Rng(seed).normal(k, h, 32 + 256 level, s).
`form="chol"` is a second fp64 route (Cholesky factors and triangular solves in place of inv) used
to measure the reference's own error."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

from oracle.rng import Rng

S_KRIGE, S_KRIGE_KNOT, LEVEL_STRIDE = 31, 32, 256


def pdist(a, b):
    """Distances between the rows of a and b, the dimensions summed in index order."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def z_new(seed, level, nn, s, h):
    i = np.arange(nn, dtype=np.uint64)
    return Rng(int(seed)).normal(i, np.full(nn, h, dtype=np.uint64), S_KRIGE + LEVEL_STRIDE * level, int(s))


def z_knot(seed, level, nK, s, h):
    k = np.arange(nK, dtype=np.uint64)
    return Rng(int(seed)).normal(k, np.full(nK, h, dtype=np.uint64), S_KRIGE_KNOT + LEVEL_STRIDE * level, int(s))


def parts(a, s1, s2, sK, form="inv"):
    """What the grid value decides: dict(Wns, iF, R (upper, R'R = iF), idDW12, dDn (not clamped))."""
    Wss, W12, Wns = np.exp(-pdist(sK, sK) / a), np.exp(-pdist(s1, sK) / a), np.exp(-pdist(s2, sK) / a)
    if form == "inv":
        iWss = np.linalg.inv(Wss)
        dDn = 1 - ((Wns @ iWss) * Wns).sum(axis=1)
        idD = 1 / (1 - np.einsum("ik,kl,il->i", W12, iWss, W12))
        idDW12 = idD[:, None] * W12
        iF = np.linalg.inv(Wss + W12.T @ idDW12)
    else:
        Ls = np.linalg.cholesky(Wss)
        dDn = 1 - (solve_triangular(Ls, Wns.T, lower=True) ** 2).sum(axis=0)
        idD = 1 / (1 - (solve_triangular(Ls, W12.T, lower=True) ** 2).sum(axis=0))
        idDW12 = idD[:, None] * W12
        iF = cho_solve(cho_factor(Wss + W12.T @ idDW12, lower=True), np.eye(len(sK)))
        iF = 0.5 * (iF + iF.T)
    return dict(Wns=Wns, iF=iF, R=np.linalg.cholesky(iF).T, idDW12=idDW12, dDn=dDn)


def residual_sd(P):
    """sqrt(dDn) of the new units: clamped at 0, and exactly 0 for a unit on a knot."""
    return np.where((P["Wns"] == 1.0).any(axis=1), 0.0, np.sqrt(np.maximum(P["dDn"], 0.0)))


def last_alpha(alphas, idx_row):
    """The grid value of the sample's last factor (0-padded row of 1-based indices)."""
    nz = np.nonzero(np.asarray(idx_row))[0]
    return float(alphas[idx_row[nz[-1]] - 1]) if len(nz) else 0.0


def krige(alphas, Eta, idx, seed, s1, s2, sK, level=0, form="inv", draws=True):
    """Eta S x np x nfmax (zero padded), idx S x nfmax (1-based grid indices, 0 = no such factor).
    Output S x nn x nfmax.  draws=False leaves both z out (the conditional mean)."""
    Eta, idx = np.asarray(Eta, dtype=np.float64), np.asarray(idx)
    s1, s2, sK = (np.asarray(x, dtype=np.float64) for x in (s1, s2, sK))
    S, npo, nfmax = Eta.shape
    nn, nK = s2.shape[0], sK.shape[0]
    out = np.zeros((S, nn, nfmax))
    cache = {}
    for s in range(S):
        a = last_alpha(alphas, idx[s])
        for h in range(nfmax):
            if idx[s, h] == 0:
                continue
            zn = z_new(seed, level, nn, s, h) if draws else np.zeros(nn)
            if not a > 0:
                out[s, :, h] = zn
                continue
            if a not in cache:
                cache[a] = parts(a, s1, s2, sK, form)
            P = cache[a]
            zk = z_knot(seed, level, nK, s, h) if draws else np.zeros(nK)
            mu = P["iF"] @ P["idDW12"].T @ Eta[s, :, h] + P["R"] @ zk
            out[s, :, h] = P["Wns"] @ mu + residual_sd(P) * zn
    return out
