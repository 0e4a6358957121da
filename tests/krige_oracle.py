"""numpy fp64 restatement of the kriging of latent factors at new spatial units
(R/predictLatentFactor.R:59-160) with the draws of the device's counter contract, for
tests/test_host_krige.py (pinned to the host path hmsc_amd.predict._krige) and
tests/test_gpu_krige.py (the device path hmsc_krige against it).

Inputs of every function: the distance matrix D of the np fitted units followed by the nn new
units ((np + nn)^2; `distances` builds it from coordinates), the grid values alphas =
alphapw[:, 0], Eta (S x np x nfmax, zero padded), idx (S x nfmax 1-based grid indices, 0 = no such
factor).  Output S x nn x nfmax.  z of new unit i, factor h, sample s is
oracle.rng.Rng(seed).normal(i, h, 31 + 256 * level, s)."""
import numpy as np

from oracle.rng import Rng

S_KRIGE = 31
LEVEL_STRIDE = 256


def distances(xy):
    """dist() of the unit coordinates, the dimensions summed in index order."""
    xy = np.asarray(xy, dtype=np.float64)
    return np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))


def z_draws(seed, level, nn, s, h):
    """The N(0, 1) column of sample s, factor h over the nn new units."""
    i = np.arange(nn, dtype=np.uint64)
    return Rng(int(seed)).normal(i, np.full(nn, h, dtype=np.uint64), S_KRIGE + LEVEL_STRIDE * level, int(s))


def mean_parts(D, npo, a):
    """K11, K12, K22 = exp(-D / a) blocks (:67-73, :100-104) and the mean operator."""
    K = np.exp(-D / a)
    return K[:npo, :npo], K[:npo, npo:], K[npo:, npo:]


def krige_mean(D, npo, a, eta_col):
    """:74-77 / :105: m = K12' K11^-1 eta."""
    K11, K12, _ = mean_parts(D, npo, a)
    return K12.T @ np.linalg.solve(K11, eta_col)


def mean_field_sd(D, npo, a):
    """:80-84: sqrt(1 - colSums((L^-1 K12)^2)), L = t(chol(K11))."""
    K11, K12, _ = mean_parts(D, npo, a)
    iLK = np.linalg.solve(np.linalg.cholesky(K11), K12)
    return np.sqrt(1 - (iLK ** 2).sum(axis=0))


def full_w(D, npo, a):
    """:106-107: W = K22 - K12' K11^-1 K12."""
    K11, K12, K22 = mean_parts(D, npo, a)
    return K22 - K12.T @ np.linalg.solve(K11, K12)


def nngp_neighbours(xy, npo, k):
    """:120-122 FNN::knnx.index: the k nearest fitted units of every new unit, by distance,
    ties to the lower index (a stable sort)."""
    xy = np.asarray(xy, dtype=np.float64)
    s1, s2 = xy[:npo], xy[npo:]
    d = np.sqrt(((s2[:, None, :] - s1[None, :, :]) ** 2).sum(-1))
    ind = np.argsort(d, axis=1, kind="stable")[:, :k]
    return ind, d


def krige(mode, alphas, Eta, idx, seed, level=0, D=None, xy=None, k=10):
    """mode 0 predictMean (:62-77), 1 predictMeanField (:78-85), 2 'Full' (:95-117), 3 'NNGP'
    (:118-160); a grid value 0 gives z (:86-91, :113-115, :157-159), 0 with predictMean."""
    Eta = np.asarray(Eta, dtype=np.float64)
    idx = np.asarray(idx)
    S, npo, nfmax = Eta.shape
    if D is None:
        D = distances(xy)
    nn = D.shape[0] - npo
    out = np.zeros((S, nn, nfmax))
    if mode == 3:
        ind, dn = nngp_neighbours(xy, npo, k)
        s1 = np.asarray(xy, dtype=np.float64)[:npo]
    for s in range(S):
        for h in range(nfmax):
            if idx[s, h] == 0:
                continue
            a = alphas[idx[s, h] - 1]
            z = None if mode == 0 else z_draws(seed, level, nn, s, h)
            if not a > 0:
                out[s, :, h] = 0.0 if mode == 0 else z
            elif mode == 0:
                out[s, :, h] = krige_mean(D, npo, a, Eta[s, :, h])
            elif mode == 1:
                out[s, :, h] = krige_mean(D, npo, a, Eta[s, :, h]) + mean_field_sd(D, npo, a) * z
            elif mode == 2:
                out[s, :, h] = krige_mean(D, npo, a, Eta[s, :, h]) + np.linalg.cholesky(full_w(D, npo, a)) @ z
            else:
                m, F = np.empty(nn), np.empty(nn)
                for i in range(nn):                                         # :137-156
                    K11 = np.exp(-distances(s1[ind[i]]) / a)
                    K12 = np.exp(-dn[i, ind[i]] / a)
                    w = np.linalg.solve(K11, K12)
                    m[i] = w @ Eta[s, ind[i], h]
                    F[i] = 1 - w @ K12
                out[s, :, h] = m + np.sqrt(F) * z
    return out
