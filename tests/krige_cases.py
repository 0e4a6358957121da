"""Inputs shared by tests/test_host_krige.py and tests/test_gpu_krige.py: a spatial level over
uniform random points in the unit square, a short pooled posterior with the features the kriging
has to cope with, and the stacked form of it that tests/krige_oracle.py takes."""
import numpy as np
import pandas as pd

from helpers import H

S, NFMAX = 5, 3


def grid_indices(rl):
    """1-based alphapw indices at a = 0 and nearest to a = 0.05, 0.4 and 1.4 (the smooth end of
    the default grid of the unit square, whose step is diag / 100)."""
    a = np.asarray(rl.alphapw)[:, 0]
    return [1] + [int(np.argmin(np.abs(a - t))) + 1 for t in (0.05, 0.4, 1.4)]


def make_level(npo, nn, seed, method="Full", distmat=False, xy=None, **kw):
    """(rl, names of the fitted units, names of the new units, coordinates fitted-then-new)."""
    if xy is None:
        xy = np.random.default_rng(seed).random((npo + nn, 2))
    names = [f"p{k:04d}" for k in range(npo)]
    newn = [f"n{k:04d}" for k in range(nn)]
    rl = H.HmscRandomLevel(sData=pd.DataFrame(xy, index=names + newn), sMethod=method, **kw)
    H.setPriors(rl, nfMin=2, nfMax=NFMAX)
    if distmat:
        # the same geometry as a distance matrix, its rows in another order
        # (test_host_predict.py::test_predict_latent_factor_distmat_equals_coordinates)
        D = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
        order = np.random.default_rng(seed + 100).permutation(npo + nn)
        alln = names + newn
        rl_d = H.HmscRandomLevel(distMat=pd.DataFrame(D[np.ix_(order, order)], index=[alln[k] for k in order]),
                                 sMethod=method, **kw)
        H.setPriors(rl_d, nfMin=2, nfMax=NFMAX)
        H.setPriors(rl_d, alphapw=rl.alphapw)
        rl = rl_d
    return rl, names, newn, xy


def make_posterior(rl, npo, seed):
    """S samples of Eta (np x nf) and Alpha: sample 1 has 2 factors only; index g04 is shared by
    factors of different samples; one factor sits at grid index 1 (a = 0)."""
    g0, g005, g04, g14 = grid_indices(rl)
    alpha = [[g04, g005, g14], [g04, g0], [g14, g04, g005], [g005, g005, g04], [g14, g04, g14]]
    rng = np.random.default_rng(seed + 7)
    eta = [rng.standard_normal((npo, len(a))) for a in alpha]
    return eta, [np.array(a) for a in alpha]


def interleave(names, newn):
    """unitsPred: new units (in order) with fitted units between them."""
    up = []
    for k, n in enumerate(newn):
        up.append(n)
        if k < len(names) and k % 2 == 0:
            up.append(names[(3 * k + 1) % len(names)])
    if len(newn) == 1:
        up = [names[2]] + up + [names[0]]
    return up


def stacked(eta, alpha):
    """(Eta S x np x nfmax zero padded, idx S x nfmax with 0 for missing factors)."""
    npo = eta[0].shape[0]
    E = np.zeros((len(eta), npo, NFMAX))
    idx = np.zeros((len(eta), NFMAX), dtype=np.int64)
    for s, (e, a) in enumerate(zip(eta, alpha)):
        E[s, :, :e.shape[1]] = e
        idx[s, :len(a)] = a
    return E, idx


def lattice_tie_level(method="NNGP", k=3):
    """Fitted units on the 4 x 4 integer lattice, one new unit at the cell centre (1.5, 1.5):
    its four nearest fitted units are at exactly sqrt(0.5), so k = 3 must take the three lowest
    indices -- (1, 1), (1, 2), (2, 1) = units 5, 6, 9 in row-major order."""
    gx, gy = np.meshgrid(np.arange(4.0), np.arange(4.0), indexing="ij")
    xy = np.vstack([np.column_stack([gx.ravel(), gy.ravel()]), [[1.5, 1.5]]])
    return make_level(16, 1, 0, method=method, xy=xy, nNeighbours=k)
