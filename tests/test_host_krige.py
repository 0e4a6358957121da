"""tests/krige_oracle.py (the restatement the device kriging is tested against) pinned to the
host path it restates, hmsc_amd.predict._krige behind predictLatentFactor
(R/predictLatentFactor.R:59-160).  No GPU and no library.  The host path draws from a numpy
generator and the restatement from Philox counters, so the stochastic modes are compared
through the quantities they are built from: a stand-in generator that returns chosen vectors
turns the host's output into its mean (z = 0), its standard deviations (z = 1) and the columns
of its Cholesky factor of W (z = e_j)."""
import numpy as np
import pytest

import krige_cases as KC
import krige_oracle as KO
from helpers import rel_err
from hmsc_amd.predict import predictLatentFactor


class FixedNormals:
    """standard_normal(n) returns the vector it was given."""

    def __init__(self, z):
        self.z = np.asarray(z, dtype=np.float64)

    def standard_normal(self, n):
        assert n == len(self.z)
        return self.z.copy()


def _new_rows(out, up, newn):
    return np.stack([out[up.index(n)] for n in newn])


def _case(npo, nn, seed, **kw):
    rl, names, newn, xy = KC.make_level(npo, nn, seed, **kw)
    eta, alpha = KC.make_posterior(rl, npo, seed)
    return rl, names, newn, xy, eta, alpha, KC.interleave(names, newn)


@pytest.mark.parametrize("distmat", [False, True])
def test_predict_mean_equals_host(distmat):
    rl, names, newn, xy, eta, alpha, up = _case(40, 9, 11, distmat=distmat)
    host = predictLatentFactor(up, names, eta, rl, predictMean=True, postAlpha=alpha)
    E, idx = KC.stacked(eta, alpha)
    ref = KO.krige(0, np.asarray(rl.alphapw)[:, 0], E, idx, seed=1, D=KO.distances(xy))
    for s in range(KC.S):
        nf = eta[s].shape[1]
        assert rel_err(ref[s][:, :nf], _new_rows(host[s], up, newn)) < 1e-12
        assert np.all(ref[s][:, nf:] == 0)
    # a = 0 (sample 1, factor 1): predictMean gives 0 on both sides
    assert np.all(_new_rows(host[1], up, newn)[:, 1] == 0) and np.all(ref[1][:, 1] == 0)


def test_mean_field_sd_and_full_w_equal_host():
    npo, nn = 40, 9
    rl, names, newn, xy, eta, alpha, up = _case(npo, nn, 12)
    D = KO.distances(xy)
    alphas = np.asarray(rl.alphapw)[:, 0]
    s, h = 0, 0                                       # a ~ 0.4
    a = alphas[alpha[s][h] - 1]
    kw = dict(postAlpha=[alpha[s]])

    def host(z, **mode):
        return _new_rows(predictLatentFactor(up, names, [eta[s]], rl, rng=FixedNormals(z), **mode, **kw)[0], up, newn)

    mean = KO.krige_mean(D, npo, a, eta[s][:, h])
    # predictMeanField: mean and standard deviation
    assert rel_err(mean, host(np.zeros(nn), predictMeanField=True)[:, h]) < 1e-12
    sd = host(np.ones(nn), predictMeanField=True)[:, h] - host(np.zeros(nn), predictMeanField=True)[:, h]
    assert rel_err(KO.mean_field_sd(D, npo, a), sd) < 1e-10
    # 'Full': mean, and W from the columns of its factor
    m0 = host(np.zeros(nn))[:, h]
    assert rel_err(mean, m0) < 1e-12
    Lw = np.column_stack([host(np.eye(nn)[j])[:, h] - m0 for j in range(nn)])
    assert np.allclose(Lw, np.tril(Lw), atol=1e-12)
    assert rel_err(KO.full_w(D, npo, a), Lw @ Lw.T) < 1e-10
    # the restatement's own draw is mean + chol(W) z with the counter contract's z
    E, idx = KC.stacked([eta[s]], [alpha[s]])
    z = KO.z_draws(5, 0, nn, 0, h)
    full = KO.krige(2, alphas, E, idx, seed=5, D=D)[0][:, h]
    assert rel_err(host(z)[:, h], full) < 1e-12
    mf = KO.krige(1, alphas, E, idx, seed=5, D=D)[0][:, h]
    assert rel_err(host(z, predictMeanField=True)[:, h], mf) < 1e-12


def test_nngp_equals_host():
    npo, nn, k = 40, 9, 5
    rl, names, newn, xy, eta, alpha, up = _case(npo, nn, 13, method="NNGP", nNeighbours=k)
    alphas = np.asarray(rl.alphapw)[:, 0]
    E, idx = KC.stacked(eta, alpha)
    ref = KO.krige(3, alphas, E, idx, seed=3, xy=xy, k=k)
    for s in range(KC.S):
        for h in range(eta[s].shape[1]):
            z = KO.z_draws(3, 0, nn, s, h)
            # the host draws factor by factor from one generator: hand it this factor's z for all
            host = predictLatentFactor(up, names, [eta[s]], rl, rng=FixedNormals(z), postAlpha=[alpha[s]])[0]
            assert rel_err(_new_rows(host, up, newn)[:, h], ref[s][:, h]) < 1e-12


def test_nngp_distance_ties_take_the_lowest_indices():
    rl, names, newn, xy = KC.lattice_tie_level(k=3)
    ind, d = KO.nngp_neighbours(xy, 16, 3)
    assert np.sum(d[0] == np.sqrt(0.5)) == 4                        # four exact ties
    assert list(ind[0]) == [5, 6, 9]                                # the three lowest indices of 5, 6, 9, 10
    # the host path uses the same three: with z = 0 its output is the mean over that neighbour
    # set, which differs from the mean over the other tied unit (10 in place of 9)
    g = KC.grid_indices(rl)[2]
    a = np.asarray(rl.alphapw)[g - 1, 0]
    eta = np.random.default_rng(0).standard_normal((16, 1))
    host = predictLatentFactor(newn, names, [eta], rl, rng=FixedNormals(np.zeros(1)), postAlpha=[np.array([g])])[0]

    def mean_over(nb):
        K11 = np.exp(-KO.distances(xy[nb]) / a)
        K12 = np.exp(-np.sqrt(((xy[16] - xy[nb]) ** 2).sum(-1)) / a)
        return np.linalg.solve(K11, K12) @ eta[nb, 0]

    assert abs(host[0, 0] - mean_over([5, 6, 9])) < 1e-12 * max(1.0, abs(host[0, 0]))
    assert abs(mean_over([5, 6, 10]) - mean_over([5, 6, 9])) > 1e-3
    # the restatement's draw over the same set
    ref = KO.krige(3, np.asarray(rl.alphapw)[:, 0], eta[None], np.array([[g]]), seed=1, xy=xy, k=3)
    z = KO.z_draws(1, 0, 1, 0, 0)
    hz = predictLatentFactor(newn, names, [eta], rl, rng=FixedNormals(z), postAlpha=[np.array([g])])[0]
    assert rel_err(hz[0, 0], ref[0, 0, 0]) < 1e-12
