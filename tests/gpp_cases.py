"""Inputs of tests/test_host_gpp_krige.py and tests/test_gpu_gpp_krige.py: a GPP level over uniform
random points in the unit square with constructKnots' knots, and a short pooled posterior on the
grid values a in {0, ~0.05, ~0.1, ~0.2} only: at a >= 0.4 two fp64 host routes already differ by
1e-10 (cond F reaches 1e5 - 2e7 and chol(iF) amplifies it), which is no reference for a 1e-9 bound;
so krige_cases.make_posterior (a ~ 1.4) is not used for mode 4."""
import numpy as np

import krige_cases as KC
from helpers import H

TARGETS = (0.05, 0.1, 0.2)
# (np, nn, nKnots): nK = 16, 25, 49 and 81 (two knot chunks of 64); nn = 1, 70, 130 cross the row tile
SHAPES = [(100, 1, 3), (100, 70, 4), (130, 130, 6), (130, 70, 8)]


def grid_indices(rl):
    """1-based alphapw indices at a = 0 and nearest to a = 0.05, 0.1 and 0.2."""
    a = np.asarray(rl.alphapw)[:, 0]
    return [1] + [int(np.argmin(np.abs(a - t))) + 1 for t in TARGETS]


def make_level(npo, nn, nKnots, seed, xy=None, sKnot=None):
    """(rl, fitted names, new names, coordinates fitted-then-new, knots)."""
    if xy is None:
        xy = np.random.default_rng(seed).random((npo + nn, 2))
    if sKnot is None:
        sKnot = H.constructKnots(xy[:npo], nKnots=nKnots)
    rl, names, newn, xy = KC.make_level(npo, nn, seed, method="GPP", xy=xy, sKnot=sKnot)
    return rl, names, newn, xy, np.asarray(rl["sKnot"], dtype=np.float64)


def make_posterior(rl, npo, seed):
    """5 samples of Eta (np x nf) and Alpha.  Sample 1 has 2 factors and its last one at a = 0 (z for
    both, although the first sits at a > 0); sample 3's first factor is at a = 0 but its last one is
    not (kriged at the last factor's a: R's ag = alpha[nf]); a ~ 0.1 is the last factor of two
    samples, so its group holds pairs of several samples."""
    g0, g05, g1, g2 = grid_indices(rl)
    alpha = [[g1, g05, g2], [g1, g0], [g2, g05, g1], [g0, g05, g1], [g05, g2, g05]]
    rng = np.random.default_rng(seed + 7)
    eta = [rng.standard_normal((npo, len(a))) for a in alpha]
    return eta, [np.array(a) for a in alpha]


def on_knot_level(seed=5, npo=100, nn=6, nKnots=4, which=(7, 18)):
    """A level whose new units 2 and 4 lie exactly on knots which[0] and which[1]."""
    xy = np.random.default_rng(seed).random((npo + nn, 2))
    sK = np.asarray(H.constructKnots(xy[:npo], nKnots=nKnots), dtype=np.float64)
    xy[npo + 2], xy[npo + 4] = sK[which[0]], sK[which[1]]
    return make_level(npo, nn, nKnots, seed, xy=xy, sKnot=sK)
