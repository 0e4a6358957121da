"""The reference the predict kernel is held to (tests/predict_reference.py), checked on the host:
it equals the oracle's restatement of R/predict.R:143-229, its error bound holds for a plain
double-precision evaluation, and the oracle's Poisson sampler -- which the device's counts are
compared with -- draws from a Poisson law on both sides of its lam < 10 switch."""
import numpy as np
import pytest

import predict_reference as PR
from helpers import O
from oracle.rng import Rng


def _post(inp):
    return [dict(Beta=inp["Beta"][s], sigma=inp["sigma"][s], Eta=[e[s] for e in inp["Eta"]],
                 Lambda=[lm[s] for lm in inp["Lambda"]]) for s in range(len(inp["Beta"]))]


@pytest.mark.parametrize("expected", [True, False])
def test_reference_equals_oracle_predict_samples(expected):
    """70 x 37, 3 samples, two levels (np < ny and np = ny), families cycling normal / probit /
    Poisson with a YScalePar on the normal columns: every cell of the extended-precision reference
    within 1e-12 relative of oracle.predict_samples (counts and indicators: equal)."""
    ny, ns, seed = 70, 37, 4321
    fam = 1 + np.arange(ns) % 3
    ysp = np.vstack([np.where(fam == 1, 0.7, 0.0), np.where(fam == 1, 1.9, 1.0)])
    inp = PR.build_inputs(ny, ns, 3, (2, 2), seed=3, np_mode=("lt", "eq"), family=fam,
                          sigma=0.5 + np.arange(ns) % 4, yscale=ysp)
    assert inp["np"] == [24, 70]
    ref = PR.reference(inp, expected, seed)["out"]
    o = np.stack(O.predict_samples(inp["X"], _post(inp), inp["Pi"], fam, ysp, expected, Rng(seed)))
    assert ref.shape == o.shape == (3, ny, ns)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(ref == o, 0.0, np.abs(ref - o) / np.abs(o))
    k = np.unravel_index(np.argmax(err), err.shape)
    print(f"expected={expected}: worst relative difference {err[k]:.3e} at (s, i, j) = {k}, family {fam[k[2]]}")
    assert err[k] <= 1e-12
    if not expected:
        disc = fam != 1
        assert np.array_equal(ref[:, :, disc], o[:, :, disc])


def test_bound_holds_for_a_double_evaluation():
    """At K = 128 (nc = 64, nf = 32, 31, 1) numpy's double-precision L lies within K 2^-53 A of
    L_ref in every cell, and not all of the bound is slack."""
    inp = PR.build_inputs(130, 65, 64, (32, 31, 1), seed=11)
    assert inp["K"] == 128
    Lr, A = PR.linear_predictor(inp)
    ratio = 0.0
    for s in range(3):
        a, b = PR._design(inp, s)
        ratio = max(ratio, float(np.max(np.abs((a @ b).astype(np.longdouble) - Lr[s]) / (128 * PR.U * A[s]))))
    print(f"double-precision L: worst |L - L_ref| / (K u A) = {ratio:.3f}")
    assert 1e-4 < ratio <= 1.0


def test_oracle_poisson_sampler_is_poisson():
    """20000 draws per rate on either side of the lam < 10 switch and up to 1e12: chi-square
    goodness of fit against scipy.stats.poisson, p >= 0.01 in every column."""
    counts = PR.oracle_poisson_counts()
    assert np.all(counts >= 0) and np.all(counts == np.round(counts))
    ps = []
    for j, lam in enumerate(PR.poisson_rates()):
        p, stat, nb = PR.poisson_gof_pvalue(counts[:, j], lam)
        print(f"lambda = {PR.POIS_LAMBDAS[j]:g}: chi2 = {stat:.1f} on {nb} bins, p = {p:.4f}")
        ps.append(p)
    assert min(ps) >= 0.01, ps


def test_goodness_of_fit_sees_a_wrong_rate():
    """The test above can fail: numpy's Poisson counts at 1.1 lambda are rejected, those at lambda
    are not."""
    g = np.random.default_rng(1)
    for lam in (1.0, 30.0, 1e6):
        assert PR.poisson_gof_pvalue(g.poisson(1.1 * lam, PR.POIS_NY), lam)[0] < 1e-3
        assert PR.poisson_gof_pvalue(g.poisson(lam, PR.POIS_NY), lam)[0] > 1e-3


def test_non_finite_rates():
    """R's rpois gives NaN for a NaN or infinite mean and 0 for mean 0; _rpois_ptrs likewise, and
    it never raises."""
    rng = Rng(5)
    assert np.isnan(O._rpois_ptrs(float("inf"), rng, 3, 0))
    assert np.isnan(O._rpois_ptrs(float("nan"), rng, 3, 0))
    assert O._rpois_ptrs(0.0, rng, 3, 0) == 0.0
    assert O._rpois_ptrs(float(np.exp(-800.0)), rng, 3, 0) == 0.0
