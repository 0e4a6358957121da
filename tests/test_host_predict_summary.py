"""The numpy restatement of the posterior predictive summaries (tests/summary_reference.py) against
numpy's own nanmean / nanquantile, evaluateModelFit's summary route against its array route, and
the argument refusals that are raised before any device call.  Runs without a GPU."""
import numpy as np
import pytest

import summary_reference as SR
from helpers import H, synthetic_model


def _random_stack(seed, ny=23, ns=7, S=41, nan_share=0.2):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((ny, ns, S)) * rng.uniform(0.1, 50.0, (1, ns, 1)) + rng.uniform(-5, 5, (1, ns, 1))
    A[rng.random(A.shape) < nan_share] = np.nan
    A[0, 0, :] = np.nan                    # a cell with no value at all
    A[1, 0, 1:] = np.nan                   # and one with a single value
    return A


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_against_numpy(seed):
    """mean within n 2^-53 mean|x| of np.nanmean; type-7 quantiles within 2 ulp of max(|lo|, |hi|) of
    np.nanquantile (numpy's default method is R's type 7); n, occ and the n = 0 cell."""
    A = _random_stack(seed)
    probs = (0.0, 0.025, 0.25, 0.5, 0.9, 0.975, 1.0)
    r = SR.summarise(A, probs)
    with np.errstate(all="ignore"), pytest.warns(RuntimeWarning):
        nm = np.nanmean(A, axis=2)
        nq = np.nanquantile(A, probs, axis=2)
    ok = r["n"] > 0
    assert not ok[0, 0] and r["n"][1, 0] == 1 and ok.sum() == ok.size - 1
    assert np.array_equal(r["n"], (~np.isnan(A)).sum(axis=2))
    assert np.all(np.abs(r["mean"] - nm)[ok] <= SR.mean_bound(A)[ok])
    assert np.isnan(r["mean"][0, 0]) and np.isnan(r["occ"][0, 0]) and np.all(np.isnan(r["quantiles"][:, 0, 0]))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(r["occ"][ok], (np.nansum(A > 0, axis=2) / r["n"])[ok])
    scale = np.maximum(np.abs(r["lo"]), np.abs(r["hi"]))
    err = np.abs(r["quantiles"] - nq)
    assert np.all(err[:, ok] <= 2 * np.spacing(scale[:, ok]))
    assert np.all(r["quantiles"][:, 1, 0] == A[1, 0, 0])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(r["quantiles"][0][ok], np.fmin.reduce(A, axis=2)[ok])
        assert np.array_equal(r["quantiles"][-1][ok], np.fmax.reduce(A, axis=2)[ok])


def test_restatement_flags_columns_and_ties():
    """Unflagged columns are NaN; heavy ties (0 / 1 values) and S = 1 select exactly."""
    rng = np.random.default_rng(5)
    A = (rng.random((6, 4, 9)) < 0.4).astype(np.float64)
    r = SR.summarise(A, (0.5, 0.975), qcols=[1, 0, 1, 0])
    assert np.all(np.isnan(r["quantiles"][:, :, [1, 3]]))
    assert np.array_equal(r["quantiles"][0][:, [0, 2]], np.median(A, axis=2)[:, [0, 2]])
    assert np.array_equal(r["occ"], A.mean(axis=2))
    one = SR.summarise(A[:, :, :1], (0.025, 0.5, 0.975))
    assert np.array_equal(one["quantiles"], np.broadcast_to(A[None, :, :, 0], (3, 6, 4)))
    assert np.array_equal(one["mean"], A[:, :, 0])


@pytest.fixture(scope="module")
def model():
    hM = synthetic_model(ny=60, ns=9, nc=3, nf=2, nr=1, units=[60], n_normal=3, n_poisson=3, seed=8)
    rng = np.random.default_rng(3)
    Y = np.array(hM.Y, dtype=np.float64)
    Y[rng.random(Y.shape) < 0.1] = np.nan
    hM.Y = Y
    return hM


def _compare_fit(hM, A):
    fam = hM.distr[:, 0]
    with np.errstate(all="ignore"):
        ref = H.evaluateModelFit(hM, A)
        got = H.evaluateModelFit(hM, summary=SR.as_summary(A, fam))
    assert set(ref) == set(got) and {"RMSE", "R2", "AUC", "TjurR2", "SR2", "O.AUC", "O.TjurR2", "O.RMSE", "C.SR2",
                                     "C.RMSE"} <= set(ref)
    for key in ref:
        assert np.array_equal(np.isnan(ref[key]), np.isnan(got[key])), key
        ok = ~np.isnan(ref[key])
        assert ok.any(), key
        assert np.all(np.abs(ref[key][ok] - got[key][ok]) <= 1e-12), (key, ref[key], got[key])


@pytest.mark.parametrize("integer_poisson", [True, False], ids=["integer", "real"])
def test_model_fit_from_summary_equals_model_fit_from_array(model, integer_poisson):
    """evaluateModelFit(summary = reference summary of A) against evaluateModelFit(A) on a random
    mixed-family array with NA in Y: every key to 1e-12 with the same NaN pattern; the Poisson block
    once all-integer (draws), once real-valued (expected values)."""
    hM = model
    fam = hM.distr[:, 0]
    rng = np.random.default_rng(17 + integer_poisson)
    S = 24
    A = rng.standard_normal((hM.ny, hM.ns, S)) + rng.standard_normal((hM.ny, hM.ns, 1))
    A[:, fam == 2, :] = rng.random((hM.ny, int((fam == 2).sum()), S))
    lam = np.exp(rng.standard_normal((hM.ny, int((fam == 3).sum()), 1)))
    A[:, fam == 3, :] = rng.poisson(lam, (hM.ny, lam.shape[1], S)) if integer_poisson else lam * rng.random((1, 1, S))
    _compare_fit(hM, A)


def test_refusals_before_any_device_call(model, monkeypatch):
    """Both or neither of predY and summary; more than 8 probs; a probability outside [0, 1]: each a
    ValueError, with the device library never asked for."""
    from hmsc_amd import _lib

    def no_device():
        raise AssertionError("the device library was loaded")
    monkeypatch.setattr(_lib, "lib", no_device)
    hM = model
    A = np.zeros((hM.ny, hM.ns, 2))
    sm = SR.as_summary(A, hM.distr[:, 0])
    with pytest.raises(ValueError, match="exactly one"):
        H.evaluateModelFit(hM)
    with pytest.raises(ValueError, match="exactly one"):
        H.evaluateModelFit(hM, A, summary=sm)
    post = [dict()]
    with pytest.raises(ValueError, match="at most 8"):
        H.predictSummary(hM, post=post, probs=np.linspace(0.1, 0.9, 9))
    with pytest.raises(ValueError, match="at most 8"):        # 8 given, 0.5 added for the Poisson columns
        H.predictSummary(hM, post=post, probs=np.linspace(0.1, 0.45, 8))
    for bad in (-0.01, 1.5, np.nan):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            H.predictSummary(hM, post=post, probs=(0.5, bad))
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            H.computePredictedValues(hM, summary=True, probs=(bad,))
