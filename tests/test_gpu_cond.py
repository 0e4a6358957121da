"""Batched conditional prediction on the device (hmsc_predict_conditional, hmsc_amd/csrc/cond.hip)
against the numpy restatement (tests/cond_oracle.py over oracle/hmsc_oracle.py) on the same Philox
key and iteration contract: every sample's conditioned Eta of every level to 1e-8 relative to
max |Eta|, the bound tests/test_gpu_predict.py::test_conditional_prediction_matches_oracle holds
the per-sample path to.  Then repeatability, the predict / computePredictedValues plumbing
(condBatch, partition_sp), reduced-rank regression models and the C-level errors."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cond_oracle as CO
import rrr_oracle as RO
from helpers import H, synthetic_model
from hmsc_amd import _lib as L
from hmsc_amd._lib import HmscNativeError

P = importlib.import_module("hmsc_amd.predict")

pytestmark = pytest.mark.gpu

UP = {"GammaEta": False}
TOL = 1e-8


def _fit(**kw):
    hM = synthetic_model(**kw)
    return H.sampleMcmc(hM, samples=4, transient=10, thin=1, nChains=1, updater=UP, seed=5, verbose=0)


@pytest.fixture(scope="module")
def fitted():
    """ny = 90: a 64-site tile plus a ragged one; ns = 9: two species quads plus one species (the
    16-wide MFMA tiles of E ragged); units 90 (np = ny) and 15 (grouped); all families."""
    hM = _fit(ny=90, ns=9, nc=3, nf=2, nr=2, units=[90, 15], n_normal=2, n_poisson=3, seed=61, yscale=True)
    return hM, H.poolMcmcChains(hM.postList)[:3]


@pytest.fixture(scope="module")
def fitted37():
    """ns = 37 crosses the 32-species tile of the Z launch (and K = 3 + 3 + 3 = 9 > 8 takes the
    second operand depth)."""
    hM = _fit(ny=70, ns=37, nc=3, nf=3, nr=2, units=[70, 10], n_normal=3, n_poisson=4, n_lognormal=2, seed=62,
              yscale=True)
    return hM, H.poolMcmcChains(hM.postList)[:3]


def _mixed_yc(hM):
    """Probit columns observed, one Poisson column on every third row, one normal column, the rest NA."""
    fam = hM.distr[:, 0]
    probit, pois, normal = (np.nonzero(fam == f)[0] for f in (2, 3, 1))
    Yc = np.full((hM.ny, hM.ns), np.nan)
    Yc[:, probit] = hM.Y[:, probit]
    Yc[::3, pois[0]] = hM.Y[::3, pois[0]]
    Yc[:, normal[0]] = hM.Y[:, normal[0]]
    return Yc


def _species_fold_yc(hM):
    Yc = np.array(hM.Y, dtype=np.float64)
    Yc[:, :3] = np.nan
    return Yc


def _random_na_yc(hM):
    Yc = np.array(hM.Y, dtype=np.float64)
    Yc[np.random.default_rng(4).random(Yc.shape) < 0.3] = np.nan
    Yc[7] = np.nan                     # a site, hence a unit of the np = ny level, with nothing observed
    return Yc


def _assert_parity(dev, ora):
    assert len(dev) == len(ora)
    worst = 0.0
    for k, (d, o) in enumerate(zip(dev, ora)):
        for r, (dr, orr) in enumerate(zip(d, o)):
            assert dr.shape == orr.shape
            e = np.max(np.abs(dr - orr)) / np.max(np.abs(orr))
            worst = max(worst, e)
            assert e < TOL, (k, r, e)
    print("max relative Eta error", worst)


@pytest.mark.parametrize("mask", ["mixed", "species_fold", "random_na"])
def test_matches_oracle_step_by_step(fitted, mask):
    hM, post = fitted
    Yc = dict(mixed=_mixed_yc, species_fold=_species_fold_yc, random_na=_random_na_yc)[mask](hM)
    args = CO.device_inputs(hM, post)
    dev = P.conditional_etas_device(*args, Yc, 2, 9177)
    _assert_parity(dev, CO.restate(*args, Yc, 2, 9177))
    if mask == "species_fold":         # whole columns NA, equal unit sizes: one class per level
        for r in range(2):
            assert P.cond_classes(~np.isnan(Yc), hM.Pi[:, r] - 1, int(hM.np[r]))[0].shape[0] == 1


@pytest.mark.parametrize("mask", ["mixed", "random_na"])
def test_matches_oracle_across_the_species_tile(fitted37, mask):
    hM, post = fitted37
    Yc = dict(mixed=_mixed_yc, random_na=_random_na_yc)[mask](hM)
    args = CO.device_inputs(hM, post)
    dev = P.conditional_etas_device(*args, Yc, 2, 52)
    _assert_parity(dev, CO.restate(*args, Yc, 2, 52))


def test_repeatable_and_chunk_independent(fitted):
    hM, post = fitted
    Yc = _random_na_yc(hM)
    args = CO.device_inputs(hM, post)
    a = P.conditional_etas_device(*args, Yc, 2, 3)
    b = P.conditional_etas_device(*args, Yc, 2, 3)
    c = P.conditional_etas_device(*args, Yc, 2, 3, sample_chunk=1)
    d = P.conditional_etas_device(*args, Yc, 2, 3, sample_chunk=2)
    for k in range(len(post)):
        for r in range(hM.nr):
            np.testing.assert_array_equal(a[k][r], b[k][r])
            np.testing.assert_array_equal(a[k][r], c[k][r])
            np.testing.assert_array_equal(a[k][r], d[k][r])
    t = np.zeros(4)
    L.check(L.lib().hmsc_debug_cond_timing(L.fptr(t)))
    assert np.all(t >= 0) and t[1] > 0 and t[2] > 0


def test_predict_cond_batch_matches_per_sample_path(fitted):
    """predict(Yc, condBatch=True) against condBatch=False (the per-sample path) for the same seed:
    same key, same starting Eta, same draws.  The bound (rtol 1e-6, atol 1e-8) is loose on purpose:
    accuracy is held by the oracle tests above, this one catches a mis-wired sample, level or unit
    index, which gives O(1) differences.  Measured maximum absolute difference of the expected
    values on this model: 3.0e-12."""
    hM, post = fitted
    Yc = _mixed_yc(hM)
    one = np.stack(H.predict(hM, post=post, Yc=Yc, mcmcStep=3, expected=True, seed=11), axis=2)
    bat = np.stack(H.predict(hM, post=post, Yc=Yc, mcmcStep=3, expected=True, seed=11, condBatch=True), axis=2)
    print("max |condBatch - per-sample|", np.max(np.abs(one - bat)))
    np.testing.assert_allclose(bat, one, rtol=1e-6, atol=1e-8)
    base = np.stack(H.predict(hM, post=post, expected=True, seed=11), axis=2)
    assert not np.allclose(bat, base)
    same = np.stack(H.predict(hM, post=post, Yc=np.full((hM.ny, hM.ns), np.nan), expected=True, seed=11,
                              condBatch=True), axis=2)
    np.testing.assert_array_equal(same, base)


def test_all_na_returns_the_input_eta(fitted):
    hM, post = fitted
    args = CO.device_inputs(hM, post)
    out = P.conditional_etas_device(*args, np.full((hM.ny, hM.ns), np.nan), 2, 1)
    for k in range(len(post)):
        for r in range(hM.nr):
            np.testing.assert_array_equal(out[k][r], args[3][k][r])


@pytest.mark.parametrize("nc, nfs", [(3, (20, 12)), (40, (32, 30))])
def test_wide_models_match_oracle(nc, nfs):
    """K = nc + sum(nf) = 35 and 102: the two deeper operand depths of the Z launch (K <= 64, K <=
    128) and the 16- and 32-factor forms of the Eta launch, on a made-up two-sample posterior."""
    rng = np.random.default_rng(nc)
    ny, ns, S, units = 70, 10, 2, (70, 9)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, nc - 1))])
    fam = np.array([1, 1, 3, 3, 2, 2, 2, 2, 2, 2], dtype=np.int32)
    Pi = np.column_stack([np.arange(ny) % u + 1 for u in units]).astype(np.int32)
    betas = [rng.normal(0, 0.3 / np.sqrt(nc), (nc, ns)) for _ in range(S)]
    sigmas = [rng.uniform(0.5, 2.0, ns) for _ in range(S)]
    etas = [[rng.standard_normal((u, nf)) for u, nf in zip(units, nfs)] for _ in range(S)]
    lams = [[rng.normal(0, 0.5 / np.sqrt(nf), (nf, ns)) for nf in nfs] for _ in range(S)]
    Yc = np.where(fam[None, :] == 1, rng.standard_normal((ny, ns)),
                  np.where(fam[None, :] == 3, rng.poisson(1.5, (ny, ns)), rng.integers(0, 2, (ny, ns)))).astype(float)
    Yc[rng.random((ny, ns)) < 0.2] = np.nan
    args = (X, betas, sigmas, etas, lams, Pi, fam)
    dev = P.conditional_etas_device(*args, Yc, 2, 808)
    _assert_parity(dev, CO.restate(*args, Yc, 2, 808))


def test_rrr_model():
    """A reduced-rank regression model: the call takes the [X, XRRR] design and the per-sample
    stacked rbind(BetaNRRR, t(wRRR) BetaRRR); the per-sample path still refuses."""
    hM = RO.synthetic_rrr(ny=90, ns=8, ncN=2, ncRRR=2, ncORRR=4, units=(15,), n_normal=3, seed=6)
    out = H.sampleMcmc(hM, samples=4, transient=4, nChains=1, seed=2, verbose=0)
    post = H.poolMcmcChains(out.postList)[:3]
    Yc = np.array(hM.Y, dtype=np.float64)
    Yc[:, 5:] = np.nan
    ncN = out.ncNRRR
    Xa = np.hstack([np.asarray(hM.X, dtype=np.float64), hM["XRRR"]])
    betas = [np.vstack([s["Beta"][:ncN], np.asarray(s["wRRR"]).T @ s["Beta"][ncN:]]) for s in post]
    rng = np.random.default_rng(21)
    dev = P._conditional_etas_batched(out, post, Xa, betas, hM.studyDesign, Yc, 2, rng, 0)
    key = int(np.random.default_rng(21).integers(1, 2 ** 62))
    args = CO.device_inputs(out, post, X=Xa, betas=betas)
    _assert_parity(dev, CO.restate(*args, Yc, 2, key))
    pred = H.predict(out, post=post, Yc=Yc, mcmcStep=2, expected=True, seed=21, condBatch=True)
    assert len(pred) == 3 and np.all(np.isfinite(np.stack(pred)))
    with pytest.raises(NotImplementedError, match="reduced-rank"):
        H.predict(out, post=post, Yc=Yc, mcmcStep=2, expected=True, seed=21)


@pytest.fixture(scope="module")
def cv_model():
    hM = synthetic_model(ny=60, ns=7, nc=3, nf=2, nr=1, n_normal=2, n_poisson=2, seed=71, yscale=True)
    return H.sampleMcmc(hM, samples=4, transient=4, thin=1, nChains=1, updater=UP, seed=8, verbose=0)


@pytest.mark.parametrize("cond_batch", [False, True])
def test_partition_sp(cv_model, cond_batch):
    """2 row folds x 3 species folds: shape, finiteness, and one (k, i) block bit for bit against
    predict called by hand on the fold's refit with that fold's Yc and seed."""
    hM = cv_model
    part, part_sp, seed = np.arange(hM.ny) % 2 + 1, np.arange(hM.ns) % 3 + 1, 13
    full = H.computePredictedValues(hM, partition=part, partition_sp=part_sp, mcmcStep=2, expected=True, seed=seed,
                                    nChains=1, updater=UP, condBatch=cond_batch)
    assert full.shape == (hM.ny, hM.ns, hM.samples) and np.all(np.isfinite(full))
    k, i = 2, 3
    train, val, val_sp = part != k, part == k, part_sp == i
    dev = P._cv_refit(hM, train, k, seed, 1, UP, None, 1)
    sdv = hM.studyDesign.loc[val].reset_index(drop=True)
    pv = np.stack(H.predict(dev, post=H.poolMcmcChains(dev.postList), X=hM.X[val], studyDesign=sdv,
                            Yc=P.cv_sp_fold_yc(hM.Y[val], part_sp, i), mcmcStep=2, expected=True,
                            seed=P.cv_sp_fold_seed(seed, k, i), condBatch=cond_batch), axis=2)
    np.testing.assert_array_equal(full[val][:, val_sp], pv[:, val_sp])
    # without a row partition it is ignored, as in R
    a = H.computePredictedValues(hM, partition_sp=part_sp, expected=True, seed=3)
    np.testing.assert_array_equal(a, H.computePredictedValues(hM, expected=True, seed=3))


def test_c_level_errors(fitted):
    hM, post = fitted
    X, betas, sigmas, etas, lams, Pi, fam = CO.device_inputs(hM, post)
    Yc = _mixed_yc(hM)
    bad = Pi.copy()
    bad[5, 1] = int(hM.np[1]) + 1
    with pytest.raises(HmscNativeError, match="Pi out of range"):
        P.conditional_etas_device(X, betas, sigmas, etas, lams, bad, fam, Yc, 1, 1)
    wide_e = [[np.zeros((e[0].shape[0], 33)), e[1]] for e in etas]
    wide_l = [[np.zeros((33, hM.ns)), lm[1]] for lm in lams]
    with pytest.raises(HmscNativeError, match="nf = 33 of level 0 exceeds 32"):
        P.conditional_etas_device(X, betas, sigmas, wide_e, wide_l, Pi, fam, Yc, 1, 1)
    sig = [s.copy() for s in sigmas]
    sig[1][2] = np.inf
    with pytest.raises(HmscNativeError, match="sigma of sample 1, species 2"):
        P.conditional_etas_device(X, betas, sig, etas, lams, Pi, fam, Yc, 1, 1)
    a = L.hmsc_cond_args()                       # nsamples = 0 returns before anything is read
    assert L.lib().hmsc_predict_conditional(C.byref(a), (L.dp * L.MAX_LEVELS)()) == 0
