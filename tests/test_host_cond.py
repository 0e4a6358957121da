"""Host side of batched conditional prediction and of species-fold cross-validation (no GPU):
the count-vector form of the unit precision and the factor-once form of the Eta step against the
oracle's updateEta (1e-12), the class finder, partition_sp's arguments, Yc and seeds, and the
eligibility check of predict(condBatch=True)."""
import importlib

import numpy as np
import pytest

import cond_oracle as CO
from helpers import H, O, oracle_model, rel_err, synthetic_model
from oracle.rng import Rng

P = importlib.import_module("hmsc_amd.predict")   # (hmsc_amd.predict the attribute is the function)


@pytest.fixture(scope="module")
def two_level():
    """Two levels (np = ny and grouped), all families, random NA plus a wholly-NA species block;
    (oracle model, state after init with Z drawn)."""
    hM = synthetic_model(ny=48, ns=9, nc=3, nf=3, nr=2, units=[48, 7], n_normal=2, n_poisson=2, na_frac=0.25, seed=5)
    Y = np.array(hM.Y, dtype=np.float64)
    Y[:, 5:7] = np.nan
    hM = H.Hmsc(Y=Y, X=hM.X, XScale=False, YScale=False, distr=hM.distr, studyDesign=hM.studyDesign,
                ranLevels={n: hM.ranLevels[n] for n in hM.rLNames})
    m = oracle_model(hM)
    rng = Rng(31)
    st = O.compute_initial_parameters(m, rng)
    st["Z"] = O.update_z(st, m, rng, 1)
    return m, st


def _classes(m, st):
    cnts, classes, factors, Qs = [], [], [], []
    obs = ~np.isnan(m["Y"])
    for r in range(m["Pi"].shape[1]):
        npr = st["Eta"][r].shape[0]
        cnt, ucls = P.cond_classes(obs, m["Pi"][:, r] - 1, npr)
        Q, F = CO.class_factors(cnt, st["Lambda"][r], st["iSigma"])
        cnts.append(cnt), classes.append(ucls), factors.append(F), Qs.append(Q)
    return cnts, classes, factors, Qs


def test_count_vector_precision_matches_oracle(two_level):
    m, st = two_level
    cnts, classes, _, Qs = _classes(m, st)
    for r in range(2):
        S = st["Z"] - m["X"] @ st["Beta"] - O.l_ran(st, m, 1 - r)
        precs, _ = O.eta_unit_moments(st, m, r, S)
        assert rel_err(Qs[r][classes[r]], precs) < 1e-12
        np.testing.assert_array_equal(cnts[r][classes[r]], CO.unit_counts(m["Y"], m["Pi"][:, r] - 1, precs.shape[0]))
    assert len(cnts[0]) > 1 and len(cnts[1]) > 1      # the NA pattern gives several classes


def test_factor_once_eta_step_matches_oracle(two_level):
    m, st = two_level
    cnts, classes, factors, _ = _classes(m, st)
    want = O.update_eta(st, m, Rng(77), 4)
    got = CO.update_eta_factored(st, m, Rng(77), 4, cnts, classes, factors)
    for r in range(2):
        assert rel_err(got[r], want[r]) < 1e-12, r


def test_class_finder_on_hand_made_masks():
    obs = np.array([[1, 1, 0], [1, 0, 0], [1, 1, 0], [0, 0, 0], [1, 0, 0]], dtype=bool)
    cnt, ucls = P.cond_classes(obs, np.arange(5), 5)               # np = ny: a class per distinct row
    assert cnt.dtype == np.int32 and ucls.dtype == np.int32
    np.testing.assert_array_equal(cnt, [[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    np.testing.assert_array_equal(ucls, [2, 1, 2, 0, 1])
    cnt, ucls = P.cond_classes(obs, np.array([0, 1, 0, 1, 2]), 3)   # grouped: counts add up
    np.testing.assert_array_equal(cnt[ucls], [[2, 2, 0], [1, 0, 0], [1, 0, 0]])
    assert cnt.shape[0] == 2
    cnt, ucls = P.cond_classes(obs, np.array([0, 0, 0, 3, 3]), 4)   # units without rows: the zero vector
    np.testing.assert_array_equal(cnt[ucls], [[3, 2, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]])
    # a species fold: whole columns NA, equal unit sizes -> one class
    obs = np.ones((12, 5), dtype=bool)
    obs[:, :2] = False
    cnt, ucls = P.cond_classes(obs, np.arange(12) % 4, 4)
    np.testing.assert_array_equal(cnt, [[0, 0, 3, 3, 3]])
    assert not ucls.any()


def _fake_fitted(**kw):
    """A model with a one-sample posterior, without a sampler run."""
    hM = synthetic_model(ny=20, ns=4, nc=2, nf=2, seed=3, **kw)
    rng = np.random.default_rng(0)
    nf = 2
    sam = dict(Beta=rng.standard_normal((hM.nc, hM.ns)), sigma=np.ones(hM.ns),
               Eta=[rng.standard_normal((int(hM.np[0]), nf))], Lambda=[rng.standard_normal((nf, hM.ns))],
               Alpha=[np.ones(nf, dtype=np.int64)])
    return hM, [sam]


def test_partition_sp_wrong_length_raises():
    hM, post = _fake_fitted()
    hM.postList = [post]
    hM.samples = 1
    with pytest.raises(ValueError, match="partition.sp"):
        H.computePredictedValues(hM, partition=np.arange(hM.ny) % 2 + 1, partition_sp=np.arange(hM.ns + 1) % 2 + 1)
    with pytest.raises(ValueError, match="partition.sp"):
        H.computePredictedValues(hM, partition_sp=[1, 2])


def test_species_fold_yc_is_what_r_builds():
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((6, 5))
    Y[1, 3] = np.nan
    part_sp = np.array([1, 2, 3, 1, 2])
    for i in (1, 2, 3):
        Yc = P.cv_sp_fold_yc(Y, part_sp, i)
        want = np.full(Y.shape, np.nan)                # R:134  Yc = matrix(NA, sum(val), ns)
        want[:, part_sp != i] = Y[:, part_sp != i]     # R:135  Yc[, train.sp] = hM$Y[val, train.sp]
        np.testing.assert_array_equal(Yc, want)
        assert np.all(np.isnan(Yc[:, part_sp == i]))
    assert Y[0, 0] == Y[0, 0]                          # the input is left alone


def test_cv_sp_fold_seed():
    seeds = {(k, i): P.cv_sp_fold_seed(13, k, i) for k in (1, 2, 3) for i in (1, 2, 3)}
    assert seeds == {(k, i): P.cv_sp_fold_seed(13, k, i) for k in (1, 2, 3) for i in (1, 2, 3)}
    assert len(set(seeds.values())) == 9
    assert not set(seeds.values()) & {P.cv_fold_seed(13, k) for k in (1, 2, 3)}
    assert P.cv_sp_fold_seed(14, 1, 1) != seeds[(1, 1)]
    assert P.cv_sp_fold_seed(None, 1, 1) is None


@pytest.mark.parametrize("kind, word", [("spatial", "spatial"), ("xdata", "xData")])
def test_cond_batch_refuses_by_name_without_the_library(monkeypatch, kind, word):
    hM, post = _fake_fitted(spatial=[0]) if kind == "spatial" else _fake_fitted(x_dim=2)
    if kind == "xdata":
        post[0]["Lambda"] = [np.zeros((2, hM.ns, 2))]

    def no_lib():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(P.L, "lib", no_lib)
    Yc = np.full((hM.ny, hM.ns), np.nan)
    Yc[:, 0] = hM.Y[:, 0]
    with pytest.raises(NotImplementedError, match=f"lev0.*{word}"):
        H.predict(hM, post=post, Yc=Yc, condBatch=True)


def test_cond_batch_refuses_wide_levels(monkeypatch):
    hM, post = _fake_fitted()
    post[0]["Eta"] = [np.zeros((int(hM.np[0]), 33))]
    post[0]["Lambda"] = [np.zeros((33, hM.ns))]
    monkeypatch.setattr(P.L, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    Yc = np.full((hM.ny, hM.ns), np.nan)
    Yc[:, 0] = hM.Y[:, 0]
    with pytest.raises(NotImplementedError, match="lev0.*nf > 32"):
        H.predict(hM, post=post, Yc=Yc, condBatch=True)
