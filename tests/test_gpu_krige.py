"""Kriging of new spatial units on the device (hmsc_krige, hmsc_amd/csrc/krige.hip) against
the numpy restatement tests/krige_oracle.py (itself pinned to the host path by
tests/test_host_krige.py).  Tolerances are the project's parity bounds: 1e-10 relative (normwise,
helpers.rel_err) for kriging means, 1e-9 for outputs that carry draws.  Inputs: uniform random
points in the unit square and grid values a in {0, ~0.05, ~0.4, ~1.4}; at these shapes
cond(K11) <= 4.5e4 and two host fp64 routes (solve / Cholesky + triangular solves) agree to
<= 3.7e-13 for means and draws, so the reference alone is > 100x inside the bounds."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import krige_cases as KC
import krige_oracle as KO
from helpers import H, rel_err
from hmsc_amd import _lib as L
from hmsc_amd.predict import predictLatentFactor

pytestmark = pytest.mark.gpu

SEED = 20240607
SHAPES = [(100, 1), (100, 70), (130, 130), (200, 7)]
_cache = {}


def _case(npo, nn, method="Full", distmat=False, **kw):
    key = (npo, nn, method, distmat, tuple(sorted(kw.items())))
    if key not in _cache:
        rl, names, newn, xy = KC.make_level(npo, nn, 1000 + npo + nn, method=method, distmat=distmat, **kw)
        eta, alpha = KC.make_posterior(rl, npo, npo + nn)
        _cache[key] = (rl, names, newn, xy, eta, alpha, KC.interleave(names, newn))
    return _cache[key]


def _reference(case, mode, level=0, k=10):
    rl, names, newn, xy, eta, alpha, up = case
    key = ("ref", id(case), mode, level, k)
    if key not in _cache:
        E, idx = KC.stacked(eta, alpha)
        _cache[key] = KO.krige(mode, np.asarray(rl.alphapw)[:, 0], E, idx, seed=SEED, level=level, xy=xy, k=k)
    return _cache[key]


def _device(case, level=0, **kw):
    rl, names, newn, xy, eta, alpha, up = case
    out = predictLatentFactor(up, names, eta, rl, postAlpha=alpha, device=0, seed=SEED, level=level, **kw)
    # rows of known units are the posterior Eta rows themselves
    for s, e in enumerate(out):
        assert e.shape == (len(up), eta[s].shape[1])
        for r, u in enumerate(up):
            if u in names:
                assert np.array_equal(e[r], eta[s][names.index(u)])
    return [np.stack([e[up.index(n)] for n in newn]) for e in out]


def _check(dev, ref, eta, tol):
    errs = []
    for s, d in enumerate(dev):
        nf = eta[s].shape[1]
        assert np.all(np.isfinite(d))
        errs.append(rel_err(d, ref[s][:, :nf]))
    print("rel_err per sample:", ["%.2e" % e for e in errs])
    assert max(errs) < tol


@pytest.mark.parametrize("npo,nn", SHAPES)
def test_predict_mean(npo, nn):
    case = _case(npo, nn)
    dev = _device(case, predictMean=True)
    _check(dev, _reference(case, 0), case[4], 1e-10)
    assert np.all(dev[1][:, 1] == 0)                 # the factor at a = 0


@pytest.mark.parametrize("npo,nn", SHAPES)
def test_predict_mean_field(npo, nn):
    case = _case(npo, nn)
    _check(_device(case, predictMeanField=True), _reference(case, 1), case[4], 1e-9)


@pytest.mark.parametrize("npo,nn", SHAPES)
def test_full(npo, nn):
    case = _case(npo, nn)
    _check(_device(case), _reference(case, 2), case[4], 1e-9)


def test_full_distmat_level_equals_coordinates():
    a = _device(_case(100, 70))
    b = _device(_case(100, 70, distmat=True))
    for x, y in zip(a, b):
        assert rel_err(y, x) < 1e-12
    _check(b, _reference(_case(100, 70), 2), _case(100, 70)[4], 1e-9)


@pytest.mark.parametrize("nn", [1, 9])
def test_nngp(nn):
    case = _case(40, nn, method="NNGP", nNeighbours=5)
    _check(_device(case), _reference(case, 3, k=5), case[4], 1e-9)


def test_nngp_distance_ties():
    rl, names, newn, xy = KC.lattice_tie_level(k=3)
    g = KC.grid_indices(rl)
    eta = [np.random.default_rng(0).standard_normal((16, 2))]
    alpha = [np.array([g[2], g[3]])]
    dev = predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=SEED)[0]
    ref = KO.krige(3, np.asarray(rl.alphapw)[:, 0], eta[0][None], np.array(alpha), seed=SEED, xy=xy, k=3)[0]
    assert rel_err(dev, ref) < 1e-9


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_more_pairs_on_a_grid_point_than_one_tile(mode):
    """70 samples x 2 factors, 130 of the 140 pairs on one grid point: the pairs' columns cross
    two 64-column tiles of every product (and two rounds of 64 pairs of the NNGP kernel)."""
    npo, nn, S = 70, 5, 70
    method = "NNGP" if mode == 3 else "Full"
    rl, names, newn, xy = KC.make_level(npo, nn, 77, method=method, nNeighbours=5)
    g = KC.grid_indices(rl)
    rng = np.random.default_rng(8)
    eta = [rng.standard_normal((npo, 2)) for _ in range(S)]
    alpha = [np.array([g[2], g[2]]) for _ in range(S)]
    for s in range(5):
        alpha[7 * s][s % 2] = g[1 + s % 3]
    dev = predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=SEED,
                              predictMeanField=(mode == 1))
    ref = KO.krige(mode, np.asarray(rl.alphapw)[:, 0], np.stack(eta), np.stack(alpha), seed=SEED, xy=xy, k=5)
    assert rel_err(np.stack(dev), ref) < 1e-9


def test_draws_repeat_and_follow_the_counters():
    case = _case(100, 70)
    a, b = _device(case), _device(case)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))           # bit-equal
    c = _device(case, level=1)
    assert all(not np.array_equal(x, y) for x, y in zip(a, c))
    _check(c, _reference(case, 2, level=1), case[4], 1e-9)
    # sample 1, factor 1 sits at a = 0: the output is z of the contract itself
    for lev, out in ((0, a), (1, c)):
        z = KO.z_draws(SEED, lev, 70, 1, 1)
        assert np.max(np.abs(out[1][:, 1] - z)) < 1e-12 * np.max(np.abs(z))


def test_non_spatial_level_draws_from_the_contract():
    rl = H.HmscRandomLevel(units=["a", "b", "c"])
    post = [np.arange(6.0).reshape(3, 2), 10 + np.arange(9.0).reshape(3, 3)]
    out = predictLatentFactor(["b", "z", "a", "y"], ["a", "b", "c"], post, rl, device=0, seed=SEED, level=2)
    assert np.array_equal(out[0][0], post[0][1]) and np.array_equal(out[1][2], post[1][0])
    for s, nf in ((0, 2), (1, 3)):
        for h in range(nf):
            z = KO.z_draws(SEED, 2, 2, s, h)
            assert np.max(np.abs(out[s][[1, 3], h] - z)) < 1e-12 * np.max(np.abs(z))
    mean = predictLatentFactor(["b", "z"], ["a", "b", "c"], post, rl, predictMean=True, device=0, seed=SEED)
    assert np.all(mean[0][1] == 0)


def _raw_args(npo=20, nn=3, **kw):
    xy = np.random.default_rng(2).random((npo + nn, 2))
    keep = [np.ascontiguousarray(xy.T.ravel()), np.array([0.0, 0.3, 0.9]),
            np.random.default_rng(3).standard_normal(2 * 2 * npo), np.array([[2, 3], [3, 2]], dtype=np.int32)]
    a = L.hmsc_krige_args()
    a.device, a.np, a.nn, a.sDim, a.G, a.S, a.nfmax, a.mode, a.nNeighbours, a.level = 0, npo, nn, 2, 3, 2, 2, 2, 5, 0
    a.seed = 1
    a.coords, a.alphas, a.Eta, a.alpha = L.fptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2]), L.iptr(keep[3])
    for k, v in kw.items():
        setattr(a, k, v)
    return a, keep, np.zeros(2 * 2 * nn)


def _error_of(a, out):
    rc = L.lib().hmsc_krige(C.byref(a), L.fptr(out))
    return rc, L.lib().hmsc_last_error().decode()


def test_refusals_by_name():
    a, keep, out = _raw_args()
    assert _error_of(a, out)[0] == 0                                 # the plain call is fine
    a, keep, out = _raw_args(mode=3, nNeighbours=33)
    rc, msg = _error_of(a, out)
    assert rc != 0 and "nNeighbours <= 32" in msg
    a, keep, out = _raw_args(mode=3)
    D = np.ascontiguousarray(KO.distances(np.random.default_rng(2).random((23, 2))).ravel())
    a.coords, a.dist = None, L.fptr(D)
    rc, msg = _error_of(a, out)
    assert rc != 0 and "needs coordinates" in msg
    a, keep, out = _raw_args()
    keep[3][1, 0] = 4                                                # G = 3
    rc, msg = _error_of(a, out)
    assert rc != 0 and "grid index 4" in msg and "outside the alphapw grid" in msg
    # Python side: NNGP on a distMat level, GPP with a device
    rl, names, newn, xy = KC.make_level(25, 2, 4, method="NNGP", distmat=True, nNeighbours=5)
    eta, alpha = KC.make_posterior(rl, 25, 4)
    with pytest.raises(ValueError, match="needs coordinates"):
        predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=1)
    xyg = np.random.default_rng(5).random((27, 2))
    rlg = H.HmscRandomLevel(sData=pd.DataFrame(xyg, index=names + newn), sMethod="GPP",
                            sKnot=H.constructKnots(xyg[:25], nKnots=4))
    H.setPriors(rlg, nfMin=2, nfMax=KC.NFMAX)
    with pytest.raises(NotImplementedError, match="GPP kriging on the device"):
        predictLatentFactor(newn, names, eta, rlg, postAlpha=alpha, device=0, seed=1)


def test_indefinite_w_is_refused():
    """Two new units at identical coordinates: W = K22 - K12' K11^-1 K12 is singular, R's chol stops."""
    xy = np.random.default_rng(6).random((32, 2))
    xy[31] = xy[30]
    rl, names, newn, _ = KC.make_level(30, 2, 0, xy=xy)
    eta, alpha = KC.make_posterior(rl, 30, 6)
    with pytest.raises(L.HmscNativeError, match="W = K22 - K12' K11\\^-1 K12 of the new units is not positive definite"):
        predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=1)
    # the means do not need W
    out = predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=1, predictMean=True)
    assert all(np.array_equal(e[0], e[1]) for e in out)


# ---- end to end ------------------------------------------------------------------------

def _fitted_full_model():
    if "e2e" not in _cache:
        ny, ns = 60, 5
        rng = np.random.default_rng(3)
        xy = rng.random((ny + 6, 2))
        names = [f"s{k:03d}" for k in range(ny + 6)]
        field = np.sin(4 * xy[:, 0]) + np.cos(3 * xy[:, 1])
        X = np.column_stack([np.ones(ny), rng.standard_normal(ny)])
        lam = rng.standard_normal(ns)
        Lp = X @ rng.normal(0, 0.5, (2, ns)) + field[:ny, None] * lam[None, :]
        Y = (Lp + rng.standard_normal((ny, ns)) > 0).astype(float)
        rl = H.HmscRandomLevel(sData=pd.DataFrame(xy, index=names), sMethod="Full")
        H.setPriors(rl, nfMin=2, nfMax=2)
        hM = H.Hmsc(Y=Y, X=X, covNames=["(Intercept)", "x1"], distr="probit",
                    studyDesign=pd.DataFrame({"plot": names[:ny]}), ranLevels={"plot": rl})
        hM = H.sampleMcmc(hM, samples=8, transient=10, thin=1, nChains=1, seed=9, verbose=0)
        _cache["e2e"] = (hM, names)
    return _cache["e2e"]


def test_predict_kriged_on_the_device_equals_host():
    hM, names = _fitted_full_model()
    post = H.poolMcmcChains(hM.postList)
    sd = pd.DataFrame({"plot": names[-6:] + names[:2]})
    Xn = np.column_stack([np.ones(8), np.linspace(-1, 1, 8)])
    kw = dict(post=post, X=Xn, studyDesign=sd, expected=True, seed=4)
    host = np.stack(H.predict(hM, predictEtaMean=True, **kw))
    dev = np.stack(H.predict(hM, predictEtaMean=True, krigeDevice=True, **kw))
    assert host.shape == (8, 8, hM.ns)
    assert rel_err(dev, host) < 1e-8                                  # predictMean: no randomness
    a = np.stack(H.predict(hM, krigeDevice=True, **kw))
    b = np.stack(H.predict(hM, krigeDevice=True, **kw))
    assert np.array_equal(a, b) and not np.array_equal(a, dev)
    assert np.all((a >= 0) & (a <= 1))


def test_conditional_prediction_takes_the_option():
    """predict(Yc=..., krigeDevice=True) routes the conditional chain's starting Eta through the
    device path too; at the fitted units there is nothing to krige or draw, so the result is the
    host path's bit for bit."""
    hM, names = _fitted_full_model()
    post = H.poolMcmcChains(hM.postList)[:3]
    Yc = hM.Y.copy()
    Yc[::2, :2] = np.nan
    a = np.stack(H.predict(hM, post=post, Yc=Yc, expected=True, seed=11))
    b = np.stack(H.predict(hM, post=post, Yc=Yc, expected=True, seed=11, krigeDevice=True))
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def test_spatial_cross_validation_with_device_kriging():
    hM, names = _fitted_full_model()
    partition = (np.arange(hM.ny) >= hM.ny // 2).astype(int)          # two blocks of units
    pred = H.computePredictedValues(hM, partition=partition, seed=5, krigeDevice=True)
    assert pred.shape == (hM.ny, hM.ns, 8)
    assert np.all(np.isfinite(pred)) and np.all((pred >= 0) & (pred <= 1))
