"""Batched conditional prediction with spatial 'Full' and 'GPP' levels on the device
(hmsc_predict_conditional_spatial, hmsc_amd/csrc/cond.hip) against the numpy restatement over the
oracle (tests/cond_spatial_oracle.py) on the same Philox key and iteration contract: every sample's
conditioned Eta of every level to 1e-8 relative to max |Eta|, the bound of tests/test_gpu_cond.py.
The posteriors are made up; the units sit on a jittered lattice and the alphas in use come from the
lower part of a short grid, and every fixture asserts cond(W_g) <= 1e5 for the values in use, so the
restatement's own error (about cond * 2^-53) stays far inside the bound (measured worst ratio over
the cases here: 8.2e-14).  Then repeatability, the
plain call through the new entry point, the predict / computePredictedValues plumbing
(condSpatial) and the C-level errors."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cond_spatial_oracle as CS
from helpers import H, synthetic_model
from hmsc_amd import _lib as L
from hmsc_amd._lib import HmscNativeError

P = importlib.import_module("hmsc_amd.predict")

pytestmark = pytest.mark.gpu

UP = {"GammaEta": False}
TOL = 1e-8
FAM9 = [1, 1, 3, 3, 2, 2, 2, 2, 2]


def _masks(case):
    full, fam = case["full"], case["fam"]
    mixed = np.full(full.shape, np.nan)                     # probit columns, a Poisson column on every
    mixed[:, fam == 2] = full[:, fam == 2]                  # third row, one normal column
    mixed[::3, np.nonzero(fam == 3)[0][0]] = full[::3, np.nonzero(fam == 3)[0][0]]
    mixed[:, np.nonzero(fam == 1)[0][0]] = full[:, np.nonzero(fam == 1)[0][0]]
    fold = full.copy()
    fold[:, :3] = np.nan
    rna = full.copy()
    rna[np.random.default_rng(4).random(rna.shape) < 0.3] = np.nan
    rna[7] = np.nan                                         # a site with nothing observed
    return dict(mixed=mixed, species_fold=fold, random_na=rna)


def _checked(case):
    for r, xy in case["xy"].items():
        assert CS.worst_cond(xy, case["used"][r]) <= 1e5
    return case


@pytest.fixture(scope="module")
def grouped():
    """ny = 70; level 0 spatial with 35 units of two rows and 3 factors (N = 105), level 1 plain with
    np = ny; all three families; samples of 3, 3 and 2 factors; grid index 1 (alpha = 0) in use."""
    return _checked(CS.made_up(11, 70, 9, 3, (35, 70), [(3, 2), (3, 2), (2, 2)], {0}, 3, FAM9,
                               [{0: [2, 3, 4]}, {0: [3, 1, 2]}, {0: [2, 2]}]))


@pytest.fixture(scope="module")
def second():
    """np = ny = 40, 2 factors, the spatial level listed second (after a grouped plain level)."""
    return _checked(CS.made_up(12, 40, 9, 3, (8, 40), [(2, 2), (2, 2)], {1}, 2, FAM9, [{1: [2, 3]}, {1: [4, 2]}]))


@pytest.fixture(scope="module")
def blocked():
    """np = ny = 264, 4 factors: N = 1056 crosses 1024 (the blocked routines), with a ragged 64-block."""
    return _checked(CS.made_up(13, 264, 5, 2, (264,), [(4,), (4,)], {0}, 2, [1, 3, 2, 2, 2],
                               [{0: [2, 3, 2, 4]}, {0: [3, 3, 1, 2]}]))


@pytest.fixture(scope="module")
def gpp():
    """'GPP': ny = np = 90, 9 knots on a 3 x 3 lattice, 2 factors (nK nf = 18), plus a plain grouped
    level of 15 units; grid index 1 (alpha = 0) in use.  The low-rank arrays divide by dD = 1 - diag(W12
    iW22 W21): the fixture also holds it away from 0 (no unit on a knot)."""
    case = _checked(CS.made_up(14, 90, 9, 3, (90, 15), [(2, 2), (2, 2), (1, 2)], {0}, 3, FAM9,
                               [{0: [2, 3]}, {0: [1, 3]}, {0: [4]}], method="GPP"))
    hMc = case["model"](case["full"])
    from hmsc_amd.dataparams import gpp_grid_values
    assert gpp_grid_values(hMc, 0, hMc.rL[0], case["used"][0])[0].max() <= 1e3
    return case


def _args(case, Yc):
    hMc = case["model"](Yc)
    return hMc, (case["X"], case["betas"], case["sigmas"], case["etas"], case["lams"],
                 np.asarray(hMc.Pi, dtype=np.int32), case["fam"])


def _device(case, Yc, steps, seed, **kw):
    hMc, args = _args(case, Yc)
    return hMc, P.conditional_etas_device(*args, Yc, steps, seed, spatial=CS.device_spatial(hMc, case["alphas"]), **kw)


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


def _restate(case, hMc, steps, seed):
    return CS.restate(hMc, case["betas"], case["sigmas"], case["etas"], case["lams"], case["alphas"], steps, seed)


@pytest.mark.parametrize("mask", ["mixed", "species_fold", "random_na"])
def test_full_grouped_units_match_oracle(grouped, mask):
    Yc = _masks(grouped)[mask]
    hMc, dev = _device(grouped, Yc, 2, 9177)
    _assert_parity(dev, _restate(grouped, hMc, 2, 9177))


def test_full_level_listed_second(second):
    Yc = _masks(second)["random_na"]
    hMc, dev = _device(second, Yc, 2, 31)
    _assert_parity(dev, _restate(second, hMc, 2, 31))


def test_full_across_the_blocked_boundary(blocked):
    Yc = _masks(blocked)["random_na"]
    hMc, dev = _device(blocked, Yc, 1, 5)
    _assert_parity(dev, _restate(blocked, hMc, 1, 5))


@pytest.mark.parametrize("mask", ["mixed", "random_na"])
def test_gpp_matches_oracle(gpp, mask):
    Yc = _masks(gpp)[mask]
    hMc, dev = _device(gpp, Yc, 2, 404)
    _assert_parity(dev, _restate(gpp, hMc, 2, 404))


def test_gpp_repeatable_and_chunk_independent(gpp):
    Yc = _masks(gpp)["mixed"]
    runs = [_device(gpp, Yc, 2, 3, **kw)[1] for kw in ({}, {}, dict(sample_chunk=1), dict(sample_chunk=2))]
    for other in runs[1:]:
        for k in range(3):
            for r in range(2):
                np.testing.assert_array_equal(runs[0][k][r], other[k][r])


def test_distance_matrix_equals_coordinates(second):
    """The host's distances differ from the device's in the last bit (numpy's sum of squares against
    the kernel's), so W_g differs by a few ulp (d / alpha <= 20 here) and the conditioned Eta by at
    most about cond(W_g) * 20 * 2^-52 <= 5e-10 of its size for cond <= 1e5: held to 1e-9 of max |Eta|."""
    Yc = _masks(second)["mixed"]
    hMc, args = _args(second, Yc)
    sp = CS.device_spatial(hMc, second["alphas"])
    a = P.conditional_etas_device(*args, Yc, 1, 8, spatial=sp)
    xy = sp[1].pop("coords")
    sp[1]["dist"] = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    b = P.conditional_etas_device(*args, Yc, 1, 8, spatial=sp)
    for k in range(len(a)):
        for r in range(2):
            assert np.max(np.abs(a[k][r] - b[k][r])) <= 1e-9 * np.max(np.abs(a[k][r]))


def test_repeatable_and_chunk_independent(grouped):
    Yc = _masks(grouped)["random_na"]
    runs = [_device(grouped, Yc, 2, 3, **kw)[1] for kw in ({}, {}, dict(sample_chunk=1), dict(sample_chunk=2))]
    for other in runs[1:]:
        for k in range(3):
            for r in range(2):
                np.testing.assert_array_equal(runs[0][k][r], other[k][r])


def test_blocked_chunk_independent(blocked):
    Yc = _masks(blocked)["random_na"]
    a = _device(blocked, Yc, 1, 5)[1]
    b = _device(blocked, Yc, 1, 5, sample_chunk=1)[1]
    for k in range(2):
        np.testing.assert_array_equal(a[k][0], b[k][0])


def test_plain_call_through_the_new_entry_point(grouped):
    """Without a spatial level (every entry's method 0) the new entry point is the old one, bit for bit."""
    Yc = _masks(grouped)["random_na"]
    hMc, args = _args(grouped, Yc)
    a = P.conditional_etas_device(*args, Yc, 2, 6)
    b = P.conditional_etas_device(*args, Yc, 2, 6, spatial=[None, None])
    for k in range(3):
        for r in range(2):
            np.testing.assert_array_equal(a[k][r], b[k][r])


@pytest.fixture(scope="module")
def fitted_full():
    hM = synthetic_model(ny=60, ns=7, nc=3, nf=2, nr=2, units=[30, 60], n_normal=2, n_poisson=2, seed=71, yscale=True,
                         spatial=[0], alpha_n=8)
    hM = H.sampleMcmc(hM, samples=4, transient=10, thin=1, nChains=1, updater=UP, seed=8, verbose=0)
    return hM, H.poolMcmcChains(hM.postList)


def test_predict_cond_spatial_matches_per_sample_path(fitted_full):
    """predict(Yc, condBatch=True, condSpatial=True) against condBatch=False for the same seed: same
    key, same starting Eta, same draws.  The bound (rtol 1e-6, atol 1e-8) is the plumbing bound of
    tests/test_gpu_cond.py: accuracy is held by the oracle tests above, this one catches a mis-wired
    sample, level, unit or grid index."""
    hM, post = fitted_full
    Yc = np.array(hM.Y, dtype=np.float64)
    Yc[:, :3] = np.nan
    Yc[::4, 4] = np.nan
    one = np.stack(H.predict(hM, post=post, Yc=Yc, mcmcStep=2, expected=True, seed=11), axis=2)
    bat = np.stack(H.predict(hM, post=post, Yc=Yc, mcmcStep=2, expected=True, seed=11, condBatch=True,
                             condSpatial=True), axis=2)
    print("max |condSpatial - per-sample|", np.max(np.abs(one - bat)))
    np.testing.assert_allclose(bat, one, rtol=1e-6, atol=1e-8)
    base = np.stack(H.predict(hM, post=post, expected=True, seed=11), axis=2)
    assert not np.allclose(bat, base)
    same = np.stack(H.predict(hM, post=post, Yc=np.full((hM.ny, hM.ns), np.nan), expected=True, seed=11,
                              condBatch=True, condSpatial=True), axis=2)
    np.testing.assert_array_equal(same, base)
    with pytest.raises(NotImplementedError, match="condBatch does not serve level lev0: spatial"):
        H.predict(hM, post=post, Yc=Yc, mcmcStep=2, expected=True, seed=11, condBatch=True)


def test_partition_sp_with_cond_spatial():
    """Row folds hold units out, whose coordinates predict finds by name: the level's sData is named."""
    import pandas as pd
    h0 = synthetic_model(ny=60, ns=7, nc=3, nf=2, nr=1, units=[30], n_normal=2, n_poisson=2, seed=73, spatial=[0],
                         alpha_n=8)
    r0 = h0.rL[0]
    rl = H.HmscRandomLevel(sData=pd.DataFrame(np.asarray(r0.s), index=[f"s{k:05d}" for k in range(30)]))
    H.setPriors(rl, nfMin=2, nfMax=2, alphapw=r0.alphapw)
    hM = H.Hmsc(Y=h0.Y, X=h0.X, XScale=True, distr=h0.distr, studyDesign=h0.studyDesign, ranLevels={"lev0": rl})
    hM = H.sampleMcmc(hM, samples=4, transient=10, thin=1, nChains=1, updater=UP, seed=8, verbose=0)
    part, part_sp = np.arange(hM.ny) % 2 + 1, np.arange(hM.ns) % 2 + 1
    out = H.computePredictedValues(hM, partition=part, partition_sp=part_sp, mcmcStep=1, expected=True, seed=13,
                                   nChains=1, updater=UP, condBatch=True, condSpatial=True)
    assert out.shape == (hM.ny, hM.ns, hM.samples) and np.all(np.isfinite(out))
    probit = hM.distr[:, 0] == 2
    assert np.all((out[:, probit] >= 0) & (out[:, probit] <= 1))


def test_c_level_errors(second):
    Yc = _masks(second)["mixed"]
    hMc, args = _args(second, Yc)

    def call(**change):
        sp = CS.device_spatial(hMc, second["alphas"])
        keep = []
        a = L.hmsc_cond_args()
        X, betas, sigmas, etas, lams, Pi, fam = args
        S, ny, ns = len(betas), X.shape[0], Yc.shape[1]
        a.ny, a.ns, a.nc, a.nr, a.nsamples, a.mcmcStep, a.seed = ny, ns, X.shape[1], 2, S, 1, 1
        a.X, a.Yc = L.colmajor_ptr(X, keep), L.colmajor_ptr(Yc, keep)
        a.Beta = L.fptr(P._stack(keep, [b.reshape(-1, order="F") for b in betas]))
        a.sigma = L.fptr(P._stack(keep, sigmas))
        a.family, a.Pi = L.colmajor_ptr(fam, keep, np.int32), L.colmajor_ptr(Pi, keep, np.int32)
        out = (L.dp * L.MAX_LEVELS)()
        lev = (L.hmsc_cond_spatial * L.MAX_LEVELS)()
        nps, ncls = [8, 40], [0, 0]
        for r in range(2):
            nf, stacks = P.stack_device_levels(keep, [e[r] for e in etas], [lm[r] for lm in lams])
            a.Eta[r], a.Lambda[r] = L.fptr(stacks[0][0]), L.fptr(stacks[0][1])
            o = np.empty(S * nps[r] * nf)
            keep.append(o)
            out[r] = L.fptr(o)
        cnt, ucls = P.cond_classes(~np.isnan(Yc), Pi[:, 0] - 1, 8)
        keep += [cnt, ucls]
        a.cnt[0], a.unit_class[0], ncls[0] = L.iptr(cnt), L.iptr(ucls), cnt.shape[0]
        a.np, a.nf = L.colmajor_ptr(nps, keep, np.int32), L.colmajor_ptr([2, 2], keep, np.int32)
        a.ncls = L.colmajor_ptr(ncls, keep, np.int32)
        vals, idx = P.cond_grid_in_use(sp[1]["alphapw"], sp[1]["Alpha"], 2)
        idx = change.get("idx", idx)
        keep += [vals, idx]
        q = lev[1]
        q.method, q.sDim, q.nalpha = change.get("method", 1), 2, vals.size
        q.alphas, q.AlphaIdx, q.coords = L.fptr(vals), L.iptr(idx), L.colmajor_ptr(sp[1]["coords"], keep)
        L.check(L.lib().hmsc_predict_conditional_spatial(C.byref(a), lev, out))

    call()
    with pytest.raises(HmscNativeError, match=r"spatial method 2 \(NNGP\) of level 1 is not served"):
        call(method=2)
    with pytest.raises(HmscNativeError, match="unknown spatial method 7 of level 1"):
        call(method=7)
    with pytest.raises(HmscNativeError, match="grid index 3 of sample 1, factor 0 of level 1 is outside the 3 grid"):
        call(idx=np.array([[0, 1], [3, 0]], dtype=np.int32))
    assert L.lib().hmsc_predict_conditional_spatial(C.byref(L.hmsc_cond_args()), None, (L.dp * L.MAX_LEVELS)()) == 0


def test_c_level_errors_gpp(second):
    """A 'GPP' entry on a level with grouped units, and one with nK nf > 1024."""
    Yc = _masks(second)["mixed"]
    hMc, args = _args(second, Yc)
    alpha = [[np.array([2, 3]), np.array([2, 3])] for _ in range(2)]

    def fake(npr, nK):
        return lambda vals: (np.ones((npr, len(vals))), np.zeros((npr, nK, len(vals))),
                             np.repeat(np.eye(nK)[:, :, None], len(vals), axis=2))

    lev = lambda r, npr, nK: dict(alphapw=CS.short_grid(8, 0.6), Alpha=[a[r] for a in alpha], gpp=fake(npr, nK))  # noqa: E731
    with pytest.raises(HmscNativeError, match=r"the 'GPP' level 0 needs one row per unit \(np = 8, ny = 40\)"):
        P.conditional_etas_device(*args, Yc, 1, 1, spatial=[lev(0, 8, 4), None])
    with pytest.raises(HmscNativeError, match="nK \\* nf = 1200 of the 'GPP' level 1 exceeds 1024"):
        P.conditional_etas_device(*args, Yc, 1, 1, spatial=[None, lev(1, 40, 600)])


@pytest.fixture(scope="module")
def fitted_gpp():
    hM = synthetic_model(ny=80, ns=7, nc=3, nf=2, nr=2, units=[80, 10], n_normal=2, n_poisson=2, seed=72, yscale=True,
                         spatial=[0], alpha_n=8, spatial_method="GPP", n_knots=9)
    hM = H.sampleMcmc(hM, samples=4, transient=10, thin=1, nChains=1, updater=UP, seed=9, verbose=0)
    return hM, H.poolMcmcChains(hM.postList)


def test_predict_cond_spatial_gpp_matches_per_sample_path(fitted_gpp):
    """As test_predict_cond_spatial_matches_per_sample_path, on a fitted 'GPP' model."""
    hM, post = fitted_gpp
    Yc = np.array(hM.Y, dtype=np.float64)
    Yc[:, :3] = np.nan
    Yc[::4, 4] = np.nan
    one = np.stack(H.predict(hM, post=post, Yc=Yc, mcmcStep=2, expected=True, seed=11), axis=2)
    bat = np.stack(H.predict(hM, post=post, Yc=Yc, mcmcStep=2, expected=True, seed=11, condBatch=True,
                             condSpatial=True), axis=2)
    print("max |condSpatial - per-sample| (GPP)", np.max(np.abs(one - bat)))
    np.testing.assert_allclose(bat, one, rtol=1e-6, atol=1e-8)
    base = np.stack(H.predict(hM, post=post, expected=True, seed=11), axis=2)
    assert not np.allclose(bat, base)
    same = np.stack(H.predict(hM, post=post, Yc=np.full((hM.ny, hM.ns), np.nan), expected=True, seed=11,
                              condBatch=True, condSpatial=True), axis=2)
    np.testing.assert_array_equal(same, base)
