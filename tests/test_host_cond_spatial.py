"""Host side of batched conditional prediction with spatial levels (no GPU): the restatement
(tests/cond_spatial_oracle.py over the oracle's spatial updateEta) against brute-force Gaussian
conditioning, the form of the 'GPP' step the device uses, the grid-in-use helper and the eligibility
check of predict(condBatch=True, condSpatial=True)."""
import importlib

import numpy as np
import pytest

import cond_oracle as CO
import cond_spatial_oracle as CS
from helpers import H, O, oracle_model, rel_err, synthetic_model
from oracle.rng import Rng

P = importlib.import_module("hmsc_amd.predict")


def _state(case, hMc, k=0):
    m = oracle_model(hMc)
    st = CO.sample_state(case["betas"][k], case["sigmas"][k], case["etas"][k], case["lams"][k])
    st["Alpha"] = case["alphas"][k]
    st["Z"] = O.linear_predictor(st, m)
    st["Z"] = O.update_z(st, m, Rng(5), 1)
    return m, st


def _brute_force_mean(m, st, r, W):
    """E[vec(Eta_r) | Z, everything else] by the dense joint precision: prior bdiag_h(W_h^-1) on the
    unit-fastest vec, likelihood Z_ij - L(-r)_ij ~ N(sum_h eta[Pi_i, h] lambda_hj, sigma_j) over ALL
    cells (R's spatial branches keep the NA cells, whose Z is drawn)."""
    lam, isig = st["Lambda"][r], st["iSigma"]
    nf, (ny, ns) = lam.shape[0], st["Z"].shape
    npr = int(m["np"][r])
    pi0 = m["Pi"][:, r] - 1
    S = st["Z"] - m["X"] @ st["Beta"]
    for r2 in range(m["Pi"].shape[1]):
        if r2 != r:
            S = S - O.l_ran(st, m, r2)
    A = np.zeros((ny * ns, npr * nf))                     # row (i, j), column q + np h
    for i in range(ny):
        for j in range(ns):
            for h in range(nf):
                A[i * ns + j, pi0[i] + npr * h] = lam[h, j]
    D = np.tile(isig, ny)
    Q = A.T @ (D[:, None] * A)
    for h in range(nf):
        Q[h * npr:(h + 1) * npr, h * npr:(h + 1) * npr] += np.linalg.inv(W[h])
    return np.linalg.solve(Q, A.T @ (D * S.ravel())).reshape((npr, nf), order="F")


def test_full_step_is_gaussian_conditioning():
    """12 units of two rows, 2 factors with different alphas, one of them 0, NA cells in Yc."""
    case = CS.made_up(3, 24, 5, 2, (12, 24), [(2, 2)], {0}, 1, [1, 3, 2, 2, 2], [{0: [3, 1]}])
    Yc = case["full"].copy()
    Yc[np.random.default_rng(1).random(Yc.shape) < 0.3] = np.nan
    hMc = case["model"](Yc)
    m, st = _state(case, hMc)
    got = O.update_eta(st, m, Rng(5), 2, zero_noise=True, data_par=O.compute_data_parameters(m))[0]
    xy = CS.level_coords(hMc, 0)
    d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    grid = hMc.rL[0].alphapw[:, 0]
    W = [np.eye(12) if grid[a - 1] == 0 else np.exp(-d / grid[a - 1]) for a in case["alphas"][0][0]]
    assert rel_err(got, _brute_force_mean(m, st, 0, W)) < 1e-11


@pytest.fixture(scope="module")
def gpp_case():
    case = CS.made_up(4, 30, 5, 2, (30, 6), [(2, 2)], {0}, 1, [1, 3, 2, 2, 2], [{0: [3, 1]}], method="GPP", n_knots=4)
    Yc = case["full"].copy()
    Yc[np.random.default_rng(2).random(Yc.shape) < 0.3] = np.nan
    hMc = case["model"](Yc)
    return (case, hMc) + _state(case, hMc)


def test_gpp_step_is_gaussian_conditioning(gpp_case):
    """The prior of a 'GPP' factor is W = W12 W22^-1 W21 + diag(dD) (the identity for alpha = 0)."""
    case, hMc, m, st = gpp_case
    dp = O.compute_data_parameters(m)
    got = O.update_eta(st, m, Rng(5), 2, zero_noise=True, data_par=dp)[0]
    np.testing.assert_array_equal(got, O.gpp_eta_literal(st, m, 0, _S(m, st, 0), dp)[0])
    xy, kn = CS.level_coords(hMc, 0), np.asarray(hMc.rL[0]["sKnot"])
    d12 = np.sqrt(((xy[:, None, :] - kn[None, :, :]) ** 2).sum(-1))
    d22 = np.sqrt(((kn[:, None, :] - kn[None, :, :]) ** 2).sum(-1))
    grid = hMc.rL[0].alphapw[:, 0]
    W = []
    for a in case["alphas"][0][0]:
        al = grid[a - 1]
        if al == 0:
            W.append(np.eye(30))
            continue
        W12, W22 = np.exp(-d12 / al), np.exp(-d22 / al)
        low = W12 @ np.linalg.solve(W22, W12.T)
        W.append(low + np.diag(1.0 - np.diag(low)))
    assert rel_err(got, _brute_force_mean(m, st, 0, W)) < 1e-10


def _S(m, st, r):
    S = st["Z"] - m["X"] @ st["Beta"]
    for r2 in range(m["Pi"].shape[1]):
        if r2 != r:
            S = S - O.l_ran(st, m, r2)
    return S


def test_gpp_step_in_the_device_form(gpp_case):
    """eta = iA fS + iAW L_H^-T (L_H^-1 iAW' fS + xi2) + LiA xi1 from the arrays of the values in use
    (gpp_grid_values, cond_grid_in_use) equals the oracle's step with the same normals."""
    from hmsc_amd.dataparams import gpp_grid_values
    from oracle import rng as R
    case, hMc, m, st = gpp_case
    rng, it = Rng(5), 2
    want = O.update_eta(st, m, rng, it, data_par=O.compute_data_parameters(m))[0]
    vals, idx = P.cond_grid_in_use(hMc.rL[0].alphapw, [case["alphas"][0][0]])
    idD, idDW12, F = gpp_grid_values(hMc, 0, hMc.rL[0], vals)
    lam, isig = st["Lambda"][0], st["iSigma"]
    npr, nf, nK = 30, 2, F.shape[0]
    LDL = (lam * isig[None, :]) @ lam.T
    fS = (_S(m, st, 0) @ (lam * isig[None, :]).T)                                  # np x nf (np == ny, Pi = identity)
    assert np.array_equal(m["Pi"][:, 0], np.arange(1, npr + 1))
    B1 = np.stack([np.linalg.inv(LDL + np.diag(idD[i, idx[0]])) for i in range(npr)])
    iAW = np.zeros((npr * nf, nK * nf))
    Wm = np.zeros((npr * nf, nK * nf))
    Hm = np.zeros((nK * nf, nK * nf))
    for h2 in range(nf):
        Wm[h2 * npr:(h2 + 1) * npr, h2 * nK:(h2 + 1) * nK] = idDW12[:, :, idx[0, h2]]
        Hm[h2 * nK:(h2 + 1) * nK, h2 * nK:(h2 + 1) * nK] = F[:, :, idx[0, h2]]
        for h in range(nf):
            iAW[h * npr:(h + 1) * npr, h2 * nK:(h2 + 1) * nK] = B1[:, h, h2][:, None] * idDW12[:, :, idx[0, h2]]
    LH = np.linalg.cholesky(Hm - Wm.T @ iAW)
    stream = R.S_ETA
    xi1 = rng.normal(np.arange(npr)[:, None], np.arange(nf)[None, :], stream, it)
    xi2 = rng.normal(np.arange(nK)[:, None], O.GPP_XI2_SUB + np.arange(nf)[None, :], stream, it).ravel(order="F")
    u = np.linalg.solve(LH.T, np.linalg.solve(LH, iAW.T @ fS.ravel(order="F")) + xi2)
    eta = (iAW @ u).reshape((npr, nf), order="F")
    for i in range(npr):
        eta[i] += B1[i] @ fS[i] + np.linalg.cholesky(B1[i]) @ xi1[i]
    assert rel_err(eta, want) < 1e-11


def test_grid_in_use():
    alphapw = np.column_stack([np.arange(6) * 0.1, np.full(6, 1 / 6)])
    vals, idx = P.cond_grid_in_use(alphapw, [[4, 2, 4], [6, 6, 6], [1, 2]])
    np.testing.assert_array_equal(vals, alphapw[[0, 1, 3, 5], 0])          # the grid's order, index 1 is alpha = 0
    assert idx.dtype == np.int32
    np.testing.assert_array_equal(idx, [[2, 1, 2], [3, 3, 3], [0, 1, 0]])  # the short sample is padded with 0
    vals, idx = P.cond_grid_in_use(alphapw, [[3, 3]], nf=4)
    np.testing.assert_array_equal(vals, [0.2])
    np.testing.assert_array_equal(idx, [[0, 0, 0, 0]])
    for bad in ([0, 2], [2, 7]):
        with pytest.raises(ValueError, match="level lev0 lies outside its alphapw"):
            P.cond_grid_in_use(alphapw, [bad], name="lev0")


def _fake_fitted(nf=2, **kw):
    """A model with a one-sample posterior, without a sampler run."""
    hM = synthetic_model(ny=20, ns=4, nc=2, nf=2, seed=3, **kw)
    rng = np.random.default_rng(0)
    sam = dict(Beta=rng.standard_normal((hM.nc, hM.ns)), sigma=np.ones(hM.ns),
               Eta=[rng.standard_normal((int(hM.np[0]), nf))], Lambda=[rng.standard_normal((nf, hM.ns))],
               Alpha=[np.ones(nf, dtype=np.int64)])
    return hM, [sam]


def test_check_accepts_and_refuses_by_name():
    P.cond_batch_check(*_fake_fitted(spatial=[0]), spatial=True)
    P.cond_batch_check(*_fake_fitted(spatial=[0], units=[10]), spatial=True)          # grouped 'Full' units
    P.cond_batch_check(*_fake_fitted(spatial=[0], spatial_method="GPP"), spatial=True)
    P.cond_batch_check(*_fake_fitted(), spatial=True)
    with pytest.raises(NotImplementedError, match="condSpatial does not serve level lev0: spatial method 'NNGP'"):
        P.cond_batch_check(*_fake_fitted(spatial=[0], spatial_method="NNGP", n_neighbours=3), spatial=True)
    with pytest.raises(NotImplementedError, match="lev0: 'GPP' with grouped units"):
        P.cond_batch_check(*_fake_fitted(spatial=[0], spatial_method="GPP", units=[10]), spatial=True)
    with pytest.raises(NotImplementedError, match="lev0: 'GPP' with nf > 16"):
        P.cond_batch_check(*_fake_fitted(nf=17, spatial=[0], spatial_method="GPP"), spatial=True)
    with pytest.raises(NotImplementedError, match="lev0: xData"):
        P.cond_batch_check(*_fake_fitted(x_dim=2), spatial=True)
    with pytest.raises(NotImplementedError, match="lev0: nf > 32"):
        P.cond_batch_check(*_fake_fitted(nf=33, spatial=[0]), spatial=True)


def test_refusals_reach_predict_without_the_library(monkeypatch):
    monkeypatch.setattr(P.L, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    hM, post = _fake_fitted(spatial=[0])
    Yc = np.full((hM.ny, hM.ns), np.nan)
    Yc[:, 0] = hM.Y[:, 0]
    with pytest.raises(NotImplementedError, match="condBatch does not serve level lev0: spatial"):   # today's text
        H.predict(hM, post=post, Yc=Yc, condBatch=True)
    with pytest.raises(NotImplementedError, match="condBatch does not serve level lev0: spatial"):
        P.cond_batch_check(hM, post)
    hM, post = _fake_fitted(spatial=[0], spatial_method="NNGP", n_neighbours=3)
    with pytest.raises(NotImplementedError, match="lev0: spatial method 'NNGP'"):
        H.predict(hM, post=post, Yc=Yc, condBatch=True, condSpatial=True)
    with pytest.raises(NotImplementedError, match="lev0: spatial method 'NNGP'"):
        H.computePredictedValues(_with_post(hM, post), Yc=Yc, condBatch=True, condSpatial=True)


def _with_post(hM, post):
    hM.postList = [post]
    hM.samples = 1
    return hM
