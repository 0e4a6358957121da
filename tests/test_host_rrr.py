"""Reduced-rank regression covariates, host side (no GPU): the Hmsc() fields of R/Hmsc.R:343-420,
the moments of the updatewRRR restatement (tests/rrr_oracle.py) against brute-force Gaussian
conditioning, and combineParameters' back-transform (R/combineParameters.R:30-43)."""
import numpy as np
import pandas as pd
import pytest

from helpers import H, rel_err
from oracle.rng import Rng
import rrr_oracle as RO


def _xy(ny=40, ns=5, ncN=3, ncORRR=4, seed=0, intercept=True):
    rng = np.random.default_rng(seed)
    cols = ([np.ones(ny)] if intercept else []) + [rng.standard_normal(ny) for _ in range(ncN - int(intercept))]
    X = np.column_stack(cols)
    XRRR = rng.standard_normal((ny, ncORRR)) * 3.0 + 2.0
    XRRR[:, 1] = (rng.random(ny) < 0.5).astype(float)      # a 0/1 column: not scaled by XRRRScale=TRUE
    Y = (rng.standard_normal((ny, ns)) > 0).astype(float)
    names = (["(Intercept)"] if intercept else ["x0"]) + [f"x{k}" for k in range(1, ncN)]
    return Y, X, XRRR, names


def test_fields_scaled_with_intercept():
    Y, X, XRRR, names = _xy()
    hM = H.Hmsc(Y=Y, X=X, covNames=names, XRRR=XRRR, ncRRR=2, distr="probit")
    assert (hM.nc, hM.ncNRRR, hM.ncRRR, hM.ncORRR) == (5, 3, 2, 4)
    assert hM.covNames == names + ["XRRR_1", "XRRR_2"]
    assert hM["XRRRNames"] == ["covRRR1", "covRRR2", "covRRR3", "covRRR4"]
    mu, sd = XRRR.mean(axis=0), XRRR.std(axis=0, ddof=1)
    mu[1], sd[1] = 0.0, 1.0                                  # the 0/1 column keeps (0, 1)  (R/Hmsc.R:403,407-411)
    assert np.allclose(hM.XRRRScalePar, np.vstack([mu, sd]), rtol=1e-14, atol=0)
    assert np.allclose(hM.XRRRScaled, (XRRR - mu) / sd, rtol=1e-13, atol=1e-15)
    assert hM.XScaled.shape == (40, 3)                       # X stays the ncNRRR plain columns
    # priors sized by the full nc (R/setPriors.Hmsc.R)
    assert hM.V0.shape == (5, 5) and hM.f0 == 6 and hM.mGamma.shape == (5,) and hM.UGamma.shape == (5, 5)
    assert (hM.nuRRR, hM.a1RRR, hM.b1RRR, hM.a2RRR, hM.b2RRR) == (3, 1, 1, 50, 1)
    H.setPriors(hM, nuRRR=4.0, a1RRR=2.0, b1RRR=3.0, a2RRR=40.0, b2RRR=1.5)
    assert (hM.nuRRR, hM.a1RRR, hM.b1RRR, hM.a2RRR, hM.b2RRR) == (4.0, 2.0, 3.0, 40.0, 1.5)


def test_fields_unscaled():
    Y, X, XRRR, names = _xy(ncORRR=12)
    hM = H.Hmsc(Y=Y, X=X, covNames=names, XRRR=XRRR, ncRRR=1, XRRRScale=False, distr="probit")
    assert (hM.nc, hM.ncNRRR, hM.ncRRR, hM.ncORRR) == (4, 3, 1, 12)
    assert np.array_equal(hM.XRRRScalePar, np.vstack([np.zeros(12), np.ones(12)]))
    assert np.array_equal(hM.XRRRScaled, XRRR)
    assert hM["XRRRNames"][0] == "covRRR01" and hM["XRRRNames"][-1] == "covRRR12"   # %.2d (R/Hmsc.R:387)
    assert hM.covNames[-1] == "XRRR_1"


def test_fields_scale_selected_columns_and_data_frame():
    Y, X, XRRR, names = _xy()
    sel = np.array([True, False, False, True])
    hM = H.Hmsc(Y=Y, X=X, covNames=names, XRRR=XRRR, ncRRR=2, XRRRScale=sel, distr="probit")
    mu, sd = XRRR.mean(axis=0), XRRR.std(axis=0, ddof=1)
    assert np.allclose(hM.XRRRScalePar[:, sel], np.vstack([mu, sd])[:, sel], rtol=1e-14)
    assert np.array_equal(hM.XRRRScalePar[:, ~sel], np.array([[0.0, 0.0], [1.0, 1.0]]))
    assert np.array_equal(hM.XRRRScaled[:, ~sel], XRRR[:, ~sel])
    df = pd.DataFrame(XRRR, columns=["a", "b", "c", "d"])
    hD = H.Hmsc(Y=Y, X=X, covNames=names, XRRRData=df, XRRRFormula="~.-1", ncRRR=2, distr="probit")
    assert hD["XRRRNames"] == ["a", "b", "c", "d"] and hD.ncORRR == 4 and hD.XRRRFormula == "~.-1"
    assert np.array_equal(hD["XRRR"], XRRR) and np.allclose(hD.XRRRScaled, (XRRR - hD.XRRRScalePar[0]) / hD.XRRRScalePar[1])


def test_no_intercept_scaling_is_refused_and_unscaled_works():
    Y, X, XRRR, names = _xy(intercept=False)
    with pytest.raises(NotImplementedError, match="bug of the reference"):
        H.Hmsc(Y=Y, X=X, covNames=names, XRRR=XRRR, ncRRR=2, distr="probit")
    hM = H.Hmsc(Y=Y, X=X, covNames=names, XRRR=XRRR, ncRRR=2, XRRRScale=False, distr="probit")
    assert hM.nc == 5 and hM.XInterceptInd is None


def test_error_messages():
    Y, X, XRRR, names = _xy()
    kw = dict(Y=Y, X=X, covNames=names, ncRRR=2, distr="probit")
    with pytest.raises(ValueError, match="XRRR must be a matrix"):
        H.Hmsc(XRRR=list(XRRR[:, 0]), **kw)
    with pytest.raises(ValueError, match="number of rows in XRRR must be equal to the number of sampling units"):
        H.Hmsc(XRRR=XRRR[:-1], **kw)
    bad = XRRR.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="XRRR must contain no NA values"):
        H.Hmsc(XRRR=bad, **kw)
    with pytest.raises(ValueError, match="XRRRData must be a data.frame"):
        H.Hmsc(XRRRData=XRRR, **kw)
    with pytest.raises(ValueError, match="number of rows in XRRRData must be equal to the number of sampling units"):
        H.Hmsc(XRRRData=pd.DataFrame(XRRR[:-1]), **kw)
    with pytest.raises(ValueError, match="XRRRData must contain no NA values"):
        H.Hmsc(XRRRData=pd.DataFrame(bad), **kw)
    with pytest.raises(ValueError, match="XRRR can't be scaled if X is not scaled"):
        H.Hmsc(XRRR=XRRR, XScale=False, **kw)
    with pytest.raises(NotImplementedError, match="XSelect") as ei:
        H.Hmsc(XSelect=[dict()], **kw)
    assert "RRR" not in str(ei.value) and "reduced" not in str(ei.value)
    plain = H.Hmsc(Y=Y, X=X, covNames=names, distr="probit")
    assert plain.ncRRR == 0 and plain.ncORRR == 0 and plain.nc == plain.ncNRRR == 3 and len(plain) == 72


def _brute(st, m):
    """Posterior precision and mean of vec(wRRR) by dense Gaussian conditioning: vec(Z) =
    D vec(wRRR) + vec(X_A BetaNRRR + sum_r LRan_r) + eps, eps ~ N(0, diag(1 / iSigma) x I), prior
    precision diag(vec(PsiRRR o tau)).  Column e = k + ncRRR c of D is vec(XRRR[, c] BetaRRR[k, ])."""
    XA, XR, Z = m["XA"], m["XRRR"], st["Z"]
    ny, ns = Z.shape
    ncN, nk, nco = XA.shape[1], m["ncRRR"], XR.shape[1]
    BetaR = st["Beta"][ncN:]
    D = np.empty((ny * ns, nk * nco))
    for c in range(nco):
        for k in range(nk):
            D[:, k + nk * c] = np.kron(BetaR[k], XR[:, c])
    W = np.kron(st["iSigma"], np.ones(ny))
    rest = XA @ st["Beta"][:ncN]
    for r in range(m["Pi"].shape[1]):
        rest = rest + st["Eta"][r][m["Pi"][:, r] - 1] @ st["Lambda"][r]
    tau = np.cumprod(st["DeltaRRR"])
    P = (D * W[:, None]).T @ D + np.diag((st["PsiRRR"] * tau[:, None]).reshape(-1, order="F"))
    mean = np.linalg.solve(P, (D * W[:, None]).T @ (Z - rest).reshape(-1, order="F"))
    return P, mean


@pytest.mark.parametrize("units", [(), (7,), (6, 21)], ids=["nr0", "nr1", "nr2"])
def test_update_wrrr_moments_match_gaussian_conditioning(units):
    hM = RO.synthetic_rrr(ny=21, ns=5, ncN=2, ncRRR=2, ncORRR=3, units=units, nf=2, seed=40 + len(units), n_normal=2)
    m = RO.rrr_model(hM)
    rng = Rng(5150)
    st = RO.compute_initial_parameters(m, rng)
    st = RO.sweep_rrr(st, m, rng, 1)           # a state with iSigma != 1 and an informed Z
    iU, _, mu = RO.wrrr_moments(st, m)
    P, mean = _brute(st, m)
    assert rel_err(iU, P) < 1e-10
    assert rel_err(mu, mean) < 1e-10
    w0 = RO.update_wrrr(st, m, rng, 2, zero_noise=True)
    assert rel_err(w0.reshape(-1, order="F"), mean) < 1e-10
    w1 = RO.update_wrrr(st, m, rng, 2)
    assert w1.shape == (2, 3) and not np.allclose(w0, w1)


def test_combine_parameters_back_transform():
    """R/combineParameters.R:30-43, including its index: component k takes XRRRScalePar[, k]."""
    from hmsc_amd.sampler import combine_parameters
    hM = RO.synthetic_rrr(ny=30, ns=4, ncN=3, ncRRR=2, ncORRR=5, seed=3)
    rng = np.random.default_rng(9)
    S, nc, ns, nt = 3, hM.nc, hM.ns, hM.nt
    A = rng.standard_normal((S, nc, nc))
    rec = dict(Beta=rng.standard_normal((S, nc, ns)), Gamma=rng.standard_normal((S, nc, nt)),
               iV=A @ A.transpose(0, 2, 1) + 3 * np.eye(nc), iSigma=rng.uniform(0.5, 2, (S, ns)),
               rho=np.ones(S, dtype=np.int32), nf=np.zeros((0, S), dtype=np.int32),
               wRRR=rng.standard_normal((S, 2, 5)), PsiRRR=rng.uniform(1, 2, (S, 2, 5)), DeltaRRR=rng.uniform(1, 2, (S, 2)))
    post = combine_parameters(rec, hM)
    for k in range(S):
        Beta, Gamma, iV = rec["Beta"][k].copy(), rec["Gamma"][k].copy(), rec["iV"][k].copy()
        for kk in range(hM.ncNRRR):
            mm, ss = hM.XScalePar[:, kk]
            if mm != 0 or ss != 1:
                Beta[kk] /= ss
                Gamma[kk] /= ss
                Beta[0] -= mm * Beta[kk]
                Gamma[0] -= mm * Gamma[kk]
                iV[kk, :] *= ss
                iV[:, kk] *= ss
        for kk in range(hM.ncRRR):
            mm, ss = hM.XRRRScalePar[:, kk]
            row = hM.ncNRRR + kk
            Beta[row] /= ss
            Gamma[row] /= ss
            Beta[0] -= mm * Beta[row]
            Gamma[0] -= mm * Gamma[row]
            iV[row, :] *= ss
            iV[:, row] *= ss
        assert rel_err(post[k]["Beta"], Beta) < 1e-14 and rel_err(post[k]["Gamma"], Gamma) < 1e-14
        assert rel_err(post[k]["V"], np.linalg.inv(iV)) < 1e-10
        assert np.array_equal(post[k]["wRRR"], rec["wRRR"][k]) and np.array_equal(post[k]["PsiRRR"], rec["PsiRRR"][k])
        assert post[k]["DeltaRRR"].shape == (2, 1) and len(post[k]) == 13
