"""numpy restatement of batched conditional prediction (hmsc_predict_conditional,
hmsc_amd/csrc/cond.hip) over oracle/hmsc_oracle.py: per sample Z = L, updateZ given Yc, then
mcmcStep x (updateEta, updateZ) with Beta, sigma and Lambda fixed (R/predict.R:181-198), on the
call's iteration contract; and the two forms the device relies on -- the unit precision from its
count vector, and the Eta step from a factor computed once -- next to the oracle's own."""
import numpy as np

from helpers import O
from oracle import rng as R
from oracle.rng import Rng


def cond_model(X, Pi, distr, Yc):
    """The oracle model of the conditioning chain: (Yc, X) in R's unscaled space, plain levels."""
    Pi = np.asarray(Pi).reshape(np.asarray(X).shape[0], -1)
    d = np.asarray(distr)
    d = np.column_stack([d, np.zeros_like(d)]) if d.ndim == 1 else d   # (family, variance flag)
    return dict(X=np.asarray(X, dtype=np.float64), Y=np.asarray(Yc, dtype=np.float64), Pi=Pi, distr=d,
                rL=[dict(sDim=0, xDim=0) for _ in range(Pi.shape[1])])


def sample_state(beta, sigma, etas, lams):
    return dict(Beta=np.asarray(beta, dtype=np.float64), iSigma=1.0 / np.asarray(sigma, dtype=np.float64),
                Eta=[np.asarray(e, dtype=np.float64) for e in etas],
                Lambda=[np.asarray(lm, dtype=np.float64) for lm in lams])


def restate(X, betas, sigmas, etas, lams, Pi, distr, Yc, mcmc_step, seed):
    """[sample][level] conditioned Eta.  Sample k uses the iterations it0 = 1 + k (2 mcmcStep + 1):
    Z at it0, then for step t Eta at it0 + 1 + 2 t and Z at it0 + 2 + 2 t, all under the key `seed`
    (the loop of tests/test_gpu_predict.py::test_conditional_prediction_matches_oracle)."""
    m = cond_model(X, Pi, distr, Yc)
    rng = Rng(seed)
    out = []
    for k in range(len(betas)):
        st = sample_state(betas[k], sigmas[k], etas[k], lams[k])
        st["Z"] = O.linear_predictor(st, m)
        it = 1 + k * (2 * mcmc_step + 1)
        st["Z"] = O.update_z(st, m, rng, it)
        for t in range(mcmc_step):
            st["Eta"] = O.update_eta(st, m, rng, it + 1 + 2 * t)
            st["Z"] = O.update_z(st, m, rng, it + 2 + 2 * t)
        out.append(st["Eta"])
    return out


def unit_counts(Yc, pi0, npr):
    """c[q, j]: the number of rows of unit q in which species j is observed."""
    c = np.zeros((npr, Yc.shape[1]), dtype=np.int64)
    np.add.at(c, pi0, (~np.isnan(Yc)).astype(np.int64))
    return c


def class_factors(cnt, lam, isig):
    """Per class c: Q_c = I + sum_j cnt[c, j] isigma_j lambda_j lambda_j' and its lower Cholesky factor."""
    nf = lam.shape[0]
    Q = np.stack([np.eye(nf) + (lam * (c * isig)[None, :]) @ lam.T for c in cnt])
    return Q, np.linalg.cholesky(Q)


def update_eta_factored(st, model, rng, it, cnts, classes, factors):
    """updateEta as the device takes it: level by level, b_q = sum over the unit's rows and the
    observed species of isigma_j lambda_j (Z_ij - L(-r)_ij), eta_q = F^-T (F^-1 b_q + xi_q) with the
    factor F of the unit's class (class_factors, computed once for the whole mcmcStep loop)."""
    nr = model["Pi"].shape[1]
    st = dict(st)
    Eta = list(st["Eta"])
    Yx = ~np.isnan(model["Y"])
    for r in range(nr):
        st["Eta"] = Eta
        Lm = model["X"] @ st["Beta"]
        for r2 in range(nr):
            if r2 != r:
                Lm = Lm + O.l_ran(st, model, r2)
        lam, isig = st["Lambda"][r], st["iSigma"]
        pi0 = model["Pi"][:, r] - 1
        npr, nf = Eta[r].shape[0], lam.shape[0]
        W = np.where(Yx, st["Z"] - Lm, 0.0) * isig[None, :]
        b = np.zeros((npr, nf))
        np.add.at(b, pi0, W @ lam.T)
        xi = rng.normal(np.arange(npr)[:, None], np.arange(nf)[None, :], R.S_ETA + R.LEVEL_STRIDE * r, it)
        new = np.empty((npr, nf))
        for q in range(npr):
            F = factors[r][classes[r][q]]
            y = np.linalg.solve(F, b[q]) + xi[q]
            new[q] = np.linalg.solve(F.T, y)
        Eta[r] = new
    return Eta


def device_inputs(hM, post, X=None, betas=None):
    """The arguments of hmsc_amd.predict.conditional_etas_device / restate for a fitted model
    predicted at its own study design (no new units): per-sample Beta, sigma, Eta, Lambda."""
    X = np.asarray(hM.X if X is None else X, dtype=np.float64)
    betas = [np.asarray(s["Beta"], dtype=np.float64) for s in post] if betas is None else betas
    sigmas = [np.asarray(s["sigma"], dtype=np.float64) for s in post]
    etas = [[np.asarray(e, dtype=np.float64) for e in s["Eta"]] for s in post]
    lams = [[np.asarray(lm, dtype=np.float64) for lm in s["Lambda"]] for s in post]
    return X, betas, sigmas, etas, lams, np.asarray(hM.Pi, dtype=np.int32), hM.distr[:, 0].astype(np.int32)
