"""numpy restatement of batched conditional prediction with spatial levels
(hmsc_predict_conditional_spatial, hmsc_amd/csrc/cond.hip) over oracle/hmsc_oracle.py: the loop of
cond_oracle.restate on the oracle model of the conditioning Hmsc (helpers.oracle_model), with the
sample's Alpha in the state and computeDataParameters' grid -- so O.update_z draws the NA cells
(R/updateZ.R:92) and O.update_eta takes R's spatial branch (R/updateEta.R:110-196).  Also the
made-up conditioning models the tests share: units on a jittered lattice and a short alphapw grid,
which keep every W_g in use well conditioned."""
import numpy as np
import pandas as pd

import cond_oracle as CO
from helpers import H, O, oracle_model
from oracle.rng import Rng


def restate(hMc, betas, sigmas, etas, lams, alphas, mcmc_step, seed):
    """[sample][level] conditioned Eta of the conditioning model hMc (Y = Yc, unscaled X);
    alphas[k][r]: the 1-based grid indices of sample k's factors of level r."""
    m = oracle_model(hMc)
    dp = O.compute_data_parameters(m)
    rng = Rng(seed)
    out = []
    for k in range(len(betas)):
        st = CO.sample_state(betas[k], sigmas[k], etas[k], lams[k])
        st["Alpha"] = [np.asarray(a, dtype=np.int64) for a in alphas[k]]
        st["Z"] = O.linear_predictor(st, m)
        it = 1 + k * (2 * mcmc_step + 1)
        st["Z"] = O.update_z(st, m, rng, it)
        for t in range(mcmc_step):
            st["Eta"] = O.update_eta(st, m, rng, it + 1 + 2 * t, data_par=dp)
            st["Z"] = O.update_z(st, m, rng, it + 2 + 2 * t)
        out.append(st["Eta"])
    return out


def level_coords(hMc, r):
    """The coordinates of level r's units in Eta's order."""
    from hmsc_amd.dataparams import _level_order
    rl = hMc.rL[r]
    return np.asarray(rl.s, dtype=np.float64)[_level_order(hMc, r, rl)]


def device_spatial(hMc, alphas):
    """conditional_etas_device's `spatial` argument for hMc and the samples' Alpha."""
    from hmsc_amd.dataparams import gpp_grid_values
    out = []
    for r, rl in enumerate(hMc.rL):
        if not rl.sDim:
            out.append(None)
            continue
        geo = (dict(gpp=lambda vals, r=r, rl=rl: gpp_grid_values(hMc, r, rl, vals)) if rl.spatialMethod == "GPP" else
               dict(coords=level_coords(hMc, r)))
        out.append(dict(alphapw=rl.alphapw, Alpha=[a[r] for a in alphas], **geo))
    return out


def lattice(n, rng, jitter=0.25):
    """n points of the unit square on a jittered lattice (spacing 1 / ceil(sqrt(n)))."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n]
    return (g + 0.5 + jitter * rng.uniform(-1, 1, (n, 2))) / side


def short_grid(alpha_n, top):
    """alphapw of alpha_n + 1 values 0 .. top with R's prior weights."""
    return np.column_stack([top * np.arange(alpha_n + 1) / alpha_n, np.r_[0.5, np.full(alpha_n, 0.5 / alpha_n)]])


def worst_cond(xy, values):
    """max over the grid values of cond(W_g), W_g = exp(-d / alpha_g) (the identity for alpha = 0)."""
    d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    return max(1.0 if a == 0 else np.linalg.cond(np.exp(-d / a)) for a in values)


def made_up(seed, ny, ns, nc, units, nfs, spatial, S, fam, alpha_used, method="Full", alpha_n=8, top=0.6, n_knots=9):
    """A conditioning setting with a made-up posterior (tests/test_gpu_cond.py::
    test_wide_models_match_oracle): units[r] units per level (rows i of unit i % units[r]), the levels
    in `spatial` spatial with lattice coordinates, nfs[k][r] factors of sample k, alpha_used[k][r] the
    1-based grid indices of a spatial level's factors.  Returns a dict: the arrays of
    conditional_etas_device, `full` (the complete Y a mask is cut from), `model(Yc)` (the
    conditioning Hmsc) and alphas."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, nc - 1))])
    fam = np.asarray(fam, dtype=np.int32)
    names, rls, xys = [f"lev{r}" for r in range(len(units))], {}, {}
    sd = {}
    for r, u in enumerate(units):
        sd[names[r]] = np.array([f"s{i % u:05d}" for i in range(ny)])
        if r in spatial:
            xys[r] = lattice(u, rng)
            kn = None
            if method == "GPP":
                side = int(round(np.sqrt(n_knots)))
                kn = (np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) + 0.5) / side
            rl = H.HmscRandomLevel(sData=pd.DataFrame(xys[r], index=[f"s{i:05d}" for i in range(u)]), sMethod=method,
                                   sKnot=kn)
            H.setPriors(rl, alphapw=short_grid(alpha_n, top))
        else:
            rl = H.HmscRandomLevel(units=sd[names[r]])
        rls[names[r]] = rl
    betas = [rng.normal(0, 0.3 / np.sqrt(nc), (nc, ns)) for _ in range(S)]
    sigmas = [np.where(fam == 2, 1.0, rng.uniform(0.5, 2.0, ns)) for _ in range(S)]
    etas = [[rng.standard_normal((u, nf)) for u, nf in zip(units, nfs[k])] for k in range(S)]
    lams = [[rng.normal(0, 0.5 / np.sqrt(nf), (nf, ns)) for nf in nfs[k]] for k in range(S)]
    alphas = [[np.asarray(alpha_used[k][r], dtype=np.int64) if r in spatial else np.ones(nfs[k][r], dtype=np.int64)
               for r in range(len(units))] for k in range(S)]
    full = np.where(fam[None, :] == 1, rng.standard_normal((ny, ns)),
                    np.where(fam[None, :] == 3, rng.poisson(1.5, (ny, ns)), rng.integers(0, 2, (ny, ns)))).astype(float)
    distr = [{1: "normal", 2: "probit", 3: "poisson"}[int(f)] for f in fam]

    def model(Yc):
        return H.Hmsc(Y=Yc, X=X, XScale=False, YScale=False, distr=distr, studyDesign=pd.DataFrame(sd), ranLevels=rls)

    used = {r: short_grid(alpha_n, top)[np.unique(np.concatenate([alpha_used[k][r] for k in range(S)])) - 1, 0]
            for r in spatial}
    return dict(X=X, betas=betas, sigmas=sigmas, etas=etas, lams=lams, fam=fam, alphas=alphas, full=full, model=model,
                xy=xys, used=used)
