"""Reduced-rank regression covariates on the device: updatewRRR, updatewRRRPriors, their initial
draws and the refresh of everything derived from the design matrix, against the numpy
restatement (tests/rrr_oracle.py over oracle/hmsc_oracle.py) on the same state and Philox key.
Tolerances are the project's: draws 1e-9, conditional moments 1e-10, three sweeps 1e-7."""
import numpy as np
import pandas as pd
import pytest
from scipy import stats

from helpers import H, O, phylo_corr, rel_err, synthetic_model
from hmsc_amd._lib import HmscNativeError
from oracle.rng import Rng
import rrr_oracle as RO

pytestmark = pytest.mark.gpu

TOL_MOMENT = 1e-10
TOL_DRAW = 1e-9
TOL_SWEEPS = 1e-7
UP = {"GammaEta": False}

# the updatewRRR Z pass' tile (hmsc_amd/csrc/rrr.hip RRR_TS sites x RRR_SC species per workgroup;
# test_tile_constants holds these to the library's)
RRR_TS, RRR_SC = 256, 64

MODELS = {
    "nr0": dict(ny=130, ns=9, ncN=2, ncRRR=1, ncORRR=1, seed=1),
    "nr1_probit": dict(ny=203, ns=22, ncN=3, ncRRR=2, ncORRR=5, units=(50,), seed=2),
    "nr2_mixed": dict(ny=257, ns=37, ncN=3, ncRRR=3, ncORRR=17, units=(40, 257), na_frac=0.05, n_normal=8,
                      n_poisson=9, seed=3),
    # two full site tiles and two full species chunks of the Z pass plus a ragged remainder of
    # each; ns = 135 is not a multiple of 4
    "wide": dict(ny=2 * RRR_TS + 37, ns=2 * RRR_SC + 7, ncN=2, ncRRR=2, ncORRR=3, units=(30,), seed=4),
}
# The chain seed.  updateGamma2 evaluates R's formulas literally (R/updateGamma2.R:37-50), which
# cancel (XZT - XX iP XZT, V0 - ...) and lose digits in proportion to X'X over iV; the RRR
# columns XRRR wRRR^T are not scaled, so at many states the reference's own draw moves by 1e-9
# to 1e-6 (relative) when X is perturbed by one ulp -- a draw parity of 1e-9 then says nothing
# about the code.  The seed is therefore chosen by the reference alone: the first of 1, 2, 3, ...
# for which that ulp perturbation moves the numpy oracle's Gamma2 draw by less than 1e-10 (a tenth
# of the draw tolerance) at the state test_updaters_after_wrrr_see_the_new_design uses, in every
# model (seeds 1 .. 25: 2e-10 .. 1e-6 in the "wide" or "nr1_probit" model; 26: 2.8e-11, 8.4e-12,
# 1.1e-13 in "wide", "nr1_probit", "nr0").
SEED = 26


@pytest.fixture(scope="module", params=list(MODELS))
def setup(request):
    """(name, hM, model factory, state): the oracle's state after init and two sweeps, computed
    once per model and left unchanged; model() returns an oracle model whose design matrix is
    that state's."""
    hM = RO.synthetic_rrr(**MODELS[request.param])
    base = RO.rrr_model(hM)
    rng = Rng(SEED)
    st = RO.compute_initial_parameters(base, rng)
    for it in (1, 2):
        st = RO.sweep_rrr(st, base, rng, it, updater=UP)

    def model(w=None):
        m = dict(base)
        RO.set_design(m, st["wRRR"] if w is None else w)
        return m
    return request.param, hM, model, st


def _chain(hM, st=None, seed=SEED):
    ch = H.Chain(hM, seed, device=0, updater=UP)
    ch.init()
    if st is not None:
        ch.set_state(st)
    return ch


def test_tile_constants():
    hM = RO.synthetic_rrr(**MODELS["nr0"])
    ch = H.Chain(hM, 1, device=0, updater=UP)
    assert list(ch.debug_get("rrr_tiles", 2)) == [RRR_TS, RRR_SC]
    ch.close()


def test_init_parity(setup):
    name, hM, model, _ = setup
    ch = _chain(hM)
    g = ch.get_state()
    X = ch.debug_get("X", hM.ny * hM.nc).reshape(hM.nc, hM.ny).T
    ch.close()
    m = model()
    o = RO.compute_initial_parameters(m, Rng(SEED))
    for k in ("DeltaRRR", "PsiRRR", "wRRR", "Gamma", "iV", "Beta", "iSigma", "Z"):
        assert rel_err(g[k], o[k]) < TOL_DRAW, (name, k, rel_err(g[k], o[k]))
    for r in range(hM.nr):
        for k in ("Eta", "Lambda", "Psi", "Delta"):
            assert rel_err(g[k][r], o[k][r]) < TOL_DRAW, (name, k, r)
    assert rel_err(X, m["X"]) < TOL_DRAW     # X = [XScaled, XRRR wRRR^T]  (R/computeInitialParameters.R:27-50)


def test_wrrr_draw_parity_and_design_refresh(setup):
    name, hM, model, st = setup
    ch = _chain(hM, st)
    ch.update("wRRR", 7)
    g = ch.get_state()
    X = ch.debug_get("X", hM.ny * hM.nc).reshape(hM.nc, hM.ny).T
    XX = ch.debug_get("XX", hM.nc * hM.nc).reshape(hM.nc, hM.nc).T
    ch.close()
    w = RO.update_wrrr(st, model(), Rng(SEED), 7)
    assert rel_err(g["wRRR"], w) < TOL_DRAW, (name, rel_err(g["wRRR"], w))
    Xo = RO.set_design(model(), w)
    assert rel_err(X, Xo) < TOL_DRAW and rel_err(XX, Xo.T @ Xo) < TOL_DRAW


def test_wrrr_priors_draw_parity(setup):
    name, hM, model, st = setup
    ch = _chain(hM, st)
    ch.update("wRRRPriors", 7)
    g = ch.get_state()
    ch.close()
    psi, delta = RO.update_wrrr_priors(st, model(), Rng(SEED), 7)
    assert rel_err(g["PsiRRR"], psi) < TOL_DRAW and rel_err(g["DeltaRRR"], delta) < TOL_DRAW
    assert rel_err(g["wRRR"], st["wRRR"]) == 0.0


def test_wrrr_conditional_mean(setup):
    name, hM, model, st = setup
    ch = _chain(hM, st)
    ch.set_noise_mode(1)
    ch.update("wRRR", 3)
    g = ch.get_state()
    ch.close()
    w = RO.update_wrrr(st, model(), Rng(SEED), 3, zero_noise=True)
    assert rel_err(g["wRRR"], w) < TOL_MOMENT, (name, rel_err(g["wRRR"], w))


@pytest.mark.parametrize("upd", ["Gamma2", "BetaLambda", "Eta", "Z"])
def test_updaters_after_wrrr_see_the_new_design(setup, upd):
    """Every buffer derived from X (XX and Gamma2's prep, XEta and its Gram, XZ) follows a wRRR
    update: the next updater's draw equals the oracle's on the refreshed design matrix."""
    name, hM, model, st = setup
    ch = _chain(hM, st)
    ch.update("wRRR", 7)
    w = ch.get_state(with_z=False)["wRRR"]
    ch.update(upd, 8)
    g = ch.get_state()
    ch.close()
    assert rel_err(w, RO.update_wrrr(st, model(), Rng(SEED), 7)) < TOL_DRAW
    m = model(w)
    s2 = dict(st, wRRR=w)
    rng = Rng(SEED)
    if upd == "Gamma2":
        assert rel_err(g["Gamma"], O.update_gamma2(s2, m, rng, 8)) < TOL_DRAW
    elif upd == "BetaLambda":
        B, Lam = O.update_beta_lambda(s2, m, rng, 8)
        assert rel_err(g["Beta"], B) < TOL_DRAW, (name, rel_err(g["Beta"], B))
        for r in range(hM.nr):
            assert rel_err(g["Lambda"][r], Lam[r]) < TOL_DRAW
    elif upd == "Eta":
        Eta = O.update_eta(s2, m, rng, 8)
        for r in range(hM.nr):
            assert rel_err(g["Eta"][r], Eta[r]) < TOL_DRAW, (name, r, rel_err(g["Eta"][r], Eta[r]))
    else:
        Z = O.update_z(s2, m, rng, 8)
        assert rel_err(g["Z"], Z) < TOL_DRAW, (name, rel_err(g["Z"], Z))


def test_three_sweeps_track_oracle(setup):
    name, hM, model, st = setup
    ch = _chain(hM, st)
    m, rng, o = model(), Rng(SEED), st
    for it in range(10, 13):
        ch.sweep(it)
        o = RO.sweep_rrr(o, m, rng, it, updater=UP)
    g = ch.get_state()
    ch.close()
    for k in ("Beta", "Gamma", "iV", "Z", "wRRR", "PsiRRR", "DeltaRRR"):
        assert rel_err(g[k], o[k]) < TOL_SWEEPS, (name, k, rel_err(g[k], o[k]))


def test_graph_replay_matches_eager(setup, monkeypatch):
    """run() replays the captured unfused sweep (updatewRRR and updatewRRRPriors inside it) bit for
    bit like eager launches, every sweep recorded, with the RRR fields in the record."""
    name, hM, _, _ = setup
    out = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("HMSC_NO_GRAPH", no_graph)
        monkeypatch.setenv("HMSC_GRAPH_SWEEPS", "4")
        ch = H.Chain(hM, 77, device=0, updater=UP)
        ch.init()
        rec = ch.run(transient=0, samples=11, thin=1, adaptNf=[0] * max(1, hM.nr))
        built = ch.debug_get("graph", 4)
        ch.close()
        assert bool(built[0]) == (no_graph == "0") and bool(built[1]) == (no_graph == "0")
        out.append(rec)
    keys = ["Beta", "Gamma", "iV", "iSigma", "wRRR", "PsiRRR", "DeltaRRR"]
    for r in range(hM.nr):
        keys += [f"Lambda{r}", f"Eta{r}", f"Psi{r}", f"Delta{r}"]
    for k in keys:
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
    assert out[0]["wRRR"].shape == (11, hM.ncRRR, hM.ncORRR) and out[0]["DeltaRRR"].shape == (11, hM.ncRRR)
    assert np.all(np.isfinite(out[0]["wRRR"])) and np.all(out[0]["PsiRRR"] > 0) and np.all(out[0]["DeltaRRR"] > 0)
    assert np.any(out[0]["wRRR"][0] != out[0]["wRRR"][-1])


def test_refusals():
    hM = RO.synthetic_rrr(**MODELS["nr1_probit"])
    with pytest.raises(HmscNativeError, match="species-sharded"):
        H.Chain(hM, 1, device=0, updater=UP, host_allreduce=lambda x: None)
    with pytest.raises(HmscNativeError, match="updateGammaEta"):
        H.Chain(hM, 1, device=0)                         # every updater on: the GammaEta bit
    hP = RO.synthetic_rrr(**MODELS["nr1_probit"])
    hP.C = phylo_corr(hP.ns)
    with pytest.raises(HmscNativeError, match="phylogeny"):
        H.Chain(hP, 1, device=0, updater=UP)
    rng = np.random.default_rng(0)
    ny, ns = 60, 6
    pi = np.arange(ny) % 12
    names = np.array([f"s{k:05d}" for k in pi])
    rl = H.HmscRandomLevel(sData=rng.random((12, 2)))
    H.setPriors(rl, nfMin=2, nfMax=2)
    hS = H.Hmsc(Y=(rng.standard_normal((ny, ns)) > 0).astype(float),
                X=np.column_stack([np.ones(ny), rng.standard_normal(ny)]), covNames=["(Intercept)", "x1"],
                XRRR=rng.standard_normal((ny, 3)), ncRRR=1, distr="probit",
                studyDesign=pd.DataFrame({"lev0": names}), ranLevels={"lev0": rl})
    with pytest.raises(HmscNativeError, match="spatial"):
        H.Chain(hS, 1, device=0, updater=UP)
    big = RO.synthetic_rrr(ny=40, ns=4, ncN=2, ncRRR=4, ncORRR=65, seed=9)     # 260 > the cap of 256
    with pytest.raises(HmscNativeError, match="ncRRR \\* ncORRR <= 256"):
        H.Chain(big, 1, device=0, updater=UP)


def test_plain_chain_is_unchanged():
    """A model without XRRR: the RRR bits are ignored, its record carries no RRR arrays and its
    posterior samples keep wRRR = PsiRRR = DeltaRRR = None."""
    hM = synthetic_model(ny=80, ns=10, nc=3, nf=2, seed=5)
    ch = H.Chain(hM, 3, device=0, updater=UP)
    ch.init()
    before = ch.get_state()
    ch.update("wRRR", 1)
    ch.update("wRRRPriors", 1)
    after = ch.get_state()
    rec = ch.run(transient=1, samples=3, adaptNf=[0])
    ch.close()
    for k in ("Beta", "Gamma", "iV", "Z"):
        assert np.array_equal(before[k], after[k])
    assert "wRRR" not in before and "wRRR" not in rec and "PsiRRR" not in rec
    out = H.sampleMcmc(hM, samples=3, transient=2, updater=UP, seed=1, verbose=0)
    s = out.postList[0][0]
    assert s["wRRR"] is None and s["PsiRRR"] is None and s["DeltaRRR"] is None and len(s) == 13


def test_sample_mcmc_and_predict(capsys):
    """sampleMcmc end to end on an RRR model (GammaEta switched off with a message), then
    predict(expected=True) against R/predict.R:144-153 evaluated directly in numpy."""
    hM = RO.synthetic_rrr(ny=90, ns=8, ncN=2, ncRRR=2, ncORRR=4, units=(15,), n_normal=3, seed=6)
    out = H.sampleMcmc(hM, samples=6, transient=4, nChains=2, seed=2, verbose=0)
    assert "Setting updater$GammaEta=FALSE due to reduced rank regression" in capsys.readouterr().out
    s = out.postList[1][3]
    assert s["wRRR"].shape == (2, 4) and s["PsiRRR"].shape == (2, 4) and s["DeltaRRR"].shape == (2, 1)
    assert s["Beta"].shape == (4, 8) and s["V"].shape == (4, 4) and len(s) == 13
    post = H.poolMcmcChains(out.postList)
    rng = np.random.default_rng(3)
    Xn, XRn = np.column_stack([np.ones(20), rng.standard_normal(20)]), rng.standard_normal((20, 4))
    sdn = pd.DataFrame({"lev0": np.asarray(hM.studyDesign["lev0"])[:20]})
    pred = H.predict(out, post=post, X=Xn, XRRR=XRn, studyDesign=sdn, expected=True, seed=1)
    from hmsc_amd.model import _factor_levels
    units = [str(u) for u in _factor_levels(hM.studyDesign["lev0"])]
    upred = [str(u) for u in _factor_levels(sdn["lev0"])]
    for k in (0, len(post) - 1):
        sam = post[k]
        X1 = np.hstack([Xn, XRn @ sam["wRRR"].T])                                   # :145,151
        eta = sam["Eta"][0][[units.index(u) for u in upred]]
        Lp = X1 @ sam["Beta"] + eta[[upred.index(str(v)) for v in sdn["lev0"]]] @ sam["Lambda"][0]
        want = np.where(hM.distr[:, 0] == 2, stats.norm.cdf(Lp), Lp)
        assert rel_err(pred[k], want) < 1e-10, (k, rel_err(pred[k], want))
    fit = H.computePredictedValues(out, expected=True, seed=1)
    assert fit.shape == (90, 8, 12) and np.all(np.isfinite(fit))
