"""Variable selection (Hmsc(XSelect = ...)) on the device: updateBetaSel, its initial draw, the
masked BetaLambda kernels and every reader of the masked linear predictor, against the numpy
restatement (tests/betasel_oracle.py over oracle/hmsc_oracle.py) on the same state and Philox
key.  Tolerances are the project's: draws 1e-9, conditional moments 1e-10, three sweeps 1e-7."""
import numpy as np
import pandas as pd
import pytest

from helpers import H, O, oracle_model, phylo_corr, rel_err, synthetic_model
from hmsc_amd._lib import HmscNativeError
from oracle.rng import Rng
import betasel_oracle as BO

pytestmark = pytest.mark.gpu

TOL_MOMENT = 1e-10
TOL_DRAW = 1e-9
TOL_SWEEPS = 1e-7
UP = {"Gamma2": False, "GammaEta": False}     # R/sampleMcmc.R:207-216 clears both with ncsel > 0


def _partition(ns, sizes):
    """1-based group labels: consecutive runs of the given sizes, the last group taking the rest."""
    g = np.empty(ns, dtype=np.int64)
    pos = 0
    for k, n in enumerate(sizes):
        g[pos:pos + n] = k + 1
        pos += n
    g[pos:] = len(sizes) + 1
    return g


# Every code path at the smallest size:
#   one_group    no random level, one group holding every species (a serial sum over 9 species);
#   per_species  one group per species, ns = 22 not a multiple of 4 (the wave BetaLambda kernel's
#                ragged last workgroup), one unit per site: the fused Eta launch;
#   two_sel      two selections on disjoint columns whose uneven partitions share species (the
#                second selection sees the mask the first left), normal and probit species,
#                5 % NA (the direct pass over Z, the masked Gram of NA species, eta_na_row), two
#                levels (the general Eta path);
#   wideK        K = 6 + 30 = 36 > 32: the workgroup BetaLambda kernel.
MODELS = {
    "one_group": dict(ny=70, ns=9, nc=4, selections=[dict(covGroup=[3], spGroup=np.ones(9, dtype=int), q=[0.5])], seed=1),
    "per_species": dict(ny=130, ns=22, nc=5, units=(130,), nf=2, seed=2,
                        selections=[dict(covGroup=[2, 4], spGroup=np.arange(1, 23), q=np.linspace(0.2, 0.8, 22))]),
    "two_sel": dict(ny=203, ns=37, nc=6, units=(40, 203), nf=2, n_normal=15, na_frac=0.05, seed=3,
                    selections=[dict(covGroup=[2, 3], spGroup=_partition(37, [5, 13]), q=[0.4, 0.6, 0.5]),
                                dict(covGroup=[5], spGroup=_partition(37, [11, 2, 20]), q=[0.5, 0.3, 0.7, 0.5])]),
    "wideK": dict(ny=70, ns=10, nc=6, units=(70,), nf=30, seed=4,
                  selections=[dict(covGroup=[2, 6], spGroup=_partition(10, [4]), q=[0.5, 0.5])]),
}
# The chain seed, chosen on the CPU by the restatement alone: the first of 1, 2, 3, ... for which
# every decision of updateBetaSel at the iterations the tests use (7; 10, 11, 12 from the fixture
# state) keeps a margin |lldif + pridif - log u| > 1e-6 (1 + scale) in every model, so a decision
# cannot turn on rounding, and for which the update at iteration 7 flips some group (seed 1 holds
# the margin, 4e-3, but flips none; seed 2: margin 1.1e-2, 4 groups flip).  test_decision_margins
# asserts both.
SEED = 2
# test_adaptation_five_sweeps: the first seed for which the restatement both adds and drops a
# factor inside the five sweeps (nf 3, 4, 3, 4, 4; decision margins >= 0.24)
ADAPT_SEED = 2


def make_model(name):
    return BO.synthetic_sel(**MODELS[name])


@pytest.fixture(scope="module", params=list(MODELS))
def setup(request):
    """(name, hM, oracle model, state): the restatement's state after init and two sweeps,
    computed once per model and left unchanged."""
    hM = make_model(request.param)
    m = BO.sel_model(hM)
    rng = Rng(SEED)
    st = BO.compute_initial_parameters(m, rng)
    for it in (1, 2):
        st = BO.sweep_sel(st, m, rng, it, updater=UP)
    return request.param, hM, m, st


def _chain(hM, st=None, seed=SEED):
    ch = H.Chain(hM, seed, device=0, updater=UP)
    ch.init()
    if st is not None:
        ch.set_state(st)
    return ch


def _flat(bsel):
    return np.concatenate([np.asarray(b, dtype=bool) for b in bsel])


def _blx(ch, hM):
    nf = int(np.sum(ch.nf())) if hM.nr else 0
    K = hM.nc + nf
    return ch.debug_get("BLx", K * hM.ns).reshape(hM.ns, K).T, ch.debug_get("BL", K * hM.ns).reshape(hM.ns, K).T


FLIPS = {}


def _margin(info):
    with np.errstate(divide="ignore"):
        return min(float(np.min(np.abs(i["logratio"] - np.log(i["u"])) / (1 + i["scale"]))) for i in info)


def _margins(st, m, it):
    return _margin(BO.update_beta_sel(st, m, Rng(SEED), it)[1])


def test_decision_margins(setup):
    """The precondition of every exact comparison of decisions, on the restatement alone."""
    name, hM, m, st = setup
    assert _margins(st, m, 7) > 1e-6, name
    FLIPS[name] = int(np.sum(_flat(BO.update_beta_sel(st, m, Rng(SEED), 7)[0]) != _flat(st["BetaSel"])))
    if len(FLIPS) == len(MODELS):
        assert sum(FLIPS.values()) > 0, FLIPS
    o, rng = st, Rng(SEED)
    for it in (10, 11, 12):
        info = []
        o = BO.sweep_sel(o, m, rng, it, updater=UP, info_out=info)
        assert _margin(info[0]) > 1e-6, (name, it)


def test_init_parity(setup):
    """BetaSel bit for bit; the initial Z from the unmasked X (R/computeInitialParameters.R:229-254)."""
    name, hM, m, _ = setup
    ch = _chain(hM)
    g = ch.get_state()
    blx, bl = _blx(ch, hM)
    ch.close()
    o = BO.compute_initial_parameters(m, Rng(SEED))
    assert np.array_equal(_flat(g["BetaSel"]), _flat(o["BetaSel"])), name
    for k in ("Gamma", "iV", "Beta", "iSigma", "Z"):
        assert rel_err(g[k], o[k]) < TOL_DRAW, (name, k, rel_err(g[k], o[k]))
    M = BO.column_mask(m, o["BetaSel"])
    assert np.array_equal(blx[:hM.nc], M * bl[:hM.nc]) and np.array_equal(blx[hM.nc:], bl[hM.nc:])
    if not _flat(o["BetaSel"]).all():   # the masked predictor would have given another Z
        assert rel_err(O.update_z(BO.masked(o, m), m, Rng(SEED), 0, Y=m["Yraw"]), o["Z"]) > 1e-6


def test_log_ratio_and_decisions(setup):
    name, hM, m, st = setup
    assert _margins(st, m, 7) > 1e-6, name                      # no case left out
    ch = _chain(hM, st)
    ch.update("BetaSel", 7)
    g = ch.get_state(with_z=False)
    ntot = _flat(st["BetaSel"]).size
    lr, sc = ch.debug_get("BetaSelLogRatio", ntot), ch.debug_get("BetaSelScale", ntot)
    blx, bl = _blx(ch, hM)
    ch.close()
    b, info = BO.update_beta_sel(st, m, Rng(SEED), 7)
    want = np.concatenate([i["logratio"] for i in info])
    scale = np.concatenate([i["scale"] for i in info])
    print(name, "max |dlr| / (1 + scale):", np.max(np.abs(lr - want) / (1 + scale)))
    assert np.all(np.abs(lr - want) <= TOL_DRAW * (1 + scale)), (name, np.abs(lr - want) / (1 + scale))
    assert np.all(np.isfinite(sc)) and np.all(sc >= 0)
    assert np.array_equal(_flat(g["BetaSel"]), _flat(b)), name
    assert rel_err(g["Beta"], st["Beta"]) == 0.0                       # BL stays raw
    M = BO.column_mask(m, b)
    assert np.array_equal(blx[:hM.nc], M * bl[:hM.nc]) and np.array_equal(blx[hM.nc:], bl[hM.nc:])


def _flipped(st):
    return dict(st, BetaSel=[~np.asarray(b, dtype=bool) for b in st["BetaSel"]])


@pytest.mark.parametrize("flip", [False, True])
def test_beta_lambda_after_a_selection(setup, flip):
    name, hM, m, st = setup
    s2 = _flipped(st) if flip else st
    ch = _chain(hM, s2)
    ch.set_noise_mode(1 | 2)
    ch.update("BetaLambda", 5)
    g = ch.get_state(with_z=False)
    K = hM.nc + (int(np.sum(ch.nf())) if hM.nr else 0)
    dp = ch.debug_get("BL_prec", hM.ns * K * K).reshape(hM.ns, K, K).transpose(0, 2, 1)
    ch.set_state(s2)
    ch.set_noise_mode(0)
    ch.update("BetaLambda", 5)
    d = ch.get_state(with_z=False)
    blx, bl = _blx(ch, hM)
    ch.close()
    precs, _ = BO.beta_lambda_moments(s2, m)
    assert rel_err(dp, precs) < TOL_MOMENT, (name, rel_err(dp, precs))
    M = BO.column_mask(m, s2["BetaSel"])
    off = np.nonzero(M[:, 0] == 0)[0]
    if off.size and not np.isnan(m["Y"][:, 0]).any():   # a deselected row keeps its prior precision only
        assert rel_err(dp[0][off][:, off], s2["iV"][np.ix_(off, off)]) < 1e-14
    B, Lam = BO.update_beta_lambda(s2, m, Rng(SEED), 5, zero_noise=True)
    assert rel_err(g["Beta"], B) < TOL_MOMENT, (name, rel_err(g["Beta"], B))
    for r in range(hM.nr):
        assert rel_err(g["Lambda"][r], Lam[r]) < TOL_MOMENT, (name, r)
    B, Lam = BO.update_beta_lambda(s2, m, Rng(SEED), 5)
    assert rel_err(d["Beta"], B) < TOL_DRAW, (name, rel_err(d["Beta"], B))
    for r in range(hM.nr):
        assert rel_err(d["Lambda"][r], Lam[r]) < TOL_DRAW, (name, r)
    assert np.array_equal(blx[:hM.nc], M * bl[:hM.nc])                # BLx follows the new BL


@pytest.mark.parametrize("upd", ["Eta", "InvSigma", "Z"])
def test_updaters_after_a_changed_mask(setup, upd):
    """Every reader of X Beta takes the masked BL: after set_state with every BetaSel inverted and
    a device updateBetaSel on top, the next updater's draw equals the restatement's."""
    name, hM, m, st = setup
    s2 = _flipped(st)
    ch = _chain(hM, s2)
    ch.update("BetaSel", 7)
    b = ch.get_state(with_z=False)["BetaSel"]
    ch.update(upd, 8)
    g = ch.get_state()
    ch.close()
    if _margins(s2, m, 7) > 1e-6:     # (where the margin holds, the decisions are checked here too)
        assert np.array_equal(_flat(b), _flat(BO.update_beta_sel(s2, m, Rng(SEED), 7)[0]))
    s3 = BO.masked(dict(s2, BetaSel=b), m)
    rng = Rng(SEED)
    if upd == "Eta":
        Eta = O.update_eta(s3, m, rng, 8)
        for r in range(hM.nr):
            assert rel_err(g["Eta"][r], Eta[r]) < TOL_DRAW, (name, r, rel_err(g["Eta"][r], Eta[r]))
    elif upd == "InvSigma":
        assert rel_err(g["iSigma"], O.update_inv_sigma(s3, m, rng, 8)) < TOL_DRAW
    else:
        Z = O.update_z(s3, m, rng, 8)
        assert rel_err(g["Z"], Z) < TOL_DRAW, (name, rel_err(g["Z"], Z))
    assert rel_err(g["Beta"], st["Beta"]) == 0.0


def test_three_sweeps_track_oracle(setup):
    name, hM, m, st = setup
    ch = _chain(hM, st)
    rng, o = Rng(SEED), st
    for it in range(10, 13):
        ch.sweep(it)
        o = BO.sweep_sel(o, m, rng, it, updater=UP)
    g = ch.get_state()
    ch.close()
    assert np.array_equal(_flat(g["BetaSel"]), _flat(o["BetaSel"])), name
    for k in ("Beta", "Gamma", "iV", "iSigma", "Z"):
        assert rel_err(g[k], o[k]) < TOL_SWEEPS, (name, k, rel_err(g[k], o[k]))
    for r in range(hM.nr):
        assert rel_err(g["Eta"][r], o["Eta"][r]) < TOL_SWEEPS, (name, r)


def test_graph_replay_matches_eager(setup, monkeypatch):
    """run() replays the captured sweep (updateBetaSel, the mask and BLx inside it) bit for bit
    like eager launches, every sweep recorded, BetaSel in the record."""
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
    keys = ["Beta", "Gamma", "iV", "iSigma", "BetaSel"]
    for r in range(hM.nr):
        keys += [f"Lambda{r}", f"Eta{r}", f"Psi{r}", f"Delta{r}"]
    for k in keys:
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
    ntot = sum(len(x["q"]) for x in hM["XSelect"])
    assert out[0]["BetaSel"].shape == (11, ntot) and set(np.unique(out[0]["BetaSel"])) <= {0, 1}


def test_adaptation_five_sweeps():
    """updateNf on: the repack of BL carries BLx along.  Five sweeps from iteration 21 (a level may
    grow only past iteration 20) against the restatement (ADAPT_SEED).  Bound: the three-sweep bound 1e-7 over the draw
    bound 1e-9 allows a growth of (1e-7 / 1e-9)^(1/3) = 4.6 per sweep, so five sweeps 1e-9 4.6^5 = 2e-6."""
    hM = BO.synthetic_sel(ny=90, ns=12, nc=4, units=(30,), nf=2, nf_max=5, seed=5,
                          selections=[dict(covGroup=[2, 3], spGroup=_partition(12, [5]), q=[0.5, 0.5])])
    m = BO.sel_model(hM)
    seed = ADAPT_SEED
    rng = Rng(seed)
    st = BO.compute_initial_parameters(m, rng)
    ch = H.Chain(hM, seed, device=0, updater=UP)
    ch.init()
    o = st
    nfs = []
    for it in range(21, 26):
        ch.sweep(it, adapt=True)
        o = BO.sweep_sel(o, m, rng, it, updater=UP, adapt_nf=[25])
        nfs.append(o["Lambda"][0].shape[0])
    g = ch.get_state()
    blx, bl = _blx(ch, hM)
    ch.close()
    assert any(b > a for a, b in zip([2] + nfs, nfs)) and any(b < a for a, b in zip(nfs, nfs[1:])), nfs
    assert g["Lambda"][0].shape == o["Lambda"][0].shape
    assert np.array_equal(_flat(g["BetaSel"]), _flat(o["BetaSel"]))
    M = BO.column_mask(m, g["BetaSel"])
    assert np.array_equal(blx[:hM.nc], M * bl[:hM.nc]) and np.array_equal(blx[hM.nc:], bl[hM.nc:])
    for k in ("Beta", "Gamma", "iV", "Z"):
        assert rel_err(g[k], o[k]) < 2e-6, (k, rel_err(g[k], o[k]))


def test_refusals():
    hM = make_model("per_species")
    with pytest.raises(HmscNativeError, match="species-sharded"):
        H.Chain(hM, 1, device=0, updater=UP, host_allreduce=lambda x: None)
    with pytest.raises(HmscNativeError, match="updateGamma2"):
        H.Chain(hM, 1, device=0, updater={"GammaEta": False})
    with pytest.raises(HmscNativeError, match="updateGammaEta"):
        H.Chain(hM, 1, device=0, updater={"Gamma2": False})
    hP = make_model("per_species")
    hP.C = phylo_corr(hP.ns)
    with pytest.raises(HmscNativeError, match="phylogeny"):
        H.Chain(hP, 1, device=0, updater=UP)
    rng = np.random.default_rng(0)
    ny, ns = 60, 6
    Y = (rng.standard_normal((ny, ns)) > 0).astype(float)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, 9))])
    names = ["(Intercept)"] + [f"x{k}" for k in range(1, 10)]
    sel = dict(covGroup=[2], spGroup=np.ones(ns, dtype=int), q=[0.5])
    hR = H.Hmsc(Y=Y, X=X, covNames=names, XRRR=rng.standard_normal((ny, 3)), ncRRR=1, XSelect=[sel], distr="probit")
    with pytest.raises(HmscNativeError, match="reduced-rank regression"):
        H.Chain(hR, 1, device=0, updater=UP)
    units = np.array([f"s{k:05d}" for k in np.arange(ny) % 12])
    rs = H.HmscRandomLevel(sData=rng.random((12, 2)))
    H.setPriors(rs, nfMin=2, nfMax=2)
    hS = H.Hmsc(Y=Y, X=X, covNames=names, XSelect=[sel], distr="probit",
                studyDesign=pd.DataFrame({"lev0": units}), ranLevels={"lev0": rs})
    with pytest.raises(HmscNativeError, match="spatial"):
        H.Chain(hS, 1, device=0, updater=UP)
    xdf = pd.DataFrame(np.column_stack([np.ones(12), rng.standard_normal(12)]), columns=["a", "b"],
                       index=[f"s{k:05d}" for k in range(12)])
    rx = H.HmscRandomLevel(xData=xdf)
    H.setPriors(rx, nfMin=2, nfMax=2)
    hX = H.Hmsc(Y=Y, X=X, covNames=names, XSelect=[sel], distr="probit",
                studyDesign=pd.DataFrame({"lev0": units}), ranLevels={"lev0": rx})
    with pytest.raises(HmscNativeError, match="covariate-dependent"):
        H.Chain(hX, 1, device=0, updater=UP)
    hO = H.Hmsc(Y=Y, X=X, covNames=names, XSelect=[sel, dict(sel, covGroup=[2, 3])], distr="probit")
    with pytest.raises(HmscNativeError, match="overlapping covGroups"):
        H.Chain(hO, 1, device=0, updater=UP)
    h9 = H.Hmsc(Y=Y, X=X, covNames=names, XSelect=[dict(sel, covGroup=[c]) for c in range(2, 11)], distr="probit")
    with pytest.raises(HmscNativeError, match="ncsel <= 8"):
        H.Chain(h9, 1, device=0, updater=UP)


def test_plain_chain_is_unchanged():
    """A model without XSelect: BLx is BL itself, the BetaSel bit is ignored, the record carries no
    BetaSel, and three default sweeps (every fused path on) give the state they gave before -- the
    oracle's, which this change does not touch -- identically for two chains built the same way,
    one from Hmsc(...) and one from Hmsc(..., XSelect=[])."""
    kw = dict(ny=80, ns=10, nc=3, nf=2, seed=5)
    hM = synthetic_model(**kw)
    m = oracle_model(hM)
    states = []
    for variant in (0, 1):
        h = hM if variant == 0 else H.Hmsc(Y=hM.Y, X=hM.X, covNames=list(hM.covNames), XSelect=[], distr=hM.distr,
                                           studyDesign=hM.studyDesign, ranLevels=hM.ranLevels)
        assert h.ncsel == 0 and len(h) == 72
        ch = H.Chain(h, 3, device=0, updater={"GammaEta": False})
        ch.init()
        before = ch.get_state()
        ch.update("BetaSel", 1)
        after = ch.get_state()
        for k in ("Beta", "Gamma", "iV", "Z"):
            assert np.array_equal(before[k], after[k])
        assert "BetaSel" not in before
        for it in (1, 2, 3):
            ch.sweep(it)
        g = ch.get_state()
        K = h.nc + int(np.sum(ch.nf()))
        assert np.array_equal(ch.debug_get("BLx", K * h.ns), ch.debug_get("BL", K * h.ns))
        rec = ch.run(transient=1, samples=3, adaptNf=[0], iter0=3)
        ch.close()
        assert "BetaSel" not in rec
        states.append(g)
    for k in ("Beta", "Gamma", "iV", "iSigma", "Z"):
        assert np.array_equal(states[0][k], states[1][k]), k
    rng = Rng(3)
    o = O.compute_initial_parameters(m, rng)
    for it in (1, 2, 3):
        o = O.sweep(o, m, rng, it, updater={"GammaEta": False})
    for k in ("Beta", "Gamma", "iV", "Z"):
        assert rel_err(states[0][k], o[k]) < TOL_SWEEPS, (k, rel_err(states[0][k], o[k]))


def test_sample_mcmc_and_predict(capsys):
    """sampleMcmc end to end: R's two messages, recorded Beta exactly 0 where deselected (and
    nowhere else), predict and computePredictedValues run."""
    hM = BO.synthetic_sel(ny=90, ns=8, nc=4, units=(15,), nf=2, n_normal=3, seed=6,
                          selections=[dict(covGroup=[2, 3], spGroup=_partition(8, [3]), q=[0.5, 0.5])])
    out = H.sampleMcmc(hM, samples=6, transient=4, nChains=2, seed=2, verbose=0)
    text = capsys.readouterr().out
    assert "Setting updater$Gamma2=FALSE due to X is not a matrix" in text
    assert "Setting updater$GammaEta=FALSE due to X is not a matrix" in text
    zero_rows = 0
    for chain in out.postList:
        for s in chain:
            assert len(s) == 13 and s["Beta"].shape == (4, 8)          # BetaSel is not part of a sample
            z = s["Beta"] == 0
            assert not z[[0, 3]].any()
            for grp in (slice(0, 3), slice(3, 8)):                     # a group is on or off as a whole
                assert z[1:3, grp].all() or not z[1:3, grp].any()
            zero_rows += int(z.any())
    assert zero_rows > 0                                               # some sample had a group off
    post = H.poolMcmcChains(out.postList)
    pred = H.predict(out, post=post, expected=True, seed=1)
    assert len(pred) == 12 and pred[0].shape == (90, 8) and np.all(np.isfinite(pred[0]))
    sam = post[0]
    pi = out.Pi[:, 0] - 1
    Lp = out.X @ sam["Beta"] + sam["Eta"][0][pi] @ sam["Lambda"][0]
    from scipy import stats
    want = np.where(out.distr[:, 0] == 2, stats.norm.cdf(Lp), Lp)
    assert rel_err(pred[0], want) < 1e-10
    fit = H.computePredictedValues(out, expected=True, seed=1)
    assert fit.shape == (90, 8, 12) and np.all(np.isfinite(fit))


def test_selection_sanity():
    """A strong true effect is selected, an absent one is not: ny = 200, ns = 12, covariate 2 acts
    on group A (species 1-6) only, q = 0.5; over 150 recorded sweeps the inclusion frequency of A
    exceeds that of B in each of 4 chains.  The restatement alone is held to the same first, on
    the CPU, over 60 sweeps per chain instead of 150 (it gives A 0.83, 1, 1, 1 against B 0.18, 0,
    0, 0.07 for chain seeds 1-4)."""
    eff = np.zeros((3, 12))
    eff[0] = 0.2
    eff[1, :6] = 1.5
    eff[2] = np.linspace(-0.5, 0.5, 12)
    hM = BO.synthetic_sel(ny=200, ns=12, nc=3, units=(25,), nf=2, seed=7, effects=eff,
                          selections=[dict(covGroup=[2], spGroup=_partition(12, [6]), q=[0.5, 0.5])])
    m = BO.sel_model(hM)
    for seed in (1, 2, 3, 4):
        rng = Rng(seed)
        o = BO.compute_initial_parameters(m, rng)
        acc = []
        for it in range(1, 61):
            o = BO.sweep_sel(o, m, rng, it, updater=UP)
            acc.append(_flat(o["BetaSel"]))
        fa, fb = np.mean(acc, axis=0)
        assert fa > fb, ("restatement", seed, fa, fb)
    for seed in (1, 2, 3, 4):
        ch = H.Chain(hM, seed, device=0, updater=UP)
        ch.init()
        rec = ch.run(transient=0, samples=150, adaptNf=[0], fields=("BetaSel",))
        ch.close()
        fa, fb = rec["BetaSel"].mean(axis=0)
        print("chain", seed, "inclusion A", fa, "B", fb)
        assert fa > fb, (seed, fa, fb)
