"""Variable selection (Hmsc(XSelect = ...)) on the host: the model object's checks, the limits
named before any device work, combineParameters' order of back-scaling and zeroing, and the
Metropolis step of updateBetaSel itself -- detailed balance evaluated exactly on a tiny model,
which the Gaussian density satisfies and the reference's pnorm does not."""
import numpy as np
import pandas as pd
import pytest
from scipy import stats

from helpers import H, phylo_corr
from hmsc_amd.sampler import _check_xselect, combine_parameters
from oracle.rng import Rng
import betasel_oracle as BO


def _data(ny=30, ns=4, nc=3, seed=0):
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, nc - 1)) * 2.0 + 1.5])
    Y = (rng.standard_normal((ny, ns)) > 0).astype(float)
    names = ["(Intercept)"] + [f"x{k}" for k in range(1, nc)]
    return dict(Y=Y, X=X, covNames=names, distr="probit")


def test_model_checks_and_fields():
    kw = _data()
    sel = dict(covGroup=[2, 3], spGroup=[1, 2, 1, 2], q=[0.5, 0.2])
    hM = H.Hmsc(XSelect=[sel], **kw)
    assert hM.ncsel == 1 and len(hM) == 73 and "XSelect" in hM.names()
    xs = hM["XSelect"][0]
    assert list(xs["covGroup"]) == [2, 3] and list(xs["spGroup"]) == [1, 2, 1, 2] and list(xs["q"]) == [0.5, 0.2]
    plain = H.Hmsc(**kw)
    assert plain.ncsel == 0 and len(plain) == 72 and "XSelect" not in plain.names()
    assert H.Hmsc(XSelect=[], **kw).ncsel == 0 and len(H.Hmsc(XSelect=[], **kw)) == 72
    with pytest.raises(ValueError, match="covGroup for XSelect cannot have values greater than number of columns in X"):
        H.Hmsc(XSelect=[dict(sel, covGroup=[2, 4])], **kw)
    with pytest.raises(ValueError, match="covGroup"):
        H.Hmsc(XSelect=[dict(sel, covGroup=[0, 2])], **kw)
    with pytest.raises(ValueError, match="spGroup"):
        H.Hmsc(XSelect=[dict(sel, spGroup=[1, 2, 1])], **kw)
    with pytest.raises(ValueError, match="spGroup"):
        H.Hmsc(XSelect=[dict(sel, spGroup=[1, 2, 3, 1])], **kw)
    with pytest.raises(ValueError, match="q for XSelect"):
        H.Hmsc(XSelect=[dict(sel, q=[0.5, 1.2])], **kw)
    for missing in ("covGroup", "spGroup", "q"):
        bad = {k: v for k, v in sel.items() if k != missing}
        with pytest.raises(NotImplementedError, match="XSelect") as ei:
            H.Hmsc(XSelect=[bad], **kw)
        assert "RRR" not in str(ei.value) and "reduced" not in str(ei.value)
    with pytest.raises(NotImplementedError, match="species-specific X lists"):
        H.Hmsc(Y=kw["Y"], XData=[pd.DataFrame(kw["X"][:, 1:])] * 4, XSelect=[sel], distr="probit")


def test_limits_named_before_device_work():
    kw = _data()
    sel = dict(covGroup=[2], spGroup=[1, 1, 2, 2], q=[0.5, 0.5])
    _check_xselect(H.Hmsc(XSelect=[sel], **kw))                      # supported: no error
    with pytest.raises(NotImplementedError, match="phylogeny"):
        _check_xselect(H.Hmsc(XSelect=[sel], C=phylo_corr(4), **kw))
    with pytest.raises(NotImplementedError, match="reduced-rank regression"):
        _check_xselect(H.Hmsc(XSelect=[sel], XRRR=np.random.default_rng(1).standard_normal((30, 2)), ncRRR=1, **kw))
    with pytest.raises(NotImplementedError, match="overlapping covGroups"):
        _check_xselect(H.Hmsc(XSelect=[sel, dict(sel, covGroup=[2, 3])], **kw))
    with pytest.raises(NotImplementedError, match="more than 8 selections"):
        _check_xselect(H.Hmsc(XSelect=[dict(sel, covGroup=[2])] * 9, **kw))
    names = np.array([f"s{k:05d}" for k in np.arange(30) % 10])
    rs = H.HmscRandomLevel(sData=np.random.default_rng(2).random((10, 2)))
    with pytest.raises(NotImplementedError, match="spatial"):
        _check_xselect(H.Hmsc(XSelect=[sel], studyDesign=pd.DataFrame({"lev0": names}), ranLevels={"lev0": rs}, **kw))
    xdf = pd.DataFrame(np.column_stack([np.ones(10), np.arange(10.0)]), columns=["a", "b"],
                       index=[f"s{k:05d}" for k in range(10)])
    rx = H.HmscRandomLevel(xData=xdf)
    with pytest.raises(NotImplementedError, match="covariate-dependent"):
        _check_xselect(H.Hmsc(XSelect=[sel], studyDesign=pd.DataFrame({"lev0": names}), ranLevels={"lev0": rx}, **kw))


def test_combine_parameters_scales_from_raw_rows_then_zeroes():
    """R/combineParameters.R:15-28,45-53: the intercept takes -m Beta[k,] of a deselected covariate
    from the raw row; only then is Beta[covGroup, fsp] zeroed."""
    kw = _data(ns=4)
    sel = [dict(covGroup=[2], spGroup=[1, 1, 2, 2], q=[0.5, 0.5]), dict(covGroup=[3], spGroup=[1, 2, 2, 2], q=[0.3, 0.3])]
    hM = H.Hmsc(XSelect=sel, **kw)
    S, nc, ns = 2, 3, 4
    rng = np.random.default_rng(3)
    raw = rng.standard_normal((S, nc, ns))
    iV = np.stack([np.eye(nc) * (k + 1.0) for k in range(S)])
    bsel = np.array([[1, 0, 0, 1], [0, 1, 1, 1]], dtype=np.int32)       # [sel 1: g1 g2 | sel 2: g1 g2]
    rec = dict(Beta=raw.copy(), Gamma=rng.standard_normal((S, nc, 1)), iV=iV, iSigma=np.ones((S, ns)),
               rho=np.ones(S, dtype=np.int32), nf=np.zeros((0, S), dtype=np.int32), BetaSel=bsel)
    post = combine_parameters(rec, hM)
    mu, sd = hM.XScalePar
    assert np.all(mu[1:] != 0) and np.all(sd[1:] != 1)                  # both covariates are scaled
    for k in range(S):
        want = raw[k].copy()
        for c in (1, 2):
            want[c] = want[c] / sd[c]
            want[0] = want[0] - mu[c] * want[c]                          # from the raw row, deselected or not
        on1 = bsel[k, :2][np.array([0, 0, 1, 1])].astype(bool)
        on2 = bsel[k, 2:][np.array([0, 1, 1, 1])].astype(bool)
        assert np.allclose(post[k]["Beta"][0], want[0], rtol=1e-14, atol=0)
        assert np.array_equal(post[k]["Beta"][1] == 0, ~on1) and np.array_equal(post[k]["Beta"][2] == 0, ~on2)
        assert np.allclose(post[k]["Beta"][1][on1], want[1][on1], rtol=1e-14, atol=0)
        assert np.allclose(post[k]["Beta"][2][on2], want[2][on2], rtol=1e-14, atol=0)
        assert len(post[k]) == 13                                        # BetaSel is not part of a sample
    # a record without BetaSel (a plain model): nothing is zeroed
    plain = H.Hmsc(**kw)
    rec.pop("BetaSel")
    assert np.all(combine_parameters(rec, plain)[0]["Beta"] != 0)


def _tiny(groups, seed):
    """ny = 12, ns = 3, nc = 3, no random level; one selection on columns 2 and 3."""
    ny, ns, nc = 12, 3, 3
    rng = np.random.default_rng(seed)
    q = list(rng.uniform(0.2, 0.8, max(groups)))
    hM = BO.synthetic_sel(ny, ns, nc, [dict(covGroup=[2, 3], spGroup=groups, q=q)], seed=seed)
    m = BO.sel_model(hM)
    st = dict(Beta=rng.normal(0, 0.7, (nc, ns)), Z=rng.normal(0, 1.5, (ny, ns)), iSigma=rng.uniform(0.5, 2.0, ns),
              Eta=[], Lambda=[])
    return m, st


def _log_target(st, m, bsel):
    """log pi(BetaSel | rest) up to a constant, by direct evaluation: the prior odds and the
    Gaussian log-density of every cell of Z under the masked linear predictor."""
    M = BO.column_mask(m, bsel)
    E = m["X"] @ (M * st["Beta"])
    lp = np.sum(stats.norm.logpdf(st["Z"], loc=E, scale=st["iSigma"][None, :] ** -0.5))
    for xs, b in zip(m["XSelect"], bsel):
        lp += np.sum(np.where(b, np.log(xs["q"]), np.log(1 - xs["q"])))
    return lp


def _balance_gap(m, st, g, others, density):
    """|pi_off a(off -> on) - pi_on a(on -> off)| / pi_off a(off -> on) for group g, the other
    groups held at `others`; the acceptance ratios are the restatement's own lldif + pridif."""
    lr = {}
    for cur in (False, True):
        b = np.array(others, dtype=bool)
        b[g] = cur
        _, info = BO.update_beta_sel(dict(st, BetaSel=[b]), m, Rng(1), 1, density=density)
        # (groups before g are offered a flip first, but g's ratio does not depend on them: the
        # groups of one selection hold disjoint species)
        lr[cur] = info[0]["logratio"][g]
    b_on, b_off = np.array(others, dtype=bool), np.array(others, dtype=bool)
    b_on[g], b_off[g] = True, False
    ratio = np.exp(_log_target(st, m, [b_on]) - _log_target(st, m, [b_off]))
    pi_off, pi_on = 1 / (1 + ratio), ratio / (1 + ratio)
    lhs = pi_off * min(1.0, np.exp(lr[False]))
    rhs = pi_on * min(1.0, np.exp(lr[True]))
    return abs(lhs - rhs) / lhs


@pytest.mark.parametrize("groups", [[1, 1, 1], [1, 2, 1]])
def test_detailed_balance_exact(groups):
    """pi_off min(1, r_on) = pi_on min(1, r_off), evaluated exactly (no sampling), to 1e-12."""
    ng = max(groups)
    for seed in (1, 2, 3):
        m, st = _tiny(groups, seed)
        for g in range(ng):
            for rest in ([False] * ng, [True] * ng):
                assert _balance_gap(m, st, g, rest, "dnorm") < 1e-12, (groups, seed, g, rest)


@pytest.mark.parametrize("groups", [[1, 1, 1], [1, 2, 1]])
def test_reference_pnorm_breaks_detailed_balance(groups):
    """Deviation from Hmsc 3.0-4: the same check through R/updateBetaSel.R:53,79's
    pnorm(log.p = TRUE) fails by many orders of magnitude more than rounding."""
    ng = max(groups)
    gaps = []
    for seed in (1, 2, 3):
        m, st = _tiny(groups, seed)
        gaps += [_balance_gap(m, st, g, [True] * ng, "pnorm") for g in range(ng)]
    assert min(gaps) > 1e-3, gaps


def test_init_betasel_stream():
    m, _ = _tiny([1, 2, 1], 4)
    b = BO.init_betasel(m, Rng(11))
    u = Rng(11).uniforms(np.arange(2), 0, BO.S_INIT_BETASEL, 0)[0]
    assert np.array_equal(b[0], u < m["XSelect"][0]["q"])
