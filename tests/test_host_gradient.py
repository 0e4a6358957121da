"""The host side of the gradient workflow (hmsc_amd/gradient.py, predict's XData / ranLevels /
Gradient arguments, model_matrix's xlev): constructGradient and prepareGradient against numbers
worked out by hand here, gradientSummary(predY=) against plotGradient's formulas written out in
tests/community_reference.py.  CPU only: nothing here loads the device library.
"""
import numpy as np
import pandas as pd
import pytest

import community_reference as CR
import hmsc_amd as H
from hmsc_amd import gradient as G
from hmsc_amd.predict import _new_design


def _model(n=40, seed=1, spatial="coords"):
    rng = np.random.default_rng(seed)
    x1 = rng.standard_normal(n)
    df = pd.DataFrame(dict(x1=x1, x2=0.5 * x1 + rng.standard_normal(n), hab=rng.choice(["a", "b", "c"], n),
                           f2=np.where(x1 > 0, "hi", "lo")))
    names = [f"s{k:02d}" for k in range(n)]
    xy = rng.random((n, 2))
    if spatial == "coords":
        rl = H.HmscRandomLevel(sData=pd.DataFrame(xy, index=names))
    elif spatial == "dist":
        d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
        rl = H.HmscRandomLevel(distMat=pd.DataFrame(d, index=names, columns=names))
    else:
        rl = H.HmscRandomLevel(units=names)
    rl2 = H.HmscRandomLevel(units=[f"p{k % 5}" for k in range(n)])
    sd = pd.DataFrame(dict(site=names, plot=[f"p{k % 5}" for k in range(n)]))
    Tr = np.column_stack([np.ones(4), rng.standard_normal(4)])
    hM = H.Hmsc(Y=rng.standard_normal((n, 4)), XData=df, XFormula="~x1+x2+hab+f2", Tr=Tr, studyDesign=sd,
                ranLevels=dict(site=rl, plot=rl2))
    return hM, df, xy


def test_continuous_focal_grid_and_types():
    hM, df, xy = _model()
    gr = H.constructGradient(hM, "x1", {"hab": (1,), "f2": (3, "lo")}, ngrid=7)
    X = gr["XDataNew"]
    assert list(X.columns) == ["x1", "x2", "hab", "f2"] and len(X) == 7
    xx = np.asarray(X["x1"])
    assert xx[0] == df["x1"].min() and xx[-1] == df["x1"].max()
    assert np.allclose(np.diff(xx), (df["x1"].max() - df["x1"].min()) / 6, rtol=1e-13, atol=0)
    # type 2 (the default) for x2: lm(x2 ~ x1) on the grid
    assert np.allclose(X["x2"], np.polyval(np.polyfit(df["x1"], df["x2"], 1), xx), rtol=1e-10, atol=1e-12)
    # type 1 for a factor: the mode; type 3: the value
    vals = list(df["hab"])                            # R's Mode: the first met among the most frequent
    assert set(X["hab"]) == {max(dict.fromkeys(vals), key=vals.count)}
    assert list(X["f2"]) == ["lo"] * 7
    gr1 = H.constructGradient(hM, "x1", {"x2": (1,), "hab": (1,), "f2": (1,)}, ngrid=3)
    assert np.array_equal(gr1["XDataNew"]["x2"], np.full(3, df["x2"].mean()))
    gr3 = H.constructGradient(hM, "x1", {"x2": (3, 0.25), "hab": (1,), "f2": (1,)}, ngrid=3)
    assert list(gr3["XDataNew"]["x2"]) == [0.25] * 3


def test_factor_focal_grid():
    hM, df, xy = _model()
    gr = H.constructGradient(hM, "hab", {"f2": (1,)}, ngrid=20)
    X = gr["XDataNew"]
    assert list(X["hab"]) == ["a", "b", "c"] and list(X.columns) == ["hab", "x1", "x2", "f2"]
    for name in ("x1", "x2"):       # lm on a factor: the group means
        assert np.allclose(X[name], [df[name][df["hab"] == lv].mean() for lv in "abc"], rtol=1e-10, atol=1e-12)
    assert len(gr["studyDesignNew"]) == 3


def test_new_unit_coordinates_and_counts():
    hM, df, xy = _model()
    gr = H.constructGradient(hM, "x1", {"hab": (1,), "f2": (1,)}, ngrid=4)
    sd, rl = gr["studyDesignNew"], gr["rLNew"]
    assert list(sd.columns) == ["site", "plot"] and np.all(sd.values == "new_unit") and sd.shape == (4, 2)
    assert rl["site"].s.shape == (41, 2) and np.array_equal(rl["site"].s[:40], xy)
    assert np.array_equal(rl["site"].s[40], xy.mean(axis=0))
    assert rl["site"]["sNames"][-1] == "new_unit" and rl["site"]["sNames"][:40] == [f"s{k:02d}" for k in range(40)]
    assert rl["site"].N == 41 and rl["plot"].N == hM.rL[1].N + 1 and rl["plot"].pi[-1] == "new_unit"
    assert hM.rL[0].N == 40 and hM.rL[0].s.shape == (40, 2)          # the model's own levels are untouched


def test_new_unit_distmat_row():
    hM, df, xy = _model(spatial="dist")
    dm = np.asarray(hM.rL[0].distMat)
    gr = H.constructGradient(hM, "x1", {"hab": (1,), "f2": (1,)}, ngrid=4)
    d1 = gr["rLNew"]["site"].distMat
    rm = dm.mean(axis=1)
    two = np.argsort(rm)[:2]
    assert rm[two[0]] <= rm[two[1]] and np.all(rm[two[1]] <= np.delete(rm, two))
    new = 0.5 * (dm[two[0]] + dm[two[1]])
    assert d1.shape == (41, 41) and np.array_equal(d1[:40, :40], dm)
    assert np.allclose(d1[40, :40], new, rtol=1e-15, atol=0) and np.array_equal(d1[:40, 40], d1[40, :40]) and d1[40, 40] == 0
    assert gr["rLNew"]["site"]["distNames"][-1] == "new_unit"


def test_multinom_restatement():
    """Class frequencies are recovered when the focal variable carries no information (a constant
    design: the intercept-only maximum is the frequencies); the right class on each side of a
    well-separated two-class split; and the gradient uses it for a non-focal factor of type 2."""
    y = np.array([0] * 10 + [1] * 25 + [2] * 15)
    B = G.multinom_fit(np.ones((50, 1)), y, 3)
    p = np.exp(np.r_[0.0, B[0]])
    assert np.allclose(p / p.sum(), [0.2, 0.5, 0.3], rtol=1e-9, atol=0)
    # no information in a symmetric design either: x takes both values equally often in every class
    x = np.tile([-1.0, 1.0], 25)
    B = G.multinom_fit(np.column_stack([np.ones(50), x]), np.repeat([0, 1, 2, 1, 2], 10), 3)
    assert np.allclose(B[1], 0.0, atol=1e-8)
    p = np.exp(np.r_[0.0, B[0]])
    assert np.allclose(p / p.sum(), [0.2, 0.4, 0.4], rtol=1e-8, atol=0)
    rng = np.random.default_rng(3)
    x = np.r_[rng.uniform(-3, -1, 30), rng.uniform(1, 3, 30)]
    y = np.r_[np.zeros(30, int), np.ones(30, int)]
    B = G.multinom_fit(np.column_stack([np.ones(60), x]), y, 2)
    cls = G.multinom_predict(B, np.column_stack([np.ones(4), [-2.5, -0.5, 0.5, 2.5]]))
    assert list(cls) == [0, 0, 1, 1]
    hM, df, xy = _model()
    gr = H.constructGradient(hM, "x1", {"hab": (1,)}, ngrid=6)      # f2 = "hi" exactly where x1 > 0
    lo_max, hi_min = df["x1"][df["x1"] <= 0].max(), df["x1"][df["x1"] > 0].min()
    for v, c in zip(gr["XDataNew"]["x1"], gr["XDataNew"]["f2"]):     # (the boundary lies somewhere in the gap)
        assert c == "hi" if v >= hi_min else c == "lo" if v <= lo_max else True


def test_model_matrix_xlev():
    hM, df, xy = _model()
    one = pd.DataFrame(dict(x1=[0.5, 1.5], x2=[0.0, 1.0], hab=["b", "b"], f2=["lo", "lo"]))
    X0, names0 = H.model_matrix("~x1+x2+hab+f2", one)
    assert names0 == ["(Intercept)", "x1", "x2"]                      # without xlev a one-level factor has no column
    X, names = H.model_matrix("~x1+x2+hab+f2", one, xlev=dict(hab=["a", "b", "c"], f2=["hi", "lo"]))
    assert names == list(hM.covNames) == ["(Intercept)", "x1", "x2", "habb", "habc", "f2lo"]
    assert np.array_equal(X, [[1, 0.5, 0.0, 1, 0, 1], [1, 1.5, 1.0, 1, 0, 1]])
    with pytest.raises(ValueError, match="new levels"):
        H.model_matrix("~hab", pd.DataFrame(dict(hab=["z"])), xlev=dict(hab=["a", "b"]))
    # predict's design from a Gradient: the fitted model's columns
    gr = H.constructGradient(hM, "x1", {"hab": (1,), "f2": (3, "lo")}, ngrid=5)
    hM2, Xn, sd = _new_design(hM, None, None, None, None, gr)
    assert Xn.shape == (5, hM.nc) and sd is gr["studyDesignNew"] and hM2.rL[0].N == 41 and hM.rL[0].N == 40


def test_prepare_gradient():
    hM, df, xy = _model()
    new_xy = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    gr = H.prepareGradient(hM, df.iloc[:3], dict(site=new_xy))
    assert list(gr["studyDesignNew"]["site"]) == ["new_spatial_unit000001", "new_spatial_unit000002",
                                                  "new_spatial_unit000003"]
    assert list(gr["studyDesignNew"]["plot"]) == ["new_unit"] * 3
    rl = gr["rLNew"]["site"]
    assert rl.s.shape == (43, 2) and np.array_equal(rl.s[:40], xy) and np.array_equal(rl.s[40:], new_xy)
    assert rl["sNames"][40:] == list(gr["studyDesignNew"]["site"]) and gr["rLNew"]["plot"].N == hM.rL[1].N + 1
    assert gr["XDataNew"] is not None and len(gr["XDataNew"]) == 3
    with pytest.raises(ValueError, match="sDataNew"):
        H.prepareGradient(hM, df.iloc[:3], {})


def test_predict_argument_errors():
    hM, df, xy = _model()
    gr = H.constructGradient(hM, "x1", {"hab": (1,), "f2": (1,)}, ngrid=3)
    with pytest.raises(ValueError, match="only one of XData and X"):
        H.predict(hM, post=[], XData=df, X=np.ones((3, 2)))
    with pytest.raises(ValueError, match="only one of XData and X"):
        H.predictCommunity(hM, post=[], Gradient=gr, X=np.ones((3, 2)))
    with pytest.raises(ValueError, match="necessary named levels"):
        H.predict(hM, post=[], XData=gr["XDataNew"], studyDesign=gr["studyDesignNew"], ranLevels=dict(site=gr["rLNew"]["site"]))
    with pytest.raises(ValueError, match="necessary named columns"):
        H.predict(hM, post=[], XData=gr["XDataNew"], studyDesign=gr["studyDesignNew"][["site"]])
    with pytest.raises(NotImplementedError, match="lists"):
        H.predict(hM, post=[], XData=[df, df])
    with pytest.raises(ValueError, match="17"):
        H.predictCommunity(hM, post=[], weights=np.ones((4, 14)))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        H.predictCommunity(hM, post=[], probs=(0.5, 1.5))


def test_gradient_summary_host_formulas():
    """gradientSummary(predY=) against plotGradient's lines on a small stack, NaN included."""
    hM, df, xy = _model()
    gr = H.constructGradient(hM, "x1", {"hab": (1,), "f2": (1,)}, ngrid=5)
    rng = np.random.default_rng(9)
    predY = [rng.standard_normal((5, 4)) for _ in range(11)]
    q = (0.025, 0.5, 0.975)
    for measure, index in (("S", 0), ("Y", 3), ("T", 1)):
        got = H.gradientSummary(hM, gr, measure, index=index, predY=predY)
        Pr, qp = CR.plot_gradient(predY, measure, index, q, np.asarray(hM.Tr), True)
        assert got["Pr"] == Pr and np.array_equal(np.stack([got["lo"], got["me"], got["hi"]]), qp)
        assert np.array_equal(got["xx"], gr["XDataNew"]["x1"]) and got["xlabel"] == "x1"
    assert H.gradientSummary(hM, gr, "S", predY=predY)["ylabel"] == "Summed response"
    assert H.gradientSummary(hM, gr, "Y", index=2, predY=predY)["ylabel"] == hM.spNames[2]
    assert H.gradientSummary(hM, gr, "T", index=1, predY=predY)["ylabel"] == hM.trNames[1]
    predY[4][0, 1] = np.nan
    got = H.gradientSummary(hM, gr, "S", predY=predY)
    Pr, qp = CR.plot_gradient(predY, "S", 0, q, np.asarray(hM.Tr), True)
    assert np.isnan(got["Pr"]) and np.isnan(Pr) and np.array_equal(np.stack([got["lo"], got["me"], got["hi"]]), qp)
    # the literal numbers at one grid point: type 7 on 11 values
    s = np.sort([p[2].sum() for p in predY])
    assert got["me"][2] == s[5] and np.isclose(got["lo"][2], s[0] + 0.25 * (s[1] - s[0]), rtol=1e-15)


def test_td_example_shapes():
    """The reference's examples: constructGradient(TD$m, "x1") and with x2 = list(1)."""
    from test_golden_td import td_model
    hM = td_model()
    for nf in (None, {"x2": (1,)}):
        gr = H.constructGradient(hM, "x1", nf)
        X = gr["XDataNew"]
        assert X.shape == (20, 2) and list(X.columns) == ["x1", "x2"]
        assert X["x1"].iloc[0] == np.min(hM.XData["x1"]) and X["x1"].iloc[-1] == np.max(hM.XData["x1"])
        assert set(X["x2"]) <= {"o", "c"}
        assert gr["studyDesignNew"].shape == (20, 2) and list(gr["studyDesignNew"].columns) == ["sample", "plot"]
        assert list(gr["rLNew"]) == ["sample", "plot"]
        assert gr["rLNew"]["plot"].s.shape == (hM.rL[1].s.shape[0] + 1, 2) and gr["rLNew"]["sample"].N == hM.ny + 1
        Xn = _new_design(hM, None, None, None, None, gr)[1]
        assert Xn.shape == (20, hM.nc)
    assert len(set(gr["XDataNew"]["x2"])) == 1           # type 1: one level everywhere
