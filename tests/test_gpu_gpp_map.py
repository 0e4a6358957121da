"""Prediction maps of a GPP level (predictMap(gppDevice=True): mode 4 of hmsc_predict_map,
hmsc_amd/csrc/gpp.hip and map.hip) against the route through hmsc_krige, predictSummary(...,
krigeDevice=True, gppDevice=True) and predictCommunity(..., krigeDevice=True, gppDevice=True), itself
held to tests/gpp_krige_oracle.py by test_gpu_gpp_krige.py.  Every value of a slab's Eta table is a sum
over the knots in index order and draws of (unit or knot, factor, level, sample) counters, so every
comparison is for equal doubles: with the yardstick, between slab sizes (64 splits the 150 new units
over three slabs, which a 'Full' joint draw refuses) and with a unit that two slabs share.

Model (map_cases.py): 70 fitted spatial units, 16 knots, 37 species, 9 samples of 2 or 3 factors; the
equalities do not depend on conditioning, so map_cases' grid (a up to 1.1) is used as it is."""
import functools
import importlib

import numpy as np
import pandas as pd
import pytest

import map_cases as MC
from helpers import H

P = importlib.import_module("hmsc_amd.predict")        # (hmsc_amd.predict the attribute is the function)

pytestmark = pytest.mark.gpu

PROBS = (0.1, 0.5)
SLABS = (64, 128, 0)
UP = {"GammaEta": False}                                # (updateGammaEta has no GPP method, as in R)


@functools.lru_cache(maxsize=None)
def _model():
    hM = MC.model("GPP", sKnot="auto")
    return hM, MC.posterior(hM)


def _weights(hM):
    w = np.zeros(hM.ns)
    w[4] = 1.0
    return {"sp4": w}


def _yardstick(hM, post, G, seed, expected):
    kw = dict(post=post, Gradient=G, krigeDevice=True, gppDevice=True, seed=seed, expected=expected)
    return dict(cells=H.predictSummary(hM, probs=PROBS, **kw),
                community=H.predictCommunity(hM, measures=("S", "T"), weights=_weights(hM), **kw))


def _map(hM, post, G, seed, expected, slab_rows):
    return H.predictMap(hM, post=post, Gradient=G, seed=seed, expected=expected, probs=PROBS, measures=("S", "T"),
                        weights=_weights(hM), slab_rows=slab_rows, gppDevice=True)


def _assert_same(got, ref, what):
    for part, keys in (("cells", ("n", "occ", "mean", "quantiles", "median", "probs")),
                       ("community", ("n", "mean", "quantiles", "probs"))):
        for key in keys:
            a, b = np.asarray(got[part][key]), np.asarray(ref[part][key])
            assert a.shape == b.shape, (what, part, key, a.shape, b.shape)
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, part, key)
    assert got["community"]["columns"] == ref["community"]["columns"]


def _assert_all_slabs(hM, post, G, seed, expected, what):
    ref = _yardstick(hM, post, G, seed, expected)
    assert np.all(ref["community"]["n"] > 0) and np.all(np.isfinite(ref["cells"]["mean"]))
    for rows in SLABS:
        _assert_same(_map(hM, post, G, seed, expected, rows), ref, f"{what} slab_rows={rows}")
    return ref


@pytest.mark.parametrize("expected", [True, False], ids=["expected", "draws"])
def test_agreement(expected):
    hM, post = _model()
    ref = _assert_all_slabs(hM, post, MC.grid(hM, 150), 41, expected, f"GPP expected={expected}")
    # the joint conditional is not the mean: predictEtaMean gives other values
    mean = H.predictMap(hM, post=post, Gradient=MC.grid(hM, 150), seed=41, expected=expected, probs=PROBS,
                        predictEtaMean=True)
    assert not np.array_equal(mean["cells"]["mean"], ref["cells"]["mean"])


def test_shared_spatial_units():
    """Rows 20 and 120 share one new spatial unit (and 3 and 149 another): kriged in two slabs of 64
    rows, to the same doubles."""
    hM, post = _model()
    G = MC.shared_units(MC.grid(hM, 150), ((20, 120), (3, 149)))
    assert G["studyDesignNew"]["plot"].nunique() == 148
    _assert_all_slabs(hM, post, G, 77, False, "shared units")


def test_every_sample_at_the_zero_grid_point():
    """Every sample's spatial factors at the grid's a = 0 point: the level has no kriging plan, and its
    100 new units' values are z from the assembly kernel, hmsc_krige's z of the same counters."""
    hM, post = _model()
    zero = [dict(s, Alpha=[np.ones_like(s["Alpha"][0]), s["Alpha"][1]]) for s in post]
    G = MC.grid(hM, 100)
    ref = _yardstick(hM, zero, G, 23, False)
    assert np.all(np.isfinite(ref["cells"]["mean"]))
    for rows in (64, 0):
        _assert_same(_map(hM, zero, G, 23, False, rows), ref, f"all at a = 0 slab_rows={rows}")
    assert not np.array_equal(ref["cells"]["mean"], _yardstick(hM, post, G, 23, False)["cells"]["mean"])


def test_timing_slots():
    hM, post = _model()
    _map(hM, post, MC.grid(hM, 150), 8, False, 64)
    from hmsc_amd.gradient import mapTiming
    t = mapTiming()
    assert t["trsm"] == 0.0 and all(t[k] > 0.0 for k in ("plan", "K12", "mean", "assemble", "summary"))


@functools.lru_cache(maxsize=None)
def _fitted_gpp_model():
    ny, ns = 60, 5
    rng = np.random.default_rng(4)                     # (no unit on a knot: the sampler's GPP grid needs dD > 0)
    xy = rng.random((ny, 2))
    names = [f"s{k:03d}" for k in range(ny)]
    field = np.sin(4 * xy[:, 0]) + np.cos(3 * xy[:, 1])
    X = np.column_stack([np.ones(ny), rng.standard_normal(ny)])
    Lp = X @ rng.normal(0, 0.5, (2, ns)) + field[:, None] * rng.standard_normal(ns)[None, :]
    Y = (Lp + rng.standard_normal((ny, ns)) > 0).astype(float)
    rl = H.HmscRandomLevel(sData=pd.DataFrame(xy, index=names), sMethod="GPP", sKnot=H.constructKnots(xy, nKnots=3))
    H.setPriors(rl, nfMin=2, nfMax=2)
    hM = H.Hmsc(Y=Y, X=X, covNames=["(Intercept)", "x1"], distr="probit", studyDesign=pd.DataFrame({"plot": names}),
                ranLevels={"plot": rl})
    return H.sampleMcmc(hM, samples=6, transient=10, thin=1, nChains=1, seed=9, verbose=0, updater=UP)


def test_cross_validation_kriges_held_out_units_on_the_device(monkeypatch):
    """computePredictedValues(partition=..., krigeDevice=True, gppDevice=True) on a GPP model: every
    fold's held-out units go through predictLatentFactor(device=0, gppDevice=True) under the fold's
    seed, and their factors are that call's."""
    hM = _fitted_gpp_model()
    calls = []
    real = P.predictLatentFactor

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append((a, kw, out))
        return out

    monkeypatch.setattr(P, "predictLatentFactor", spy)
    partition = (np.arange(hM.ny) >= hM.ny // 2).astype(int)
    with pytest.raises(NotImplementedError, match="GPP kriging on the device is not implemented"):
        H.computePredictedValues(hM, partition=partition, seed=5, krigeDevice=True, updater=UP)
    calls.clear()
    pred = H.computePredictedValues(hM, partition=partition, seed=5, krigeDevice=True, gppDevice=True, updater=UP)
    assert pred.shape == (hM.ny, hM.ns, 6)
    assert np.all(np.isfinite(pred)) and np.all((pred >= 0) & (pred <= 1))
    assert len(calls) == 2
    monkeypatch.undo()
    for (a, kw, out) in calls:
        assert kw["gppDevice"] is True and kw["device"] == 0 and kw["seed"] == 5
        unitsPred, units, postEta, rl = a
        assert len(unitsPred) == 30 and not set(unitsPred) & set(units)       # all held out
        again = P.predictLatentFactor(unitsPred, units, postEta, rl, postAlpha=kw["postAlpha"], device=0, seed=5,
                                      level=kw["level"], gppDevice=True)
        assert all(np.array_equal(x, y) for x, y in zip(out, again))
        assert all(np.all(np.isfinite(x)) and np.std(x) > 0 for x in out)
