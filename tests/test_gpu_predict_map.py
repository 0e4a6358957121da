"""predictMap (hmsc_predict_map, hmsc_amd/csrc/map.hip) against the route it replaces at map size:
predictSummary(..., Gradient=G, krigeDevice=True, seed=k) and predictCommunity(..., Gradient=G,
krigeDevice=True, seed=k), which krige all new units in one hmsc_krige call, bring them to the host
and send them back (held to tests/krige_oracle.py, summary_reference.py and community_reference.py
by test_gpu_krige.py, test_gpu_predict_summary.py and test_gpu_community.py).

predictMap makes the same kriged factors slab by slab on the device: every value of a slab's Eta
table is a sum over the fitted units in index order or a draw of (unit, factor, level, sample)
counters, and a cell's counters are those of its place in the whole map.  So every comparison here
is for equal doubles: with the yardstick, between slab sizes and between repeats.

Model (map_cases.py): 70 fitted spatial units (two 64-row blocks), 37 species (two 32-species
tiles), 9 samples of 2 or 3 factors (zero padding), a spatial and a non-spatial level, normal /
probit / Poisson columns with YScalePar, alpha indices at a = 0 and three positive grid values; 150
new sites from prepareGradient: every row its own new spatial unit, all rows one "new_unit".
"""
import functools

import numpy as np
import pandas as pd
import pytest

import map_cases as MC
from helpers import H
from hmsc_amd._lib import HmscNativeError

pytestmark = pytest.mark.gpu

PROBS = (0.1, 0.5)
SLABS = (64, 128, 0)
MODES = {"mean": ("Full", dict(predictEtaMean=True)), "field": ("Full", dict(predictEtaMeanField=True)),
         "nngp": ("NNGP", dict())}


@functools.lru_cache(maxsize=None)
def _model(method):
    hM = MC.model(method, **(dict(nNeighbours=5) if method == "NNGP" else {}))
    return hM, MC.posterior(hM)


def _weights(hM):
    w = np.zeros(hM.ns)
    w[4] = 1.0
    return {"sp4": w}


def _yardstick(hM, post, G, seed, expected, **kw):
    kw = dict(post=post, Gradient=G, krigeDevice=True, seed=seed, expected=expected, **kw)
    return dict(cells=H.predictSummary(hM, probs=PROBS, **kw),
                community=H.predictCommunity(hM, measures=("S", "T"), weights=_weights(hM), **kw))


def _map(hM, post, G, seed, expected, slab_rows, cells=True, **kw):
    return H.predictMap(hM, post=post, Gradient=G, seed=seed, expected=expected, cells=cells, probs=PROBS,
                        measures=("S", "T"), weights=_weights(hM), slab_rows=slab_rows, **kw)


def _assert_same(got, ref, what):
    for part, keys in (("cells", ("n", "occ", "mean", "quantiles", "median", "probs")),
                       ("community", ("n", "mean", "quantiles", "probs"))):
        if ref[part] is None or got[part] is None:
            assert got[part] is None and ref[part] is None, (what, part)
            continue
        for key in keys:
            a, b = np.asarray(got[part][key]), np.asarray(ref[part][key])
            assert a.shape == b.shape, (what, part, key, a.shape, b.shape)
            bad = ~((a == b) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a != b
            assert not bad.any(), (f"{what}: {part}[{key}] differs in {int(bad.sum())} of {bad.size} entries, first at "
                                   f"{np.unravel_index(int(np.argmax(bad)), bad.shape)}")
    if ref["community"] is not None:
        assert got["community"]["columns"] == ref["community"]["columns"]


def _assert_all_slabs(hM, post, G, seed, expected, what, **kw):
    ref = _yardstick(hM, post, G, seed, expected, **kw)
    assert np.all(ref["community"]["n"] > 0) and np.all(np.isfinite(ref["cells"]["mean"]))
    first = None
    for rows in SLABS:
        got = _map(hM, post, G, seed, expected, rows, **kw)
        _assert_same(got, ref, f"{what} slab_rows={rows} against the yardstick")
        again = _map(hM, post, G, seed, expected, rows, **kw)
        _assert_same(again, got, f"{what} slab_rows={rows} repeated")
        if first is not None:
            _assert_same(got, first, f"{what} slab_rows={rows} against slab_rows={SLABS[0]}")
        first = first or got
    return ref


@pytest.mark.parametrize("expected", [True, False], ids=["expected", "draws"])
@pytest.mark.parametrize("mode", list(MODES))
def test_agreement(mode, expected):
    """predictEtaMean, predictEtaMeanField and NNGP's conditional, expected values and draws, in slabs
    of 64, 128 and all 150 rows: the yardstick's doubles, whatever the slab, twice."""
    method, kw = MODES[mode]
    hM, post = _model(method)
    G = MC.grid(hM, 150)
    _assert_all_slabs(hM, post, G, 31 + len(mode), expected, f"{mode} expected={expected}", **kw)


@pytest.mark.parametrize("mode", ["mean", "field", "nngp"])
def test_shared_spatial_units(mode):
    """Rows 20 and 120 share one new spatial unit (and 3 and 149 another): the unit is kriged in two
    slabs of 64 rows, to the same doubles."""
    method, kw = MODES[mode]
    hM, post = _model(method)
    G = MC.shared_units(MC.grid(hM, 150), ((20, 120), (3, 149)))
    assert G["studyDesignNew"]["plot"].nunique() == 148
    _assert_all_slabs(hM, post, G, 77, False, f"shared units {mode}", **kw)


def test_full_joint_draw():
    """'Full' draws the new units jointly: served when they fit one slab, refused by name otherwise."""
    hM, post = _model("Full")
    G = MC.grid(hM, 40)
    for expected in (True, False):
        ref = _yardstick(hM, post, G, 5, expected)
        for rows in (0, 64):
            _assert_same(_map(hM, post, G, 5, expected, rows), ref, f"Full nn=40 slab_rows={rows} expected={expected}")
    with pytest.raises(NotImplementedError, match="predictEtaMean or predictEtaMeanField"):
        _map(hM, post, MC.grid(hM, 150), 5, True, 64)


def test_known_units_mixed_with_new():
    """Prediction rows at fitted units (gathered from the posterior Eta) mixed with new ones in both
    levels, rows in no order, slabs of 64: the local Pi and the units' places in the slab's table."""
    hM, post = _model("Full")
    rng = np.random.default_rng(3)
    n_new, rows = 30, 100
    names = [f"p{k:03d}" for k in range(MC.NP)] + [f"q{k:03d}" for k in range(n_new)]
    rl = hM.rL[0].copy()
    rl.s = np.vstack([np.asarray(rl.s, dtype=np.float64), rng.random((n_new, 2))])
    rl["sNames"] = names
    rl.pi = names
    rl.N = len(names)
    sites = [f"u{k:02d}" for k in range(MC.NSITE)] + ["z1", "z2"]
    sd = pd.DataFrame({"plot": rng.choice(names, rows), "site": rng.choice(sites, rows)})
    X = np.column_stack([np.ones(rows), rng.standard_normal((rows, 2))])
    kw = dict(X=X, studyDesign=sd, ranLevels={"plot": rl, "site": hM.rL[1]}, seed=9, expected=False,
              predictEtaMeanField=True)
    ref = dict(cells=H.predictSummary(hM, post=post, krigeDevice=True, probs=PROBS, **kw),
               community=H.predictCommunity(hM, post=post, krigeDevice=True, measures=("S",), **kw))
    for slab_rows in (64, 0):
        got = H.predictMap(hM, post=post, probs=PROBS, measures=("S",), slab_rows=slab_rows, **kw)
        _assert_same(got, ref, f"known and new units, slab_rows={slab_rows}")


def test_spatial_level_without_new_units():
    """100 rows whose spatial units are all fitted ones (the level's kriging plan is empty: its table is
    gathered from the posterior Eta) beside a non-spatial level with new units, predictEtaMeanField."""
    hM, post = _model("Full")
    rng = np.random.default_rng(13)
    rows = 100
    names = [f"p{k:03d}" for k in range(MC.NP)]
    sites = [f"u{k:02d}" for k in range(MC.NSITE)] + ["z1", "z2"]
    sd = pd.DataFrame({"plot": rng.choice(names, rows), "site": rng.choice(sites, rows)})
    assert set(sd["site"]) & {"z1", "z2"}
    X = np.column_stack([np.ones(rows), rng.standard_normal((rows, 2))])
    kw = dict(X=X, studyDesign=sd, ranLevels={"plot": hM.rL[0], "site": hM.rL[1]}, seed=19, expected=False,
              predictEtaMeanField=True)
    ref = dict(cells=H.predictSummary(hM, post=post, krigeDevice=True, probs=PROBS, **kw),
               community=H.predictCommunity(hM, post=post, krigeDevice=True, measures=("S",), **kw))
    for slab_rows in (64, 0):
        got = H.predictMap(hM, post=post, probs=PROBS, measures=("S",), slab_rows=slab_rows, **kw)
        _assert_same(got, ref, f"spatial level without new units, slab_rows={slab_rows}")


def test_all_normal_model_two_transforms():
    """An all-normal model: "T" takes exp of the predictions and "S" does not, two community blocks
    of one call."""
    hM = MC.model(families=(1,), ns=6)
    post = MC.posterior(hM)
    G = MC.grid(hM, 70)
    ref = _yardstick(hM, post, G, 12, False, predictEtaMean=True)
    _assert_same(_map(hM, post, G, 12, False, 64, predictEtaMean=True), ref, "all normal")


def test_other_refusals():
    hM, post = _model("Full")
    G = MC.grid(hM, 150)
    hG = MC.model("GPP", sKnot="auto")
    with pytest.raises(NotImplementedError, match="GPP kriging on the device is not implemented"):
        _map(hG, MC.posterior(hG), MC.grid(hG, 150), 1, True, 64)
    hX = MC.model(xdim=True)
    with pytest.raises(NotImplementedError, match="xData"):
        _map(hX, MC.posterior(hX), MC.grid(hX, 150), 1, True, 64, predictEtaMean=True)
    with pytest.raises(HmscNativeError, match=r"need (\d+) bytes of device memory, the budget \(factor_bytes\) is 1024 bytes"):
        _map(hM, post, G, 1, True, 64, predictEtaMean=True, factor_bytes=1024)
    # the refused call left nothing behind, and the next one is served
    live = np.zeros(4, dtype=np.int64)
    from hmsc_amd import _lib as L
    L.check(L.lib().hmsc_debug_live_resources(live.ctypes.data_as(L.C.POINTER(L.C.c_int64))))
    before = live.copy()
    _map(hM, post, G, 1, True, 64, predictEtaMean=True)
    L.check(L.lib().hmsc_debug_live_resources(live.ctypes.data_as(L.C.POINTER(L.C.c_int64))))
    assert np.array_equal(live, before)


def test_cells_false_and_timing():
    hM, post = _model("Full")
    G = MC.grid(hM, 150)
    full = _map(hM, post, G, 8, False, 64, predictEtaMeanField=True)
    part = _map(hM, post, G, 8, False, 64, cells=False, predictEtaMeanField=True)
    assert part["cells"] is None
    _assert_same(dict(cells=None, community=part["community"]), dict(cells=None, community=full["community"]), "cells=False")
    from hmsc_amd.gradient import mapTiming
    t = mapTiming()
    assert list(t) == ["plan", "K12", "trsm", "mean", "assemble", "summary", "community", "statistics", "copy"]
    assert t["summary"] == 0.0 and all(t[k] > 0.0 for k in ("plan", "K12", "trsm", "mean", "assemble", "community"))
