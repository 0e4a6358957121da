"""predictMap's host side (hmsc_amd/gradient.py) without a GPU: the slab planner on hand-made
designs, the slab size rule, and every refusal that is decided before the device call -- raised
with the library unloadable."""
import numpy as np
import pytest

import map_cases as MC
from helpers import H
from hmsc_amd import _lib
from hmsc_amd.gradient import map_slab_plan, map_slab_rows


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the device library fails the test."""
    def refuse():
        raise AssertionError("the device library was loaded")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_planner_boundaries_units_and_local_pi():
    """Two levels over 7 rows in slabs of 3: level 0 has 4 fitted units and each row's own new unit
    except rows 1 and 5, which share new unit 1, and row 6 at fitted unit 2; level 1 has 2 fitted
    units and one new unit for every row but the first."""
    u0 = np.array([4 + 0, 4 + 1, 4 + 2, 4 + 3, 4 + 4, 4 + 1, 2])
    u1 = np.array([1, 2, 2, 2, 2, 2, 2])
    plan = map_slab_plan([u0, u1], [4, 2], 3)
    assert [(s["row0"], s["rows"]) for s in plan] == [(0, 3), (3, 3), (6, 1)]
    assert [s["units"][0].tolist() for s in plan] == [[4, 5, 6], [5, 7, 8], [2]]
    assert [s["new"][0].tolist() for s in plan] == [[0, 1, 2], [1, 3, 4], []]        # unit 1 in two slabs
    assert [s["units"][1].tolist() for s in plan] == [[1, 2], [2], [2]]
    assert [s["new"][1].tolist() for s in plan] == [[0], [0], [0]]                  # "new_unit" in every slab
    assert plan[0]["Pi"].tolist() == [[0, 0], [1, 1], [2, 1]]
    assert plan[1]["Pi"].tolist() == [[1, 0], [2, 0], [0, 0]]                       # row 5 -> unit 5, first of its slab
    assert plan[2]["Pi"].tolist() == [[0, 0]]
    for s in plan:                                                                    # Pi leads back to the rows' units
        for r, u in enumerate((u0, u1)):
            assert np.array_equal(s["units"][r][s["Pi"][:, r]], u[s["row0"]:s["row0"] + s["rows"]])


def test_planner_fitted_units_come_first_and_rows_in_any_order():
    u = np.array([9, 0, 7, 3, 3, 9, 5, 0])
    plan = map_slab_plan([u], [6], 8)
    assert len(plan) == 1 and plan[0]["units"][0].tolist() == [0, 3, 5, 7, 9]
    assert plan[0]["new"][0].tolist() == [1, 3]
    assert plan[0]["Pi"][:, 0].tolist() == [4, 0, 3, 1, 1, 4, 2, 0]
    one = map_slab_plan([u], [6], 1)
    assert [s["units"][0].tolist() for s in one] == [[v] for v in u]
    with pytest.raises(ValueError, match="slab_rows"):
        map_slab_plan([u], [6], 0)


def test_planner_on_a_prepare_gradient_design():
    """150 rows of prepareGradient in slabs of 64: every slab its own rows' new spatial units with
    their global indices, and the one non-spatial new unit in each."""
    u0, u1 = MC.NP + np.arange(150), np.full(150, MC.NSITE)
    plan = map_slab_plan([u0, u1], [MC.NP, MC.NSITE], 64)
    assert [s["rows"] for s in plan] == [64, 64, 22]
    for s in plan:
        assert np.array_equal(s["new"][0], np.arange(s["row0"], s["row0"] + s["rows"]))
        assert s["new"][1].tolist() == [0] and np.all(s["Pi"][:, 1] == 0)
        assert np.array_equal(s["Pi"][:, 0], np.arange(s["rows"]))


def test_slab_rows_rule():
    assert map_slab_rows(150, 9, 10, slab_rows=64) == 64
    assert map_slab_rows(150, 9, 10, slab_rows=1000) == 150
    assert map_slab_rows(10 ** 6, 200, 10) == (1 << 30) // (200 * 8 * 10) // 64 * 64       # 1 GiB by default
    assert map_slab_rows(10 ** 6, 200, 10, scratch_bytes=200 * 8 * 10 * 64 * 3 + 5) == 192
    assert map_slab_rows(10 ** 6, 1 << 20, 1, scratch_bytes=1 << 40) == 8 * 64              # 2^23 workgroups
    with pytest.raises(ValueError, match=r"needs 1024000 bytes of scratch, scratch_bytes allows 1000"):
        map_slab_rows(10 ** 6, 200, 10, scratch_bytes=1000)


def _call(hM, post, G, **kw):
    return H.predictMap(hM, post=post, Gradient=G, measures=("S",), **kw)


def test_refusals_before_any_device_call(no_library):
    hM = MC.model()
    post = MC.posterior(hM)
    G = MC.grid(hM, 150)
    hX = MC.model(xdim=True)
    with pytest.raises(NotImplementedError, match=r"level site has xData .*xDim > 0"):
        _call(hX, MC.posterior(hX), MC.grid(hX, 20), predictEtaMean=True)
    hG = MC.model("GPP", sKnot="auto")
    with pytest.raises(NotImplementedError, match="GPP kriging on the device is not implemented"):
        _call(hG, MC.posterior(hG), MC.grid(hG, 20), seed=1)
    with pytest.raises(NotImplementedError, match=r"'Full' joint draw of level plot needs all its 150 new units in one slab "
                                                  r"\(64 rows\); use predictEtaMean or predictEtaMeanField"):
        _call(hM, post, G, seed=1, slab_rows=64)
    with pytest.raises(TypeError, match="Yc"):
        _call(hM, post, G, seed=1, predictEtaMean=True, Yc=np.zeros((150, hM.ns)))
    with pytest.raises(ValueError, match="give seed"):
        _call(hM, post, G, predictEtaMeanField=True)
    with pytest.raises(ValueError, match="give seed"):
        _call(hM, post, G, predictEtaMean=True, expected=False)
    with pytest.raises(ValueError, match="cannot be simultaneously TRUE"):
        _call(hM, post, G, seed=1, predictEtaMean=True, predictEtaMeanField=True)
    with pytest.raises(ValueError, match="nothing asked for"):
        H.predictMap(hM, post=post, Gradient=G, predictEtaMean=True, cells=False)
    with pytest.raises(TypeError, match="unexpected"):
        _call(hM, post, G, seed=1, krigeDevice=True)


def test_served_calls_reach_the_device(no_library):
    """What is not refused goes on to the library: the means without a seed, and a 'Full' draw whose
    new units fit one slab."""
    hM = MC.model()
    post = MC.posterior(hM)
    with pytest.raises(AssertionError, match="library was loaded"):
        _call(hM, post, MC.grid(hM, 150), predictEtaMean=True, slab_rows=64)
    with pytest.raises(AssertionError, match="library was loaded"):
        _call(hM, post, MC.grid(hM, 40), seed=3, slab_rows=64)
