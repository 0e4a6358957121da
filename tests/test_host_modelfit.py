"""The longdouble restatement of evaluateModelFit's measures (tests/modelfit_reference.py) against the
host evaluateModelFit, on the cases the device tests use, and the argument refusals of
evaluateModelFit(device=) that are raised before any device call.  Runs without a GPU."""
import numpy as np
import pytest

import modelfit_reference as MR
from helpers import H


def _host(Y, m, pO, family):
    with np.errstate(all="ignore"):
        return H.evaluateModelFit(MR.Stub(Y, family), summary=MR.as_summary(m, pO))


def _assert_restatement_matches_host(Y, m, pO, family, what):
    host = _host(Y, m, pO, family)
    val, bnd = MR.reference(Y, m, pO, family)
    assert set(host) == set(MR.as_dict(val, family))
    worst = MR.assert_within(host, val, bnd, what)        # AUC, O.AUC: equality; NaN / inf pattern identical
    print(f"{what}: host / bound worst ratios " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return val


@pytest.mark.parametrize("ny", [1, 2, 3, 63, 64, 65, 150])
def test_restatement_against_host_mixed(ny):
    Y, m, pO = MR.mixed_case(ny)
    val = _assert_restatement_matches_host(Y, m, pO, MR.MIXED_FAMILY, f"mixed ny = {ny}")
    if ny >= 63:   # what the device test relies on: every measure of every column's family is a number
        for j, f in enumerate(MR.MIXED_FAMILY):
            for key in ("RMSE",) + MR.FAMILY_KEYS[int(f)]:
                assert np.isfinite(val[MR.KEYS.index(key), j]), (key, j)


def test_restatement_against_host_long_column():
    family = np.array([1, 2, 3], dtype=np.int32)
    Y, m, pO = MR.mixed_case(40000, family)
    val = _assert_restatement_matches_host(Y, m, pO, family, "ny = 40000")
    assert np.isfinite(val[MR.KEYS.index("AUC"), 1]) and np.isfinite(val[MR.KEYS.index("C.SR2"), 2])


def test_restatement_against_host_edge_rows():
    Y, m, pO, family = MR.edge_case()
    val = _assert_restatement_matches_host(Y, m, pO, family, "edge rows")
    k = MR.KEYS.index
    # the cases are what they claim to be
    assert np.isnan(val[k("AUC"), 1]) and np.isnan(val[k("TjurR2"), 1])            # NaN in m reaches both
    assert np.isfinite(val[k("AUC"), 3])                                           # ... unless Y is NA there
    assert np.isnan(val[k("AUC"), 4]) and np.isnan(val[k("TjurR2"), 4])            # single class
    assert val[k("AUC"), 5] == 0.5 and val[k("TjurR2"), 5] == 0.0                  # constant m
    assert np.isfinite(val[k("AUC"), 7]) and np.isinf(val[k("RMSE"), 7])           # +inf in m
    assert np.isnan(val[k("R2"), 10]) and np.isnan(val[k("R2"), 11])               # constant m, +inf in m
    assert np.isinf(val[k("C.RMSE"), 13]) and np.isfinite(val[k("C.SR2"), 13])     # m / pO = +inf is data
    assert np.all(np.isnan(val[[k("C.SR2"), k("C.RMSE"), k("O.AUC")], 16]))        # zeros only
    assert val[k("O.TjurR2"), 18] == 0.0 and val[k("O.AUC"), 18] == 0.5            # constant pO


def test_average_ranks_ties_and_signed_zero():
    x = np.array([0.0, -0.0, 1.0, np.inf, 1.0, -np.inf, 1.0])
    assert np.array_equal(MR.average_ranks(x), [2.5, 2.5, 5.0, 7.0, 5.0, 1.0, 5.0])
    assert np.all(np.isnan(MR.average_ranks([1.0, np.nan])))


def test_device_argument_refusals_need_no_device(monkeypatch):
    from hmsc_amd import _lib

    def no_device():
        raise AssertionError("the device library was loaded")
    monkeypatch.setattr(_lib, "lib", no_device)
    Y, m, pO = MR.mixed_case(5)
    hM, sm = MR.Stub(Y, MR.MIXED_FAMILY), MR.as_summary(m, pO)
    with pytest.raises(ValueError, match="exactly one"):
        H.evaluateModelFit(hM, device=0)
    with pytest.raises(ValueError, match="exactly one"):
        H.evaluateModelFit(hM, np.zeros((5, 9, 2)), summary=sm, device=0)
    for bad in (-1, "0", 0.0, True):
        with pytest.raises(ValueError, match="device index"):
            H.evaluateModelFit(hM, summary=sm, device=bad)
    with pytest.raises(ValueError, match="negative"):
        H.evaluateModelFit(hM, summary=sm, device=0, chunk_rows=-1)
    with pytest.raises(ValueError, match="negative"):
        H.evaluateModelFit(hM, summary=sm, device=0, scratch_bytes=-1)
    from hmsc_amd.predict import model_fit_device
    with pytest.raises(ValueError, match="do not agree"):
        model_fit_device(Y, m[:4], pO, MR.MIXED_FAMILY)
    with pytest.raises(ValueError, match="do not agree"):
        model_fit_device(Y, m, pO, MR.MIXED_FAMILY[:8])
    with pytest.raises(ValueError, match="not Y's shape"):
        model_fit_device(Y, m, pO[:, :8], MR.MIXED_FAMILY)
    # the host path is untouched by the new keywords' defaults
    with np.errstate(all="ignore"):
        assert set(H.evaluateModelFit(hM, summary=sm)) == set(MR.KEYS)
