"""Host side of the Omega convergence diagnostics (hmsc_amd/post.py; no device):
  * gelman_from_moments is gelman_diag's arithmetic from the per-chain moments, bit for bit;
  * omegaDiagnostics refuses unequal chains and fewer than 3 samples before any device call;
  * convergenceDiagnostics names and shapes its outputs (device calls replaced by numpy).
"""
import types

import numpy as np
import pytest

import hmsc_amd as H
from hmsc_amd import post as P
from oracle import post_oracle as O


@pytest.mark.parametrize("m", [2, 4])
def test_gelman_from_moments_is_gelman_diag(m):
    rng = np.random.default_rng(10 + m)
    n, p = 57, 23
    chains = [rng.standard_normal((n, p)) * (1 + 0.1 * c) + 0.05 * c for c in range(m)]
    chains[0][:, 3] = 2.0                                  # a constant column in one chain
    X = np.stack(chains)
    with np.errstate(all="ignore"):
        point, upper = H.gelman_diag(chains)
        p2, u2 = H.gelman_from_moments(X.mean(1), X.var(1, ddof=1), n)
    np.testing.assert_array_equal(p2, point)
    np.testing.assert_array_equal(u2, upper)
    assert point.shape == (p,) and np.isfinite(np.delete(point, 3)).all()
    # the moments may carry the parameter's shape
    p3, u3 = H.gelman_from_moments(X.mean(1).reshape(m, 1, p), X.var(1, ddof=1).reshape(m, 1, p), n, confidence=0.9)
    assert p3.shape == (1, p)
    np.testing.assert_array_equal(p3[0], point)
    assert np.all(np.delete(u3[0], 3) <= np.delete(upper, 3))


def _stub(lens, ns=4, nc=2, nt=2, nr=2, nf=2, phylo=False, seed=0):
    rng = np.random.default_rng(seed)

    def sample():
        s = dict(Beta=rng.standard_normal((nc, ns)), Gamma=rng.standard_normal((nc, nt)),
                 V=rng.standard_normal((nc, nc)), sigma=rng.random(ns) + 0.5,
                 Lambda=[rng.standard_normal((nf, ns)) for _ in range(nr)])
        if phylo:
            s["rho"] = rng.random()
        return s
    return types.SimpleNamespace(ns=ns, nc=nc, nt=nt, nr=nr, C=np.eye(ns) if phylo else None,
                                 spNames=[f"sp{j}" for j in range(ns)], covNames=[f"x{k}" for k in range(nc)],
                                 trNames=[f"t{k}" for k in range(nt)],
                                 postList=[[sample() for _ in range(n)] for n in lens])


def _no_device(*a, **k):
    raise AssertionError("the device was called")


def test_omega_diagnostics_refusals_come_before_the_device(monkeypatch):
    monkeypatch.setattr(P, "_omega_diag_device", _no_device)
    with pytest.raises(ValueError, match=r"unequal lengths.*\[10, 9\]"):
        H.omegaDiagnostics(_stub([10, 9]))
    with pytest.raises(ValueError, match=r"unequal lengths.*\[2, 3\]"):
        H.omegaDiagnostics(_stub([10, 12]), start=2, thin=5)     # samples 2, 7 and 2, 7, 12
    with pytest.raises(ValueError, match=r"2 samples per chain.*at least 3"):
        H.omegaDiagnostics(_stub([2, 2]))
    with pytest.raises(ValueError, match=r"2 samples per chain.*at least 3"):
        H.omegaDiagnostics(_stub([12, 12]), start=3, thin=5)     # samples 3, 8 of each chain
    with pytest.raises(ValueError, match=r"at least 3"):
        H.omegaDiagnostics(_stub([8]), r=2, start=7)


def _numpy_omega_diag(lam, nf, device=None, scratch_bytes=0, series=False):
    """_omega_diag_device restated: Omega materialised, the oracle's ESS."""
    m, n, ns, nfm = lam.shape
    ess, mean, var = (np.zeros((m, ns, ns)) for _ in range(3))
    order = np.zeros((m, ns, ns), dtype=np.int32)
    for c in range(m):
        om = np.stack([lam[c, s, :, :nf[c, s]] @ lam[c, s, :, :nf[c, s]].T for s in range(n)]).reshape(n, -1)
        ess[c] = O.effectiveSize(om).reshape(ns, ns)
        order[c] = O.spectrum0_ar(om)[1].reshape(ns, ns)
        mean[c], var[c] = om.mean(0).reshape(ns, ns), om.var(0, ddof=1).reshape(ns, ns)
    return ess, mean, var, order, None


def _numpy_ess(x, device=None):
    return O.effectiveSize(x), O.spectrum0_ar(x)[1]


@pytest.mark.parametrize("phylo", [False, True])
def test_convergence_diagnostics_names_and_shapes(monkeypatch, phylo):
    monkeypatch.setattr(P, "_omega_diag_device", _numpy_omega_diag)
    monkeypatch.setattr(P, "_ess_device", _numpy_ess)
    hM = _stub([30, 30], ns=5, nc=3, nt=2, nr=2, phylo=phylo, seed=4)
    d = H.convergenceDiagnostics(hM, start=3, thin=2)
    want = ["Beta", "Gamma", "V", "Sigma"] + (["Rho"] if phylo else []) + ["Omega"]
    assert list(d) == want
    shapes = dict(Beta=(3, 5), Gamma=(3, 2), V=(3, 3), Sigma=(5,), Rho=(1,))
    for p in want[:-1]:
        assert set(d[p]) == {"ess", "psrf", "psrf_upper"}
        for k in d[p]:
            assert d[p][k].shape == shapes[p], (p, k)
    assert len(d["Omega"]) == 2
    for o in d["Omega"]:
        assert set(o) == {"ess", "psrf", "psrf_upper"}
        assert all(o[k].shape == (5, 5) for k in o)
    # the values are those of the coda route on the same samples, entry by entry
    coda, _ = H.convertToCodaObject(hM, start=3, Eta=False, Lambda=False, Alpha=False, Psi=False, Delta=False)
    beta = [c[::2] for c in coda["Beta"]]
    assert beta[0].shape == (14, 15)
    np.testing.assert_array_equal(d["Beta"]["ess"], O.effectiveSize(beta).reshape((3, 5), order="F"))
    np.testing.assert_array_equal(d["Beta"]["psrf"], H.gelman_diag(beta)[0].reshape((3, 5), order="F"))
    om = [c[::2] for c in coda["Omega"][1]]
    np.testing.assert_allclose(d["Omega"][1]["ess"], O.effectiveSize(om).reshape(5, 5), rtol=1e-12)
    np.testing.assert_allclose(d["Omega"][1]["psrf"], H.gelman_diag(om)[0].reshape(5, 5), rtol=1e-10)
    np.testing.assert_allclose(d["Omega"][1]["psrf_upper"], H.gelman_diag(om)[1].reshape(5, 5), rtol=1e-10)
    # a subset of the parameters, one chain: no PSRF
    hM.postList = hM.postList[:1]
    d1 = H.convergenceDiagnostics(hM, parameters=("Sigma", "Omega"))
    assert list(d1) == ["Sigma", "Omega"]
    assert d1["Sigma"]["psrf"] is None and d1["Omega"][0]["psrf"] is None and d1["Omega"][0]["psrf_upper"] is None
    assert d1["Sigma"]["ess"].shape == (5,) and d1["Omega"][0]["ess"].shape == (5, 5)
    with pytest.raises(ValueError, match="unknown parameters"):
        H.convergenceDiagnostics(hM, parameters=("Beta", "Lambda"))


def test_f_quantile_of_the_upper_limit_is_exact_and_smooth():
    """gelman_diag's F quantile against a 40-digit evaluation, from a denominator df of 0.5 to the
    1e10 ... 1e14 of chains whose variances nearly agree, where scipy's stats.f.ppf is off by
    d2 * 1e-16 and jumps by as much between neighbouring d2; and its limit qchisq / d1."""
    import mpmath as mp
    from scipy import stats
    mp.mp.dps = 40
    for d1 in (1, 2, 3, 7):
        for d2 in (0.5, 1.0, 2.0, 3.7, 10.0, 150.0, 1e4, 1e7, 2.394e10, 1e14):
            for tail in (0.025, 0.05):
                q = float(P._f_upper_quantile(tail, d1, d2))
                t = mp.findroot(lambda x: mp.betainc(mp.mpf(d1) / 2, mp.mpf(d2) / 2, d1 * x / (d1 * x + d2), 1,
                                                     regularized=True) - tail, q)
                assert abs(float(q / t - 1)) < 2e-15, (d1, d2, tail)
                if d2 >= 2:   # there |dlog q / dlog d2| < 3: one ulp of d2 moves q by < 1e-15, plus the two 2e-15 above
                    q1 = float(P._f_upper_quantile(tail, d1, np.nextafter(d2, np.inf)))
                    assert abs(q1 / q - 1) < 5e-15, (d1, d2, tail)
        assert abs(float(P._f_upper_quantile(0.025, d1, 1e14)) / (stats.chi2.ppf(0.975, d1) / d1) - 1) < 1e-13
    d2 = np.logspace(0, 4, 500)                                # the ordinary range: scipy's own value
    np.testing.assert_allclose(P._f_upper_quantile(0.025, 1, d2), stats.f.ppf(0.975, 1, d2), rtol=1e-11)
    with np.errstate(all="ignore"):
        assert np.isnan(P._f_upper_quantile(0.025, 1, np.array([np.nan, np.inf, 0.0]))).all()    # as stats.f.ppf
