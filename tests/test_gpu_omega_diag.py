"""Omega convergence diagnostics on the device (hmsc_omega_diagnostics, hmsc_amd/csrc/post.hip;
hmsc_amd.omegaDiagnostics / convergenceDiagnostics) held to
  * a np.longdouble sum for the series w_ij(s) = sum_{h < nf} lambda_hi lambda_hj themselves
    (the debug output `series`), within the fma-chain bound 1.01 nf 2^-53 sum_h |l_hi| |l_hj|;
  * the verified hmsc_effective_size on those series, bit for bit (ESS and AR order), and numpy
    for the moments;
  * the numpy restatement of coda (oracle/post_oracle.py) on Omega materialised with numpy, by
    the ESS criterion of tests/test_gpu_post.py: orders equal on >= 99.9 % of the pair-chains,
    ESS within 1e-9 relative where they agree; PSRF within 1e-9 of gelman_diag.  The 0.1 % is a
    cap for near-ties of two AIC values, which summation order decides: each case first asserts
    on the host that the oracle's own AIC gap (second smallest minus smallest) is below 1e-6 on
    at most 0.1 % of its columns.
Lambda is AR(1) over the samples (phi = 0.6), so the series are autocorrelated.
"""
import functools
import types

import numpy as np
import pytest

import hmsc_amd as H
from hmsc_amd import _lib as L
from hmsc_amd import post as P
from helpers import rel_err, synthetic_model
from oracle import post_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _ar1(n, p, phi, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, p))
    x = np.zeros((n, p))
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return x


@functools.lru_cache(maxsize=None)
def _case(ns, nfmax, n, m=2, seed=11, nf_lo=None, zero_species=None):
    """lam (m, n, ns, nfmax) -- each sample nfmax x ns column-major -- and nf (m, n), alternating
    nf_lo and nfmax over the samples.  Factors h >= nf keep their values: the call must ignore them."""
    lam = np.stack([_ar1(n, ns * nfmax, 0.6, seed + 100 * c).reshape(n, ns, nfmax) for c in range(m)])
    nf = np.full((m, n), nfmax, dtype=np.int32)
    if nf_lo is not None:
        nf[:, ::2] = nf_lo
    if zero_species is not None:
        lam[:, :, zero_species, :] = 0.0
    lam.setflags(write=False)
    nf.setflags(write=False)
    return lam, nf


def _pairs(ns):
    """(i, j) of the canonical pair order p = i + j (j + 1) / 2, i <= j."""
    jj, ii = np.tril_indices(ns)
    return ii, jj


def _masked(lam, nf):
    h = np.arange(lam.shape[3])
    return lam * (h[None, None, None, :] < nf[:, :, None, None])


@functools.lru_cache(maxsize=None)
def _reference(key):
    """Per case, once: Omega materialised with numpy for the pairs i <= j, (m, n, npairs), and
    the oracle's spec order / ESS per chain."""
    lam, nf = _case(*key)
    lm = _masked(lam, nf)
    ii, jj = _pairs(lam.shape[2])
    om = np.stack([np.einsum("sih,sjh->sij", c, c)[:, ii, jj] for c in lm])
    order = np.stack([O.spectrum0_ar(x)[1] for x in om])
    ess = np.stack([O.effectiveSize(x) for x in om])
    for a in (om, order, ess):
        a.setflags(write=False)
    return om, order, ess


def _xaic(x):
    """The AIC values spectrum0_ar chooses among (oracle/post_oracle.py:32-64), (order_max + 1, p)."""
    n, p = x.shape
    xc = x - x.mean(axis=0)
    omax = int(min(n - 1, np.floor(10 * np.log10(n))))
    r = np.stack([np.sum(xc[: n - k] * xc[k:], axis=0) / n for k in range(omax + 1)])
    r0 = np.where(r[0] > 0, r[0], 1.0)
    vars_ = np.empty((omax + 1, p))
    vars_[0] = r0
    a = np.zeros((omax + 1, p))
    v = r0.copy()
    for m in range(1, omax + 1):
        acc = r[m] - np.sum(a[1:m] * r[m - 1:0:-1], axis=0) if m > 1 else r[m].copy()
        k = acc / v
        a_new = a.copy()
        a_new[m] = k
        if m > 1:
            a_new[1:m] = a[1:m] - k * a[m - 1:0:-1]
        a = a_new
        v = v * (1 - k * k)
        vars_[m] = v
    with np.errstate(divide="ignore", invalid="ignore"):
        return n * np.log(vars_) + 2 * np.arange(omax + 1)[:, None] + 2.0


def _assert_oracle_is_decided(om, order_o, label):
    """The oracle's own choice is no near-tie on all but 0.1 % of the columns (host only)."""
    near = total = 0
    for x, o in zip(om, order_o):
        xa = _xaic(x)
        live = np.isfinite(xa).all(axis=0)
        np.testing.assert_array_equal(np.argmin(xa, axis=0)[live], o[live])   # it is the oracle's rule
        if xa.shape[0] > 1:
            s = np.sort(xa[:, live], axis=0)
            near += int(np.sum(s[1] - s[0] < 1e-6))
        total += x.shape[1]
    print(f"{label}: oracle AIC gap < 1e-6 on {near} of {total} pair-chains")
    assert near <= 1e-3 * total


def _hold_to_oracle(key, res, label):
    """Test 3's criterion on all pairs of a case; res = (ess, mean, var, order) per chain (m, ns, ns)."""
    lam, nf = _case(*key)
    m, n, ns = lam.shape[:3]
    om, order_o, ess_o = _reference(key)
    _assert_oracle_is_decided(om, order_o, label)
    ii, jj = _pairs(ns)
    ess_d, order_d = res[0][:, ii, jj], res[3][:, ii, jj]
    same = order_o == order_d
    ok = same & (ess_o > 0)
    worst = rel_err(ess_d[ok], ess_o[ok]) if ok.any() else 0.0
    print(f"{label}: AR order equal on {same.mean():.6f} of {same.size} pair-chains; worst ESS rel err {worst:.3e}")
    assert same.mean() >= 0.999, np.argwhere(~same)
    assert worst < 1e-9
    with np.errstate(all="ignore"):
        pd, _ = H.gelman_from_moments(res[1][:, ii, jj], res[2][:, ii, jj], n)
        po, _ = H.gelman_diag(list(om))
    fin = np.isfinite(po)
    print(f"{label}: worst PSRF rel err {np.max(np.abs(pd[fin] / po[fin] - 1), initial=0.0):.3e}")
    np.testing.assert_allclose(pd, po, rtol=1e-9, atol=0)


def _upper_one_ulp_noise(om, n):
    """How far gelman_diag's own upper limit moves, per column, when its moments move by one ulp
    (chain 0's variance or mean, up or down) or are formed in longdouble: the reference's own error."""
    xb, s2 = om.mean(1), om.var(1, ddof=1)
    X = om.astype(np.longdouble)
    variants = [(X.mean(1).astype(np.float64), X.var(1, ddof=1).astype(np.float64))]
    for d in (np.inf, -np.inf):
        a, b = s2.copy(), xb.copy()
        a[0], b[0] = np.nextafter(a[0], d), np.nextafter(b[0], d)
        variants += [(xb, a), (b, s2)]
    with np.errstate(all="ignore"):
        base = H.gelman_from_moments(xb, s2, n)[1]
        fin = np.isfinite(base)
        worst = np.zeros(base.shape)
        for vx, vs in variants:
            worst[fin] = np.maximum(worst[fin], np.abs(H.gelman_from_moments(vx, vs, n)[1][fin] / base[fin] - 1))
    return worst


def _hold_upper_to_gelman_diag(key, res, label):
    """psrf_upper within 1e-9 relative of gelman_diag on the materialised chains (the other half of
    test 3's PSRF criterion, kept apart from _hold_to_oracle: see test_psrf_upper_against_gelman_diag)."""
    lam, _ = _case(*key)
    n, ns = lam.shape[1:3]
    om = _reference(key)[0]
    ii, jj = _pairs(ns)
    with np.errstate(all="ignore"):
        _, ud = H.gelman_from_moments(res[1][:, ii, jj], res[2][:, ii, jj], n)
        _, uo = H.gelman_diag(list(om))
    fin = np.isfinite(uo)
    e, own = np.abs(ud[fin] / uo[fin] - 1), _upper_one_ulp_noise(om, n)
    print(f"{label}: psrf_upper worst rel err {e.max(initial=0.0):.3e}, above 1e-9 on {int((e > 1e-9).sum())} of "
          f"{e.size} pairs; gelman_diag's own upper limit under one ulp of its moments: worst "
          f"{own.max(initial=0.0):.3e}, above 1e-9 on {int((own > 1e-9).sum())}, above 1e-10 on {int((own > 1e-10).sum())}")
    np.testing.assert_allclose(ud, uo, rtol=1e-9, atol=0)


def _hold_to_ess_kernel(res, series, label=""):
    """Test 2: the call's per-chain ESS and order are hmsc_effective_size's on the returned series,
    bit for bit; mean and var are numpy's within n 2^-53 of the scale of what is summed (mean |x|
    for the mean, the variance itself -- a sum of squares -- for the variance)."""
    m, npairs, n = series.shape
    ns = res[0].shape[1]
    ii, jj = _pairs(ns)
    for c in range(m):
        x = series[c].T                                       # (n, npairs), a pair's samples contiguous
        np.testing.assert_array_equal(res[0][c, ii, jj], H.effectiveSize(x))
        np.testing.assert_array_equal(res[3][c, ii, jj], H.spectrum0_ar(x)[1])
        dm = np.abs(res[1][c, ii, jj] - x.mean(axis=0))
        dv = np.abs(res[2][c, ii, jj] - x.var(axis=0, ddof=1))
        assert np.all(dm <= n * U * np.abs(x).mean(axis=0))
        assert np.all(dv <= n * U * x.var(axis=0, ddof=1))


def _assert_symmetric(res):
    for a in res[:4]:
        np.testing.assert_array_equal(a, np.swapaxes(a, 1, 2))


K70 = (70, 3, 150, 2, 11, 2)          # ns = 70: one 64-block plus an edge of 6; nf alternates 2, 3


KZERO = (20, 3, 150, 2, 13, 2, 7)     # species 7: loadings 0 in every sample
EDGES = {"ns1": (1, 3, 150, 2, 21, 2), "ns64": (64, 3, 150, 2, 22, 2), "ns65": (65, 3, 150, 2, 23, 2),
         "nf1": (20, 1, 150, 2, 24), "n3": (20, 3, 3, 2, 25, 2), "n1100": (20, 3, 1100, 2, 26, 2)}
K200 = (200, 5, 200, 2, 31, 4)        # 20,100 pairs per chain, nf alternating 4, 5


@functools.lru_cache(maxsize=None)
def _run(key):
    """The device call of a case, once: (ess, mean, var, order, series)."""
    lam, nf = _case(*key)
    res = P._omega_diag_device(lam, nf, series=True)
    for a in res:
        a.setflags(write=False)
    return res


def _run70():
    return _run(K70)


def test_series_cell_by_cell():
    lam, nf = _case(*K70)
    series = _run70()[4]
    lm = np.abs(_masked(lam, nf)).astype(np.longdouble)
    ls = _masked(lam, nf).astype(np.longdouble)
    ii, jj = _pairs(70)
    worst = 0.0
    for c in range(lam.shape[0]):
        ref = np.einsum("sph,sph->ps", ls[c][:, ii, :], ls[c][:, jj, :])           # (npairs, n)
        mag = np.einsum("sph,sph->ps", lm[c][:, ii, :], lm[c][:, jj, :])
        bound = 1.01 * nf[c][None, :] * U * mag
        err = np.abs(series[c].astype(np.longdouble) - ref)
        live = bound > 0                                      # (every chain starts at Lambda = 0: w = 0 exactly)
        worst = max(worst, float(np.max(err[live] / bound[live])))
        assert np.all(err <= bound)
    print(f"series against longdouble: worst error / bound = {worst:.4f} over {series.size} elements")


def test_ess_is_the_verified_kernels():
    res = _run70()
    _hold_to_ess_kernel(res, res[4])
    assert res[3].max() > 0                                   # autocorrelated: the order is not trivially 0


def test_against_the_oracle_end_to_end():
    _hold_to_oracle(K70, _run70(), "ns=70")


def test_slab_and_repeat_independence():
    lam, nf = _case(*K70)
    base = _run70()
    pair_bytes = 150 * 8
    runs = [P._omega_diag_device(lam, nf, scratch_bytes=1000 * pair_bytes, series=True),   # columns 0-43, 44-61, 62-69
            P._omega_diag_device(lam, nf, scratch_bytes=70 * pair_bytes, series=True),     # the least: one column's pairs
            P._omega_diag_device(lam, nf, series=True), P._omega_diag_device(lam, nf, series=True)]
    for r in runs:
        for a, b in zip(r, base):
            np.testing.assert_array_equal(a, b)


def test_symmetry_and_the_degenerate_series():
    _assert_symmetric(_run70())
    key = KZERO
    lam, nf = _case(*key)
    res = _run(key)
    _assert_symmetric(res)
    assert np.all(res[0][:, 7, :] == 0.0) and np.all(res[0][:, :, 7] == 0.0)
    assert np.all(res[4][:, [i + j * (j + 1) // 2 for i, j in [(7, 7), (0, 7), (7, 19)]]] == 0.0)
    _hold_to_ess_kernel(res, res[4])
    with np.errstate(all="ignore"):
        pd, ud = H.gelman_from_moments(res[1], res[2], 150)
        om = _masked(lam, nf)
        po, uo = H.gelman_diag([np.einsum("sih,sjh->sij", c, c).reshape(150, -1) for c in om])
    np.testing.assert_array_equal(pd[7], po.reshape(20, 20)[7])       # what gelman_diag gives there (NaN: W = B = 0)
    np.testing.assert_array_equal(ud[:, 7], uo.reshape(20, 20)[:, 7])
    _hold_to_oracle(key, res, "zero species")


@pytest.mark.parametrize("key", list(EDGES.values()), ids=list(EDGES))
def test_edges_of_tiling_and_n(key):
    res = _run(key)
    _assert_symmetric(res)
    _hold_to_ess_kernel(res, res[4])
    _hold_to_oracle(key, res, f"ns={key[0]} nfmax={key[1]} n={key[2]}")
    if key[2] == 1100:
        assert int(np.floor(10 * np.log10(1100))) == 30 and res[3].max() <= 30


def _posterior(lam, nf, hM=None):
    hM = hM or types.SimpleNamespace(ns=lam.shape[2], nr=1)
    hM.postList = [[dict(Lambda=[lam[c, s, :, :nf[c, s]].T.copy()]) for s in range(lam.shape[1])]
                   for c in range(lam.shape[0])]
    return hM


def test_omega_diagnostics_at_a_useful_size():
    key = K200
    lam, nf = _case(*key)
    d = H.omegaDiagnostics(_posterior(lam, nf))
    assert d["ess"].shape == (200, 200) and d["mean"].shape == (2, 200, 200) and d["order"].dtype == np.int32
    _hold_to_oracle(key, _per_chain(lam, nf, d), "ns=200")
    with np.errstate(all="ignore"):
        pd, ud = H.gelman_from_moments(d["mean"], d["var"], 200)
    np.testing.assert_array_equal(d["psrf"], pd)
    np.testing.assert_array_equal(d["psrf_upper"], ud)
    # start / thin per chain: the same call on the kept samples
    d2 = H.omegaDiagnostics(_posterior(lam, nf), start=3, thin=2, scratch_bytes=1 << 20)
    r2 = P._omega_diag_device(lam[:, 2::2], nf[:, 2::2])
    np.testing.assert_array_equal(d2["ess"], r2[0][0] + r2[0][1])
    np.testing.assert_array_equal(d2["order"], r2[3])


def _per_chain(lam, nf, d):
    """omegaDiagnostics returns the ESS summed over chains; its per-chain parts for the oracle's
    criterion are the device call's, whose sum it must be."""
    r = _run(K200)
    np.testing.assert_array_equal(d["ess"], r[0][0] + r[0][1])
    for k, name in ((1, "mean"), (2, "var"), (3, "order")):
        np.testing.assert_array_equal(d[name], r[k])
    return r


@functools.lru_cache(maxsize=None)
def _synthetic():
    """tests/test_gpu_post.py's _synthetic_posterior shape (70 species, 2 levels, ragged nf, 2 chains
    of 30), with V and sigma, every entry AR(1) over the samples: (hM, convergenceDiagnostics(hM),
    the coda matrices, omegaDiagnostics per level)."""
    hM = synthetic_model(ny=400, ns=70, nc=5, nf=3, nt=3, nr=2, units=[400, 50], seed=3)
    S, ns, nc, nt = 30, hM.ns, hM.nc, hM.nt
    chains = []
    for c in range(2):
        B, G, V, sg = (_ar1(S, p, 0.6, 40 + 10 * c + k) for k, p in enumerate((nc * ns, nc * nt, nc * nc, ns)))
        l1, l2 = _ar1(S, 3 * ns, 0.6, 45 + 10 * c), _ar1(S, 3 * ns, 0.6, 46 + 10 * c) * 0.5
        chains.append([dict(Beta=B[s].reshape(nc, ns), Gamma=G[s].reshape(nc, nt), V=V[s].reshape(nc, nc),
                            sigma=np.exp(0.3 * sg[s]),
                            Lambda=[l1[s].reshape(3, ns)[:3 if s % 4 else 2], l2[s].reshape(3, ns)]) for s in range(S)])
    hM.postList = chains
    coda, _ = H.convertToCodaObject(hM, Eta=False, Lambda=False, Alpha=False, Psi=False, Delta=False)
    return hM, H.convergenceDiagnostics(hM), coda, [H.omegaDiagnostics(hM, r=r + 1) for r in range(2)]


def test_convergence_diagnostics_on_a_synthetic_posterior():
    hM, d, coda, omega = _synthetic()
    ns, nc, nt = hM.ns, hM.nc, hM.nt
    assert list(d) == ["Beta", "Gamma", "V", "Sigma", "Omega"] and len(d["Omega"]) == 2
    for p, shape in (("Beta", (nc, ns)), ("Gamma", (nc, nt)), ("V", (nc, nc)), ("Sigma", (ns,))):
        np.testing.assert_array_equal(d[p]["ess"], H.effectiveSize(coda[p]).reshape(shape, order="F"))
        point, upper = H.gelman_diag(coda[p])
        np.testing.assert_array_equal(d[p]["psrf"], point.reshape(shape, order="F"))
        np.testing.assert_array_equal(d[p]["psrf_upper"], upper.reshape(shape, order="F"))
    for r in range(2):
        om, o = coda["Omega"][r], omega[r]                    # 2 chains of (30, ns^2), crossprod by BLAS
        for k in ("ess", "psrf", "psrf_upper"):
            np.testing.assert_array_equal(d["Omega"][r][k], o[k])
        order_c = np.stack([H.spectrum0_ar(x)[1] for x in om]).reshape(2, ns, ns)
        same = (order_c == o["order"]).all(axis=0)
        assert same.mean() >= 0.999
        ess_c = H.effectiveSize(om).reshape(ns, ns)
        ok = same & (ess_c > 0)
        assert rel_err(o["ess"][ok], ess_c[ok]) < 1e-9
        np.testing.assert_allclose(o["psrf"], H.gelman_diag(om)[0].reshape(ns, ns), rtol=1e-9, atol=0)


UPPER = dict(ns70=K70, zero=KZERO, **EDGES, ns200=K200)


@pytest.mark.parametrize("key", list(UPPER.values()), ids=list(UPPER))
def test_psrf_upper_against_gelman_diag(key):
    """psrf_upper within 1e-9 relative of gelman_diag on the chains materialised with numpy, for every
    case of this file (the bound and the reference are the ones set for psrf beside it, which holds:
    _hold_to_oracle).

    The upper limit takes an F quantile at W_df = 2 W^2 / var_w, 1e10 and more for two chains whose
    variances nearly agree.  With scipy's stats.f.ppf there, this test missed at one pair each of
    ns = 70 (1.5e-08) and ns = 200 (1.3e-09), and gelman_diag fed its own moments one ulp apart moved
    by 2.9e-08 and 5.7e-09: f.ppf loses d2 * 1e-16 of the quantile.  post._f_upper_quantile replaced it
    (tests/test_host_omega_diag.py holds it to 40 digits); _upper_one_ulp_noise, printed with -s, is
    the reference's own movement that remains."""
    _hold_upper_to_gelman_diag(key, _run(key), f"ns={key[0]} nfmax={key[1]} n={key[2]}")


def test_psrf_upper_of_the_synthetic_posterior():
    """The same bound for convergenceDiagnostics' Omega against gelman_diag of convertToCodaObject's
    Omega matrices (see test_psrf_upper_against_gelman_diag for what decides it)."""
    hM, d, coda, omega = _synthetic()
    for r in range(2):
        upper = H.gelman_diag(coda["Omega"][r])[1].reshape(hM.ns, hM.ns)
        e = np.abs(omega[r]["psrf_upper"] / upper - 1)
        print(f"level {r + 1}: psrf_upper worst rel err {e.max():.3e}, above 1e-9 on {int((e > 1e-9).sum())} of {e.size}")
    for r in range(2):
        np.testing.assert_allclose(omega[r]["psrf_upper"], H.gelman_diag(coda["Omega"][r])[1].reshape(hM.ns, hM.ns),
                                   rtol=1e-9, atol=0)


def _raw(m, n, ns, nfmax, nf, scratch=0, lam=None):
    lam = np.zeros(max(1, min(m * n * ns * nfmax, 1 << 20))) if lam is None else lam
    nf = np.ascontiguousarray(nf, dtype=np.int32)
    out = [np.zeros(m * ns * ns) for _ in range(3)]
    L.check(L.lib().hmsc_omega_diagnostics(0, m, n, ns, nfmax, L.iptr(nf), L.fptr(lam), scratch, L.fptr(out[0]),
                                           L.fptr(out[1]), L.fptr(out[2]), None, None))


def test_the_abis_refusals():
    """Each is refused before Lambda or an output is touched."""
    with pytest.raises(L.HmscNativeError, match=r"n = 2 samples per chain, at least 3"):
        _raw(2, 2, 4, 2, np.full(4, 2))
    with pytest.raises(L.HmscNativeError, match=r"nfmax = 129 exceeds HMSC_KCAP = 128"):
        _raw(1, 5, 4, 129, np.full(5, 2))
    with pytest.raises(L.HmscNativeError, match=r"nf = 0 of sample 3 of chain 1 is outside 1\.\.nfmax = 2"):
        _raw(2, 5, 4, 2, [2, 2, 2, 2, 2, 2, 2, 2, 0, 2])
    with pytest.raises(L.HmscNativeError, match=r"nf = 3 of sample 0 of chain 0 is outside 1\.\.nfmax = 2"):
        _raw(2, 5, 4, 2, [3, 2, 2, 2, 2, 2, 2, 2, 2, 2])
    with pytest.raises(L.HmscNativeError, match=r"scratch_bytes = 159 is too small for one species column's pairs"):
        _raw(1, 5, 4, 2, np.full(5, 2), scratch=4 * 5 * 8 - 1)
    # 2 TB of Lambda per chain: beyond any device; both byte counts are reported
    with pytest.raises(L.HmscNativeError, match=r"needs \d{13,} bytes of device memory .*the device has \d+ bytes free"):
        _raw(1, 2_000_000, 1000, 128, np.full(2_000_000, 128), scratch=1 << 35)
    with pytest.raises(L.HmscNativeError, match=r"series is limited to 2\^28 doubles"):
        nf = np.full(300, 2, dtype=np.int32)
        out = [np.zeros(1) for _ in range(4)]
        L.check(L.lib().hmsc_omega_diagnostics(0, 1, 300, 2000, 2, L.iptr(nf), L.fptr(out[0]), 0, L.fptr(out[0]),
                                               L.fptr(out[1]), L.fptr(out[2]), None, L.fptr(out[3])))
