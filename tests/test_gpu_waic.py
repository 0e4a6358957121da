"""computeWAIC on the device (hmsc_waic, waic.hip) against mpmath cell by cell and against the
host function call by call.

Bound, and the maximum measured on an MI355X (profiles/waic_measure.txt):

    log_pnorm (hook)      5e-13 relative                  1.5e-13 (17,758 points)
    probit cells          5e-13 relative                  1.5e-13
    normal cells          4 ulp of the largest term       2.4 ulp
    Poisson cells         1.67e-15 scale (4 x measured)   4.2e-16 (ghN = 11), 3.4e-16 (ghN = 20)

log_pnorm's 5e-13 is the project's own budget (test_gpu_draw_functions.py): erfc 2e-13 relative,
doubled through 1 / (1 - p) at p = 1/2, plus the logarithm's 4 ulp.  Where log Phi(x) itself is
subnormal (x > 37.5: it is -Phi(-x) < 2.3e-308) a double cannot hold 5e-13 relative; there the
bound is two quanta of the format, 2 * 2^-1074: one for the library exp that forms the subnormal
Phi(-x), one for the roundings after it.

The Poisson bound is 4 x the error measured on an MI355X relative to scale = max(1, y |eta|_max,
e^eta_max, lgamma(y + 1)), the terms cancel and lgamma is the HIP library's; it may never exceed
1e-12 scale.
"""
import ctypes

import mpmath as mp
import numpy as np
import pytest

import waic_oracle as W
from helpers import H  # noqa: F401  (puts the repository root on sys.path)
from hmsc_amd import _lib as L
from hmsc_amd import post as P

pytestmark = pytest.mark.gpu

LOG_PNORM_BOUND = 5e-13
QUANTUM = 2.0 ** -1074
POISSON_MEASURED = 4.168e-16               # max error / scale on an MI355X (profiles/waic_measure.txt)
POISSON_BOUND = 1e-12 if POISSON_MEASURED is None else min(4 * POISSON_MEASURED, 1e-12)


def _live():
    out = (ctypes.c_int64 * 4)()
    L.check(L.lib().hmsc_debug_live_resources(out))
    return list(out)


def _window(x0, w):
    return x0 * (1.0 + np.arange(-w, w + 1) * 2.0 ** -52)


def _bisect(f, lo, hi):
    """The double where the decreasing f changes sign."""
    while np.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    return lo


def _x_grid():
    """The issue's grid, made symmetric (a probit cell with y = 0 evaluates log Phi(-x)), with the
    doubles around every branch point of waic_math.h log_pnorm:
      x = 0                                  the sign split
      |x| = 2^(k+2) - 2 sqrt 2, k = 0..3     log_fast(t)'s mantissa fold at t = 2^-k / sqrt 2
      x = 0.5448...                          log_fast(u)'s fold at u = 1 - Phi(-x) = 1 / sqrt 2
      x = 37.519..., 38.485...               Phi(-x) turns subnormal, then 0
      |x| = 1.8958e154                       x^2 / 2 leaves the double range
    The folds of log_fast(t) are hit within a few ulps of the stated point (t is one rounded
    division of the rounded z), and so are the subnormal thresholds (log Phi(-x) has slope -x
    there: its 2e-13 error moves them by 5e-15, an ulp of x): 64 ulps either side.  The fold in u
    moves with the 1.5e-13 relative error of the device's Phi(-x), 1.3e-13 in x or 1200 ulps:
    2048 ulps either side."""
    pts = [np.linspace(-40.0, 40.0, 4001), [0.0, 1e-300, 1e-17, 200.0, 1000.0, 1.3e154, 1.89e154]]
    for k in range(4):
        pts.append(_window(2.0 ** (k + 2) - 2.0 * np.sqrt(2.0), 64))
    fold = float(-mp.sqrt(2) * mp.erfinv(2 * (1 - 1 / mp.sqrt(2)) - 1))
    sub = [_bisect(lambda v: W.mp_log_pnorm(-v) - e * mp.log(2), 37.0, 39.0) for e in (-1022, -1075)]
    pts += [_window(fold, 2048)] + [_window(x0, 64) for x0 in sub]
    x = np.concatenate([np.asarray(p, dtype=np.float64) for p in pts])
    x = np.concatenate([x, -x])   # (-0.0 among them)
    return x


@pytest.fixture(scope="module")
def xref():
    """(x, reference log Phi(x) as mpf), computed once for the hook and the probit cells."""
    x = _x_grid()
    cache = {}
    ref = []
    for v in x:
        k = float(v) + 0.0   # -0.0 and 0.0 share a reference
        if k not in cache:
            cache[k] = W.mp_log_pnorm(k)
        ref.append(cache[k])
    return x, ref


def _lp_err(got, ref):
    """max over elements of |got - ref| / max(5e-13 |ref|, 2 quanta) (<= 1 passes) and the largest
    relative error among the references a double holds as a normal number."""
    worst, rel, at = 0.0, 0.0, 0
    for k, (g, r) in enumerate(zip(got, ref)):
        assert np.isfinite(g), (k, g)
        e = abs(mp.mpf(float(g)) - r)
        q = float(e / max(LOG_PNORM_BOUND * abs(r), mp.mpf(2 * QUANTUM)))
        if q > worst:
            worst, at = q, k
        if abs(r) > 2.3e-308:
            rel = max(rel, float(e / abs(r)))
    return worst, rel, at


def test_log_pnorm_against_mpmath(xref):
    """(1) the debug hook, compiled with waic.hip's flags, per element."""
    x, ref = xref
    before = _live()
    got = np.full(x.shape, np.nan)
    L.check(L.lib().hmsc_debug_eval(0, b"log_pnorm", x.size, L.fptr(L.f64(x)), None, L.fptr(got), None))
    assert _live() == before
    worst, rel, at = _lp_err(got, ref)
    print(f"log_pnorm: max relative error {rel:.3e} over {x.size} points (bound {LOG_PNORM_BOUND:g}); "
          f"worst error / bound {worst:.3f} at x = {x[at]!r}")
    assert worst <= 1.0
    # beyond the double range of x^2 / 2
    far = np.array([-1.9e154, -np.inf, np.inf, np.nan])
    out = np.zeros(4)
    L.check(L.lib().hmsc_debug_eval(0, b"log_pnorm", 4, L.fptr(far), None, L.fptr(out), None))
    assert out[0] == -np.inf and out[1] == -np.inf and out[2] == 0.0 and np.isnan(out[3])


def _cell_model(X, Y, family):
    """ns = 1, nc = 1, nr = 0: with Beta = 1 the linear predictor is X's entry exactly and
    val[s, i] is one cell's term."""
    return W.duck_model(np.asarray(Y, dtype=np.float64)[:, None], np.asarray(X, dtype=np.float64)[:, None], [family])


def _cell_post(sigmas):
    return [dict(Beta=np.ones((1, 1)), sigma=np.array([float(s)]), Eta=[], Lambda=[]) for s in sigmas]


def test_probit_cells_against_mpmath(xref):
    """(2) the kernel's probit term over the grid of (1), y in {0, 1, NA}."""
    x, ref = xref
    lookup = {float(v) + 0.0: r for v, r in zip(x, ref)}
    n = x.size
    hM = _cell_model(np.tile(x, 3), np.r_[np.zeros(n), np.ones(n), np.full(n, np.nan)], 2)
    res = P._waic_device(hM, _cell_post([1.0, 1.0]), 11, 0)
    val = res["val"]
    assert (val[0] == val[1]).all() and (val[0, 2 * n:] == 0.0).all()
    w0, r0, a0 = _lp_err(val[0, :n], [lookup[-float(v) + 0.0] for v in x])
    w1, r1, a1 = _lp_err(val[0, n:2 * n], ref)
    print(f"probit cells: max relative error {max(r0, r1):.3e} (bound {LOG_PNORM_BOUND:g}); worst error / bound "
          f"{max(w0, w1):.3f} at x = {x[a0 if w0 > w1 else a1]!r}, y = {0 if w0 > w1 else 1}")
    assert max(w0, w1) <= 1.0


def test_normal_cells_against_mpmath():
    """(2) dnorm(y, E, sigma^(-1/2), log) for sigma in {1e-4, 1, 1e4}: 4 ulp of the largest of
    the three terms it is summed from."""
    E = np.tile(np.linspace(-40.0, 40.0, 4001), 2)
    y = np.r_[np.full(4001, 0.5), np.full(4001, 17.0)]
    sig = [1e-4, 1.0, 1e4]
    val = P._waic_device(_cell_model(E, y, 1), _cell_post(sig), 11, 0)["val"]
    worst = 0.0
    for s, sg in enumerate(sig):
        for i in range(E.size):
            t = W.mp_normal_terms(y[i], E[i], sg)
            ulp = np.spacing(float(max(abs(v) for v in t)))
            worst = max(worst, float(abs(mp.mpf(float(val[s, i])) - mp.fsum(t)) / ulp))
    print(f"normal cells: max error {worst:.3f} ulp of the largest term (bound 4)")
    assert worst <= 4.0


@pytest.mark.parametrize("ghN", [11, 20])
def test_poisson_cells_against_mpmath(ghN):
    """(2) the quadrature term for y in {0, 1, 7, 1000, 1e6} x E in [-30, 14] x sigma in {0.01, 1,
    25}, against the same sum in mpmath; the cells where the literal host form is -inf included."""
    ys = np.array([0.0, 1.0, 7.0, 1000.0, 1e6])
    Es = np.linspace(-30.0, 14.0, 23)
    y, E = [a.ravel() for a in np.meshgrid(ys, Es, indexing="ij")]
    sig = [0.01, 1.0, 25.0]
    hM = _cell_model(E, y, 3)
    post = _cell_post(sig)
    val = P._waic_device(hM, post, ghN, 0)["val"]
    with np.errstate(divide="ignore"):
        host = P._waic_val_host(hM, post, ghN)
    assert np.isinf(host).any() and np.isfinite(val).all()
    gx, gw = np.polynomial.hermite.hermgauss(ghN)
    worst, worst_u, n_under = 0.0, 0.0, 0
    for s, sg in enumerate(sig):
        for i in range(E.size):
            r, scale = W.mp_poisson_cell(y[i], E[i], sg, gx, gw)
            e = float(abs(mp.mpf(float(val[s, i])) - r) / scale)
            worst = max(worst, e)
            if np.isinf(host[s, i]):
                n_under += 1
                worst_u = max(worst_u, e)
    print(f"Poisson cells, ghN = {ghN}: max error / scale {worst:.3e} (bound {POISSON_BOUND:g}); "
          f"{n_under} cells where the host form is -inf, max there {worst_u:.3e}")
    assert worst <= POISSON_BOUND


# ---------------------------------------------------------------------------
# (3) whole-call parity with the host function
# ---------------------------------------------------------------------------
def _parity(hM, post, ghN=11, chunk=0):
    """The posteriors of these cases are spread so that a site's val varies over the samples by
    more than a tenth of its size: V's relative error is 2 |dval| / sd(val), and log_pnorm's
    5e-13 budget on val then stays inside V's 1e-11 (samples that nearly agree at a site make the
    variance ill conditioned whoever computes it)."""
    hM.postList = [post]
    before = _live()
    dev = P._waic_device(hM, post, ghN, 0, chunk)
    assert _live() == before
    val = P._waic_val_host(hM, post, ghN)
    host = H.computeWAIC(hM, ghN=ghN, byUnit=True)
    assert np.isfinite(val).all() and np.isfinite(host["WAIC"])
    assert (np.abs(dev["val"] - val) <= 1e-12 * np.maximum(1.0, np.abs(val))).all()
    np.testing.assert_allclose(dev["Bl"], host["Bl"], rtol=1e-11, atol=0)
    np.testing.assert_allclose(dev["V"], host["V"], rtol=1e-11, atol=0)
    assert abs(dev["WAIC"] - host["WAIC"]) <= 1e-11 * abs(host["WAIC"])
    assert H.computeWAIC(hM, ghN=ghN, device=0) == dev["WAIC"]
    u = H.computeWAIC(hM, ghN=ghN, device=0, byUnit=True)
    assert u["WAIC"] == dev["WAIC"] and (u["Bl"] == dev["Bl"]).all() and (u["V"] == dev["V"]).all()
    return dev


def _pi(rng, ny, units):
    """1-based Pi columns: ny units (one per site) or grouped units, every unit used."""
    cols = [np.arange(ny) + 1 if n == ny else rng.permutation(np.arange(ny) % n) + 1 for n in units]
    return np.column_stack(cols)


MIXED_FAMILY = np.r_[[3] * 3, [2] * 30, [1] * 18, [2] * 19]   # ns = 70


def _mixed_model(na=False, seed=11):
    """ny = 65, ns = 70: 3 Poisson, then 30 probit, 18 normal, 19 probit columns; two levels, one
    with 13 grouped units.  With ghN = 11 a Poisson cell of column c reads its y of node g from
    column c + 3 g (the recycling of dpois(Y, exp(gX)) in R), columns 0..32: those hold counts
    and 0/1 values, for which dpois is positive.  The NA cells (10 %) go to the normal and probit
    columns from 33 on, the ones the recycling does not read: an NA read by a Poisson cell makes
    the host function's own value NaN, and leaves nothing to compare."""
    rng = np.random.default_rng(seed)
    ny, ns = 65, 70
    Y = rng.integers(0, 2, (ny, ns)).astype(float)
    Y[:, :3] = rng.poisson(2.0, (ny, 3))
    Y[:, 33:51] = rng.standard_normal((ny, 18))
    if na:
        mask = rng.random((ny, ns)) < 0.1
        mask[:, :33] = False
        Y[mask] = np.nan
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, 2))])
    hM = W.duck_model(Y, X, MIXED_FAMILY, Pi=_pi(rng, ny, [ny, 13]), nps=[ny, 13])
    return hM, W.random_post(hM, 37, [3, 2], seed, nf_jitter=True)


@pytest.fixture(scope="module")
def mixed():
    return _mixed_model()


def test_parity_probit_no_levels():
    rng = np.random.default_rng(5)
    ny, ns = 130, 33
    hM = W.duck_model(rng.integers(0, 2, (ny, ns)).astype(float),
                      np.column_stack([np.ones(ny), rng.standard_normal((ny, 2))]), [2] * ns)
    _parity(hM, W.random_post(hM, 3, [], 5, beta_scale=0.8))


def test_parity_mixed_families_two_levels(mixed):
    _parity(*mixed)


def test_parity_mixed_families_with_na():
    hM, post = _mixed_model(na=True)
    assert np.isnan(hM.Y).mean() > 0.03
    _parity(hM, post)


def test_parity_all_poisson_with_na():
    rng = np.random.default_rng(7)
    ny, ns = 70, 9
    Y = rng.poisson(3.0, (ny, ns)).astype(float)
    Y[rng.random((ny, ns)) < 0.1] = np.nan
    hM = W.duck_model(Y, np.column_stack([np.ones(ny), rng.standard_normal(ny)]), [3] * ns,
                      Pi=_pi(rng, ny, [10]), nps=[10])
    _parity(hM, W.random_post(hM, 5, [2], 7), ghN=9)


def test_parity_xdim_level():
    rng = np.random.default_rng(8)
    ny, ns = 50, 18
    xs = [np.column_stack([np.ones(10), rng.standard_normal(10)]), None]
    hM = W.duck_model(rng.integers(0, 2, (ny, ns)).astype(float), rng.standard_normal((ny, 2)), [2] * ns,
                      Pi=_pi(rng, ny, [10, ny]), nps=[10, ny], xs=xs)
    _parity(hM, W.random_post(hM, 4, [2, 3], 8))


def test_parity_xselect_posterior():
    """A variable-selection posterior records Beta with the switched-off blocks already zero."""
    rng = np.random.default_rng(9)
    ny, ns = 40, 17
    fam = np.r_[[1] * 5, [2] * 12]
    Y = rng.integers(0, 2, (ny, ns)).astype(float)
    Y[:, :5] = rng.standard_normal((ny, 5))
    hM = W.duck_model(Y, np.column_stack([np.ones(ny), rng.standard_normal((ny, 3))]), fam)
    hM.XSelect = [dict(covGroup=[2, 3], spGroup=np.arange(ns) % 2 + 1, q=[0.5, 0.5])]
    post = W.random_post(hM, 6, [], 9)
    for s, smp in enumerate(post):
        smp["Beta"][np.ix_([2, 3], np.arange(ns) % 2 == s % 2)] = 0.0
    _parity(hM, post)


@pytest.mark.parametrize("K", [1, 128])
def test_parity_k_edges(K):
    rng = np.random.default_rng(K)
    ny, ns = 40, 20
    if K == 1:
        hM = W.duck_model(rng.integers(0, 2, (ny, ns)).astype(float), rng.standard_normal((ny, 1)), [2] * ns)
        nfs = []
    else:
        hM = W.duck_model(rng.integers(0, 2, (ny, ns)).astype(float), rng.standard_normal((ny, 8)), [2] * ns,
                          Pi=_pi(rng, ny, [ny, 7]), nps=[ny, 7])
        nfs = [60, 60]
    _parity(hM, W.random_post(hM, 6, nfs, K, beta_scale=1.0))


def test_k_129_is_refused_with_the_cap_named():
    rng = np.random.default_rng(2)
    ny, ns = 20, 4
    hM = W.duck_model(rng.integers(0, 2, (ny, ns)).astype(float), rng.standard_normal((ny, 9)), [2] * ns,
                      Pi=_pi(rng, ny, [ny, 5]), nps=[ny, 5])
    before = _live()
    with pytest.raises(L.HmscNativeError, match=r"129 exceeds HMSC_KCAP = 128"):
        P._waic_device(hM, W.random_post(hM, 2, [60, 60], 2), 11, 0)
    assert _live() == before


def test_td_fixture():
    """(4) test-WAIC.R:4 on the device."""
    from test_golden_td import td_model, td_postlist
    hM = td_model()
    hM.postList = td_postlist(hM)
    host = H.computeWAIC(hM)
    dev = H.computeWAIC(hM, device=0)
    assert abs(dev - host) <= 1e-12 * abs(host) and round(dev, 1) == 0.8


def test_repeat_and_chunking_are_bit_equal(mixed):
    """(5) every val[s, i] and every sum after it has one order, whatever shares a launch."""
    hM, post = mixed
    runs = [P._waic_device(hM, post, 11, 0, c) for c in (0, 0, 1, 5)]
    for r in runs[1:]:
        assert r["WAIC"] == runs[0]["WAIC"]
        for k in ("val", "Bl", "V"):
            assert (r[k] == runs[0][k]).all(), k


def test_underflow_stays_finite():
    """(6) ns = 64 probit species with E = -6 where y = 1: val is near -1300, exp(val) is 0 and
    the host function returns inf; the device returns the shifted sums of the host's val."""
    ny, ns, S = 30, 64, 8
    hM = W.duck_model(np.ones((ny, ns)), np.ones((ny, 1)), [2] * ns)
    rng = np.random.default_rng(3)
    post = [dict(Beta=-6.0 - 0.1 * rng.random((1, ns)), sigma=np.ones(ns), Eta=[], Lambda=[]) for _ in range(S)]
    hM.postList = [post]
    with np.errstate(divide="ignore"):
        assert np.isinf(H.computeWAIC(hM))
    val = P._waic_val_host(hM, post)
    assert val.max() < -1200
    Bl, V, w = W.shifted(val)
    dev = P._waic_device(hM, post, 11, 0)
    assert np.isfinite(dev["WAIC"])
    np.testing.assert_allclose(dev["Bl"], Bl, rtol=1e-11, atol=0)
    np.testing.assert_allclose(dev["V"], V, rtol=1e-11, atol=0)
    assert abs(dev["WAIC"] - w) <= 1e-11 * abs(w)


def test_lifecycle_of_refused_calls(mixed):
    """(7) every refusal leaves the live-resource counts where they were."""
    hM, post = mixed
    before = _live()
    out = np.zeros(1)

    def refused(match, **change):
        a, keep, _ = P._waic_args(hM, post, 11, 0)
        for k, v in change.items():
            setattr(a, k, v)
        with pytest.raises(L.HmscNativeError, match=match):
            L.check(L.lib().hmsc_waic(ctypes.byref(a), L.fptr(out), None, None))
        assert _live() == before

    refused("nsamples must be at least 2", nsamples=1)
    refused("sample_chunk", sample_chunk=-1)
    refused("ghN", ghN=0)
    bad = L.i32(np.full(hM.ny * 2, 99999))
    refused("Pi out of range", Pi=L.iptr(bad))
    fam = L.i32(np.full(hM.ns, 4))
    refused("family must be", family=L.iptr(fam))
    P._waic_device(hM, post, 11, 0)
    assert _live() == before
