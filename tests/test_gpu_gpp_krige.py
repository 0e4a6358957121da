"""GPP kriging of new spatial units on the device (hmsc_krige mode 4, hmsc_amd/csrc/gpp.hip) against
the numpy restatement tests/gpp_krige_oracle.py (itself pinned to the host path by
tests/test_host_gpp_krige.py), at the project's parity bound for outputs that carry draws: 1e-9
normwise (helpers.rel_err) and |dev - ref| <= 1e-9 max(1, |ref|) per element.

Inputs (gpp_cases.py): uniform random points in the unit square, constructKnots' knots, grid values
a in {0, ~0.056, ~0.098, ~0.196} only.  On these cases two fp64 host routes (the literal inv form and
a Cholesky / triangular-solve form) agree to <= 1.4e-13 for draws and <= 8.8e-14 for the mean
(normwise; <= 4.0e-13 per element), so the reference alone is > 2000x inside the bound.  At a = 0.4
the two routes already differ by 1e-10 at nK = 100 and at a = 1.4 by up to 6e-8, which is why
krige_cases.make_posterior is not used here.  A new unit on a knot is the one place where the routes
disagree visibly (dDn = +-2e-16 with either sign, 1.5e-8 after the square root); device and
restatement both give such a unit its exact dDn = 0."""
import ctypes as C

import numpy as np
import pytest

import gpp_cases as GC
import gpp_krige_oracle as GO
import krige_cases as KC
from helpers import rel_err
from hmsc_amd import _lib as L
from hmsc_amd.predict import predictLatentFactor

pytestmark = pytest.mark.gpu

SEED = 20250314
_cache = {}


def _case(npo, nn, nKnots):
    key = (npo, nn, nKnots)
    if key not in _cache:
        rl, names, newn, xy, sK = GC.make_level(npo, nn, nKnots, 1000 + npo + nn + nKnots)
        eta, alpha = GC.make_posterior(rl, npo, npo + nn)
        _cache[key] = (rl, names, newn, xy, sK, eta, alpha, KC.interleave(names, newn))
    return _cache[key]


def _reference(case, level=0):
    rl, names, newn, xy, sK, eta, alpha, up = case
    key = ("ref", id(case), level)
    if key not in _cache:
        E, idx = KC.stacked(eta, alpha)
        npo = len(names)
        _cache[key] = GO.krige(np.asarray(rl.alphapw)[:, 0], E, idx, SEED, xy[:npo], xy[npo:], sK, level=level)
    return _cache[key]


def _device(case, level=0):
    rl, names, newn, xy, sK, eta, alpha, up = case
    out = predictLatentFactor(up, names, eta, rl, postAlpha=alpha, device=0, seed=SEED, level=level, gppDevice=True)
    for s, e in enumerate(out):
        assert e.shape == (len(up), eta[s].shape[1])
        for r, u in enumerate(up):
            if u in names:
                assert np.array_equal(e[r], eta[s][names.index(u)])
    return [np.stack([e[up.index(n)] for n in newn]) for e in out]


def _check(dev, ref, eta):
    errs, elem = [], []
    for s, d in enumerate(dev):
        nf = eta[s].shape[1]
        assert np.all(np.isfinite(d))
        r = ref[s][:, :nf]
        errs.append(rel_err(d, r))
        elem.append(float(np.max(np.abs(d - r) / np.maximum(1.0, np.abs(r)))))
    print("rel_err per sample:", ["%.2e" % e for e in errs], "per element:", ["%.2e" % e for e in elem])
    assert max(errs) < 1e-9
    assert max(elem) <= 1e-9


@pytest.mark.parametrize("npo,nn,nKnots", GC.SHAPES)
def test_gpp(npo, nn, nKnots):
    case = _case(npo, nn, nKnots)
    assert case[4].shape[0] == {3: 16, 4: 25, 6: 49, 8: 81}[nKnots]
    _check(_device(case), _reference(case), case[5])


def test_more_pairs_on_a_grid_value_than_one_tile():
    """70 samples x 2 factors, 130 of the 140 pairs on one grid value: the pairs' columns cross two
    64-column tiles of the plan's products and of the slab kernel."""
    npo, nn, S = 70, 5, 70
    rl, names, newn, xy, sK = GC.make_level(npo, nn, 4, 77)
    g = GC.grid_indices(rl)
    rng = np.random.default_rng(8)
    eta = [rng.standard_normal((npo, 2)) for _ in range(S)]
    alpha = [np.array([g[1], g[2]]) for _ in range(S)]
    for s in range(5):
        alpha[7 * s][1] = g[3] if s % 2 else g[1]          # the last factor decides for both
    dev = predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=SEED, gppDevice=True)
    ref = GO.krige(np.asarray(rl.alphapw)[:, 0], np.stack(eta), np.stack(alpha), SEED, xy[:npo], xy[npo:], sK)
    _check(dev, ref, eta)


def test_draws_repeat_and_follow_the_counters():
    case = _case(100, 70, 4)
    a, b = _device(case), _device(case)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))           # bit-equal
    c = _device(case, level=1)
    assert all(not np.array_equal(x, y) for x, y in zip(a, c))
    _check(c, _reference(case, level=1), case[5])
    # sample 1's last factor sits at a = 0: both factors are z of the contract itself
    for lev, out in ((0, a), (1, c)):
        for h in range(2):
            z = GO.z_new(SEED, lev, 70, 1, h)
            assert np.max(np.abs(out[1][:, h] - z)) < 1e-12 * np.max(np.abs(z))
    # level 1 moves the knot innovation too: at equal z_new the outputs would still differ
    assert not np.array_equal(GO.z_knot(SEED, 0, 25, 0, 0), GO.z_knot(SEED, 1, 25, 0, 0))


def test_new_unit_on_a_knot():
    rl, names, newn, xy, sK = GC.on_knot_level()
    assert np.array_equal(xy[102], sK[7]) and np.array_equal(xy[104], sK[18])
    eta, alpha = GC.make_posterior(rl, 100, 3)
    dev = predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=SEED, gppDevice=True)
    E, idx = KC.stacked(eta, alpha)
    ref = GO.krige(np.asarray(rl.alphapw)[:, 0], E, idx, SEED, xy[:100], xy[100:], sK)
    _check(dev, ref, eta)


def _raw_args(npo=20, nn=3, **kw):
    xy = np.random.default_rng(2).random((npo + nn, 2))
    sK = np.random.default_rng(9).random((4, 2))
    keep = [np.ascontiguousarray(xy.T.ravel()), np.array([0.0, 0.1, 0.2]),
            np.random.default_rng(3).standard_normal(2 * 2 * npo), np.array([[2, 3], [3, 2]], dtype=np.int32),
            np.ascontiguousarray(sK.T.ravel()), xy, sK]
    a = L.hmsc_krige_args()
    a.device, a.np, a.nn, a.sDim, a.G, a.S, a.nfmax, a.mode, a.nNeighbours, a.level = 0, npo, nn, 2, 3, 2, 2, 4, 5, 0
    a.seed = 1
    a.coords, a.alphas, a.Eta, a.alpha = L.fptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2]), L.iptr(keep[3])
    a.knots, a.nK = L.fptr(keep[4]), 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a, keep, np.zeros(2 * 2 * nn)


def _error_of(a, out):
    rc = L.lib().hmsc_krige(C.byref(a), L.fptr(out))
    return rc, L.lib().hmsc_last_error().decode()


def _live():
    live = np.zeros(4, dtype=np.int64)
    L.check(L.lib().hmsc_debug_live_resources(live.ctypes.data_as(C.POINTER(C.c_int64))))
    return live


def test_refusals_by_name_and_resources():
    a, keep, out = _raw_args()
    assert _error_of(a, out)[0] == 0                                 # the plain call is fine
    base = _live()
    assert _error_of(a, out)[0] == 0 and np.all(np.isfinite(out)) and np.any(out != 0)
    assert np.array_equal(_live(), base)                             # a good call leaves nothing behind
    a, keep, out = _raw_args(nK=0)
    rc, msg = _error_of(a, out)
    assert rc != 0 and "GPP kriging needs knots" in msg
    a, keep, out = _raw_args()
    a.knots = None
    rc, msg = _error_of(a, out)
    assert rc != 0 and "GPP kriging needs knots" in msg
    a, keep, out = _raw_args()
    D = np.ascontiguousarray(GO.pdist(keep[5], keep[5]).ravel())
    a.coords, a.dist = None, L.fptr(D)
    rc, msg = _error_of(a, out)
    assert rc != 0 and "GPP kriging needs coordinates" in msg
    a, keep, out = _raw_args()
    keep[3][1, 0] = 4                                                # G = 3
    rc, msg = _error_of(a, out)
    assert rc != 0 and "grid index 4" in msg and "outside the alphapw grid" in msg
    # fitted unit 11 on knot 2
    a, keep, out = _raw_args()
    xy = keep[5].copy()
    xy[11] = keep[6][2]
    keep[0] = np.ascontiguousarray(xy.T.ravel())
    a.coords = L.fptr(keep[0])
    rc, msg = _error_of(a, out)
    assert rc != 0 and "fitted unit 11" in msg and "lies on a knot" in msg and "grid index 2" in msg
    assert np.array_equal(_live(), base)                             # nor does a refused one
    a, keep, out = _raw_args()
    assert _error_of(a, out)[0] == 0                                 # and the next call is served
