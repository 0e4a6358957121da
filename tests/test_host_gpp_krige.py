"""tests/gpp_krige_oracle.py, the restatement that hmsc_krige's mode 4 is held to
(test_gpu_gpp_krige.py), against the host path hmsc_amd.predict._krige (GPP branch,
R/predictLatentFactor.R:161-203), and the quirks both keep.  No GPU, no device library.

The host draws standard_normal(nK) then standard_normal(nn) per factor from its generator (one
standard_normal(nn) at a = 0); a stand-in generator hands it the restatement's Philox vectors in
that order."""
import numpy as np

import gpp_cases as GC
import gpp_krige_oracle as GO
import krige_cases as KC
from helpers import rel_err
from hmsc_amd.predict import _krige

SEED = 99


class QueuedNormals:
    """standard_normal(n) returns the next queued vector, which must have n entries."""

    def __init__(self, vectors):
        self.q = list(vectors)

    def standard_normal(self, n):
        v = self.q.pop(0)
        assert v.shape == (int(n),), (v.shape, n)
        return v


def _host(rl, eta, alpha, xy, npo, sK, seed=SEED, level=0):
    alphas = np.asarray(rl.alphapw, dtype=np.float64)
    nn = xy.shape[0] - npo
    out = []
    for s, (e, al) in enumerate(zip(eta, alpha)):
        a = alphas[al[-1] - 1, 0]
        q = []
        for h in range(e.shape[1]):
            if a > 0:
                q.append(GO.z_knot(seed, level, sK.shape[0], s, h))
            q.append(GO.z_new(seed, level, nn, s, h))
        gen = QueuedNormals(q)
        out.append(_krige(rl, e, al, alphas, xy[:npo], xy[npo:], False, False, gen))
        assert not gen.q
    return out


def _oracle(rl, eta, alpha, xy, npo, sK, **kw):
    E, idx = KC.stacked(eta, alpha)
    return GO.krige(np.asarray(rl.alphapw)[:, 0], E, idx, kw.pop("seed", SEED), xy[:npo], xy[npo:], sK, **kw)


def test_restatement_equals_host_path():
    for npo, nn, k in GC.SHAPES[:3]:
        rl, names, newn, xy, sK = GC.make_level(npo, nn, k, 1000 + npo + nn + k)
        eta, alpha = GC.make_posterior(rl, npo, npo + nn)
        host = _host(rl, eta, alpha, xy, npo, sK)
        ref = _oracle(rl, eta, alpha, xy, npo, sK)
        for s, h in enumerate(host):
            assert np.all(np.isfinite(h))
            assert rel_err(ref[s][:, :h.shape[1]], h) < 1e-12, (npo, nn, k, s)


def test_last_factor_decides_for_every_factor():
    """Quirk 19 (R: ag = alpha[nf])."""
    npo, nn = 60, 9
    rl, names, newn, xy, sK = GC.make_level(npo, nn, 3, 12)
    g0, g05, g1, g2 = GC.grid_indices(rl)
    eta = [np.random.default_rng(s).standard_normal((npo, 2)) for s in range(3)]
    # sample 0: first factor at a = 0, last at a > 0; sample 1: the reverse; sample 2: both at the last one's a
    alpha = [np.array([g0, g2]), np.array([g2, g0]), np.array([g2, g2])]
    ref = _oracle(rl, eta, alpha, xy, npo, sK)
    host = _host(rl, eta, alpha, xy, npo, sK)
    for s in range(3):
        assert rel_err(ref[s][:, :2], host[s]) < 1e-12
    # sample 0's first factor is kriged although its own grid value is 0: it is not z, and it is what a
    # sample with both factors at g2 gives for the same Eta column and counters
    z00 = GO.z_new(SEED, 0, nn, 0, 0)
    assert np.max(np.abs(ref[0][:, 0] - z00)) > 0.1
    both = _oracle(rl, [eta[0]], [np.array([g2, g2])], xy, npo, sK)
    assert np.array_equal(both[0][:, 0], ref[0][:, 0])
    # sample 1's last factor is at a = 0: z for both factors
    for h in range(2):
        assert np.array_equal(ref[1][:, h], GO.z_new(SEED, 0, nn, 1, h))
        assert np.array_equal(host[1][:, h], GO.z_new(SEED, 0, nn, 1, h))


def test_knot_innovation_has_covariance_R_Rt_not_iF():
    """Quirk 20: R = chol(iF) is upper and R'R = iF, but the innovation is R z, of covariance R R'."""
    npo, nn = 100, 5
    rl, names, newn, xy, sK = GC.make_level(npo, nn, 4, 31)
    a = np.asarray(rl.alphapw)[GC.grid_indices(rl)[3] - 1, 0]
    P = GO.parts(a, xy[:npo], xy[npo:], sK)
    R, iF = P["R"], P["iF"]
    assert np.allclose(np.triu(R), R) and rel_err(R.T @ R, iF) < 1e-12
    assert rel_err(R @ R.T, iF) > 1e-3                   # far above rounding
    # the restatement's innovation is linear in z_knot with matrix Wns R: with Eta = 0 and the knot
    # draw replaced by a unit vector the output column is Wns R[:, k], so its covariance is
    # Wns R R' Wns'
    zk = GO.z_knot(SEED, 0, sK.shape[0], 0, 0)
    eta0 = [np.zeros((npo, 1))]
    alpha = [np.array([GC.grid_indices(rl)[3]])]
    out = _oracle(rl, eta0, alpha, xy, npo, sK)[0][:, 0]
    resid = GO.residual_sd(P) * GO.z_new(SEED, 0, nn, 0, 0)
    assert rel_err(out - resid, P["Wns"] @ (R @ zk)) < 1e-12
    assert rel_err(out - resid, P["Wns"] @ (R.T @ zk)) > 1e-3


def test_new_unit_on_a_knot_is_finite():
    """Quirk 21: 1 - Wns iWss Wns' of a unit on a knot is a rounding residue of either sign; the host's
    sqrt gives NaN or a 1e-8 standard deviation, the restatement the exact 0."""
    rl, names, newn, xy, sK = GC.on_knot_level()
    eta, alpha = GC.make_posterior(rl, 100, 3)
    ref = _oracle(rl, eta, alpha, xy, 100, sK)
    assert np.all(np.isfinite(ref))
    with np.errstate(invalid="ignore"):
        host = _host(rl, eta, alpha, xy, 100, sK)
    on, off = [2, 4], [0, 1, 3, 5]
    residue = []
    for s, h in enumerate(host):
        nf = h.shape[1]
        assert rel_err(ref[s][off, :nf], h[off]) < 1e-12              # the other units are untouched
        d = np.abs(h[on] - ref[s][on, :nf])
        assert np.all(np.isnan(d) | (d < 1e-6))                       # NaN, or a tiny variance
        residue.append(d)
    residue = np.concatenate([r.ravel() for r in residue])
    assert np.isnan(residue).any() or np.nanmax(residue) > 0          # the host does differ there
    # both fp64 routes of the restatement leave a residue at rounding level there (a few 1e-16, of a
    # sign that the route and the grid value decide), whose square root would be the 1e-8 term
    a = np.asarray(rl.alphapw)[GC.grid_indices(rl)[2] - 1, 0]
    for form in ("inv", "chol"):
        assert np.all(np.abs(GO.parts(a, xy[:100], xy[100:], sK, form)["dDn"][on]) < 1e-14)


def test_two_routes_agree_on_the_gpu_cases():
    """The figure test_gpu_gpp_krige.py's docstring quotes: the reference's own error on its cases."""
    worst = 0.0
    for npo, nn, k in GC.SHAPES:
        rl, names, newn, xy, sK = GC.make_level(npo, nn, k, 1000 + npo + nn + k)
        eta, alpha = GC.make_posterior(rl, npo, npo + nn)
        for draws in (True, False):
            a = _oracle(rl, eta, alpha, xy, npo, sK, draws=draws)
            b = _oracle(rl, eta, alpha, xy, npo, sK, draws=draws, form="chol")
            worst = max(worst, rel_err(b, a))
    print("two-route agreement: %.2e" % worst)
    assert worst < 1e-11
