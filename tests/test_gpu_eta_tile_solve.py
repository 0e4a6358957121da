"""The fused updateEta's per-tile solve (one wave's chain of fp64 MFMAs, kernels.hip
eta_fused_kernel) against the CPU oracle, at the smallest shapes that exercise each edge of
the chain: padding of the site tile, of the 4-row covariate steps and of the factor bucket,
the three NFB instantiations, a second 16-column Gram block and the K = 64 limit.

Per element |device - oracle| <= tol * max|oracle Eta|: 1e-9 for the draw (same Philox
stream; libm ulps through the normal), 1e-10 for the conditional mean (noise mode 1).  The
Gram partials, reduced by the following updateZ, must equal XEta^T XEta to 1e-12.
"""
import numpy as np
import pytest

from helpers import H, O, oracle_model, rel_err, synthetic_model
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

TOL_MOMENT = 1e-10
TOL_DRAW = 1e-9
TOL_GRAM = 1e-12
SEED = 24681357
IT = 7
EF_FUSED = 0  # EtaMode of an eager launch

# (ny, ns, nc, nf): the edge each one exercises
SHAPES = [
    (7, 5, 1, 1),        # one partial tile, one X step mostly padding, ns < 16
    (16, 16, 4, 8),      # exact tile, NFB 8 full
    (17, 30, 5, 9),      # second tile of one site, nc not a multiple of 4, NFB 12
    (203, 50, 20, 10),   # the bench's K = 30 class
    (120, 33, 7, 13),    # NFB 16, ns not a multiple of 16
    (64, 20, 2, 16),     # nf = 16
    (95, 24, 48, 16),    # K = 64, the fused path's limit, 12 X steps
]


def _nfb(nf):
    return 8 if nf <= 8 else 12 if nf <= 12 else 16


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "ny%d_ns%d_nc%d_nf%d" % s)
def case(request):
    """The model, a state two oracle sweeps in, and the oracle's Eta (draw and mean), once."""
    ny, ns, nc, nf = request.param
    hM = synthetic_model(ny=ny, ns=ns, nc=nc, nf=nf, seed=100 + ny)
    m = oracle_model(hM)
    rng = Rng(SEED)
    st = O.compute_initial_parameters(m, rng)
    for it in range(1, 3):
        st = O.sweep(st, m, rng, it, updater={"GammaEta": False})
    draw = O.update_eta(st, m, Rng(SEED), IT)[0]
    mean = O.update_eta(st, m, Rng(SEED), IT, zero_noise=True)[0]
    for a in (draw, mean):
        a.setflags(write=False)
    return request.param, hM, m, st, draw, mean


def _chain(hM, st):
    ch = H.Chain(hM, SEED, device=0, updater={"GammaEta": False})
    ch.init()
    ch.set_state(st)
    return ch


def _update_eta_fused(ch, nf):
    """ch.update("Eta") that fails unless it was one eta_fused_kernel launch of nf's bucket."""
    before = ch.debug_get("eta_fused", 3)
    ch.update("Eta", IT)
    after = ch.debug_get("eta_fused", 3)
    assert after[0] == before[0] + 1, "updateEta did not go through eta_fused_kernel"
    assert (after[1], after[2]) == (_nfb(nf), EF_FUSED), after


def _elem_err(dev, ref):
    return float(np.max(np.abs(np.asarray(dev) - ref)) / np.max(np.abs(ref)))


def test_eta_draw(case):
    (ny, ns, nc, nf), hM, m, st, draw, _ = case
    ch = _chain(hM, st)
    _update_eta_fused(ch, nf)
    eta = ch.get_state()["Eta"][0]
    ch.close()
    assert eta.shape == draw.shape
    err = _elem_err(eta, draw)
    print("draw", (ny, ns, nc, nf), err)
    assert err <= TOL_DRAW


def test_eta_mean(case):
    (ny, ns, nc, nf), hM, m, st, _, mean = case
    ch = _chain(hM, st)
    ch.set_noise_mode(1)
    _update_eta_fused(ch, nf)
    eta = ch.get_state()["Eta"][0]
    ch.close()
    err = _elem_err(eta, mean)
    print("mean", (ny, ns, nc, nf), err)
    assert err <= TOL_MOMENT


def test_gram_after_z(case):
    """G's Eta rows come from the tile partials of the Eta launch, reduced by the next updateZ."""
    (ny, ns, nc, nf), hM, m, st, _, _ = case
    ch = _chain(hM, st)
    _update_eta_fused(ch, nf)
    ch.update("Z", IT)
    g = ch.get_state()
    K = nc + nf
    Kmax = int(ch.debug_get("dims", 8)[2])
    G = ch.debug_get("G", Kmax * Kmax).reshape(Kmax, Kmax).T[:K, :K]
    ch.close()
    XEta, _ = O._xeta_and_prior(dict(st, Eta=g["Eta"]), m)
    err = rel_err(G, XEta.T @ XEta)
    print("gram", (ny, ns, nc, nf), err)
    assert err < TOL_GRAM


@pytest.mark.parametrize("nf", [3, 9, 13])
def test_replay_matches_eager(monkeypatch, nf):
    """A recorded run as graph replays equals the eager launch sequence bit for bit, per NFB."""
    hM = synthetic_model(ny=203, ns=30, nc=4, nf=nf, seed=12)
    out = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("HMSC_NO_GRAPH", no_graph)
        ch = H.Chain(hM, 77, device=0, updater={"GammaEta": False})
        ch.init()
        rec = ch.run(transient=3, samples=13, thin=1, adaptNf=[0])
        path = ch.debug_get("eta_fused", 3)
        ch.close()
        assert path[0] >= 1 and path[1] == _nfb(nf), path
        out.append(rec)
    for k in ("Eta0", "Beta", "Lambda0"):
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
