"""Lifecycle of the library's device resources (hmsc_amd/csrc/devmem.h): every device buffer,
pinned host buffer, stream and event is held by one owner per chain or per one-shot call, and
hmsc_debug_live_resources counts what all owners hold.  After hmsc_destroy, a failed create or
a one-shot call (a refused one included) the four counts are back at their baseline -- a leak
of one 256-byte buffer or one event shows, which hipMemGetInfo would not.  The baseline is read
after one warm-up lifecycle, so whatever lives as long as the process is in it."""
import ctypes as C

import numpy as np
import pytest

import betasel_oracle as BO
import krige_cases as KC
import rrr_oracle as RO
from helpers import H, phylo_corr, synthetic_model
from hmsc_amd import _lib as L
from hmsc_amd import workloads as W
from hmsc_amd.predict import predictLatentFactor

pytestmark = pytest.mark.gpu

NO_GE = {"GammaEta": False}
SMALL = dict(ny=30, ns=8, nc=3, nf=2)
GRID3 = dict(spatial=[0], alpha_n=2)      # a 3-point alphapw grid: alpha = 0 and two positive values


def live():
    """[device buffers, pinned host buffers, streams, events] held right now."""
    out = (C.c_int64 * 4)()
    L.check(L.lib().hmsc_debug_live_resources(out))
    return list(out)


def lifecycle(hM, updater, **kw):
    """create, init, two eager sweeps, a recorded run of 4 sweeps (graphs, ring, copy path),
    profiling and kernel timing over one more sweep (their events and buffer), the debug
    precision buffer of noise mode 2, destroy."""
    ch = H.Chain(hM, 11, device=0, updater=updater, **kw)
    ch.init()
    ch.sweep(1)
    ch.sweep(2)
    rec = ch.run(transient=0, samples=4, thin=1, iter0=2)
    assert np.all(np.isfinite(rec["Beta"]))
    ch.profile(True)
    ch.kernel_timing(True)
    ch.sweep(7)
    ch.set_noise_mode(2)
    held = live()
    ch.close()
    return held


@pytest.fixture(scope="module")
def baseline():
    mp = pytest.MonkeyPatch()
    mp.setenv("HMSC_GRAPH_SWEEPS", "2")             # read at create: 4 recorded sweeps are two replays
    lifecycle(synthetic_model(seed=1, **SMALL), NO_GE)
    yield live()
    mp.undo()


def _sel():
    return BO.synthetic_sel(ny=30, ns=8, nc=3, units=(30,), seed=1,
                            selections=[dict(covGroup=[2], spGroup=np.ones(8, dtype=int), q=[0.5])])


CLASSES = {
    "probit": (lambda: synthetic_model(seed=1, **SMALL), NO_GE, {}),
    "mixed_na": (lambda: synthetic_model(seed=2, n_normal=3, na_frac=0.1, **SMALL), NO_GE, {}),
    "two_levels_grouped": (lambda: synthetic_model(ny=36, ns=8, nc=3, nf=2, nr=2, units=[36, 9], seed=3), NO_GE, {}),
    "covariate_level": (lambda: synthetic_model(ny=40, ns=8, nc=3, nf=2, units=[10], x_dim=2, seed=4), NO_GE, {}),
    "phylo": (lambda: synthetic_model(seed=5, C=phylo_corr(8, seed=5), **SMALL), NO_GE, {}),
    "full_coordinates": (lambda: synthetic_model(ny=24, ns=8, nc=2, nf=2, seed=6, **GRID3), NO_GE, {}),
    "nngp": (lambda: synthetic_model(ny=24, ns=8, nc=2, nf=2, seed=7, spatial_method="NNGP", n_neighbours=4, **GRID3),
             NO_GE, {}),
    "gpp": (lambda: synthetic_model(ny=24, ns=8, nc=2, nf=2, seed=8, spatial_method="GPP", n_knots=4, **GRID3),
            NO_GE, {}),
    "gamma_eta": (lambda: synthetic_model(seed=9, **SMALL), {}, {}),
    "gamma_eta_full": (lambda: synthetic_model(ny=24, ns=8, nc=2, nf=2, seed=10, **GRID3), {}, {}),
    "xrrr": (lambda: RO.synthetic_rrr(ny=30, ns=8, ncN=2, ncRRR=1, ncORRR=2, units=(30,), seed=1), NO_GE, {}),
    "xselect": (_sel, {"Gamma2": False, "GammaEta": False}, {}),
    "sharded_host_one_rank": (lambda: synthetic_model(seed=12, **SMALL), NO_GE,
                              dict(rank=0, nranks=1, host_allreduce=lambda x: None)),
}


@pytest.mark.parametrize("name", list(CLASSES))
def test_create_destroy_returns_to_baseline(baseline, name):
    make, updater, kw = CLASSES[name]
    held = lifecycle(make(), updater, **kw)
    assert all(h > b for h, b in zip(held, baseline)), (held, baseline)     # the chain did hold some of each
    assert live() == baseline


def test_late_create_failure_frees_everything(baseline):
    """updateGammaEta on a sharded chain is refused by a host check that runs after most of the
    chain's workspaces exist."""
    hM = synthetic_model(seed=12, **SMALL)
    with pytest.raises(L.HmscNativeError, match="error -1: updateGammaEta cannot run on a species-sharded chain"):
        H.Chain(hM, 1, device=0, updater={}, rank=0, nranks=1, host_allreduce=lambda x: None)
    assert live() == baseline


# ---- one-shot entry points: each a function of the device, returning (status, message)

def _rc(rc):
    return rc, L.lib().hmsc_last_error().decode()


def _predict(device, bad_pi=False):
    ny, ns, nc, nf, npr, S = 30, 8, 2, 2, 6, 3
    rng = np.random.default_rng(1)
    keep = [rng.standard_normal(ny * nc), rng.standard_normal(S * nc * ns), np.ones(S * ns),
            np.full(ns, 2, dtype=np.int32), np.tile([0.0, 1.0], ns), (np.arange(ny) % npr + 1).astype(np.int32),
            np.array([npr], dtype=np.int32), np.array([nf], dtype=np.int32), rng.standard_normal(S * npr * nf),
            rng.standard_normal(S * nf * ns)]
    if bad_pi:
        keep[5][ny - 1] = npr + 1
    a = L.hmsc_predict_args()
    a.ny, a.ns, a.nc, a.nr, a.nsamples, a.expected, a.seed, a.device = ny, ns, nc, 1, S, 1, 5, device
    a.X, a.Beta, a.sigma, a.family, a.YScalePar = (L.fptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2]), L.iptr(keep[3]),
                                                   L.fptr(keep[4]))
    a.Pi, a.np, a.nf = L.iptr(keep[5]), L.iptr(keep[6]), L.iptr(keep[7])
    a.Eta[0], a.Lambda[0] = L.fptr(keep[8]), L.fptr(keep[9])
    out = np.zeros(S * ny * ns)
    return _rc(L.lib().hmsc_predict(C.byref(a), L.fptr(out)))


def _omega(device):
    S, ns, nf = 4, 8, 2
    lam = np.random.default_rng(2).standard_normal(S * ns * nf)
    outs = [np.zeros(ns * ns) for _ in range(4)]
    return _rc(L.lib().hmsc_post_omega(device, S, ns, nf, L.iptr(np.full(S, nf, dtype=np.int32)), L.fptr(lam),
                                       *[L.fptr(o) for o in outs]))


def _vp(device):
    ny, ns, nc, nt, S, nf = 30, 8, 3, 2, 4, 2
    rng = np.random.default_rng(3)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, nc - 1))])
    keep = [np.array([1, 1, 2], dtype=np.int32), np.ascontiguousarray(X.T.ravel()), rng.standard_normal(ns * nt),
            np.ascontiguousarray(np.cov(X, rowvar=False).ravel()), rng.standard_normal(S * nc * ns),
            rng.standard_normal(S * nc * nt), np.full(S, nf, dtype=np.int32), rng.standard_normal(S * nf * ns)]
    a = L.hmsc_vp_args()
    a.device, a.ny, a.ns, a.nc, a.nt, a.S, a.ngroups, a.nr = device, ny, ns, nc, nt, S, 2, 1
    a.group, a.X, a.Tr, a.cM = L.iptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2]), L.fptr(keep[3])
    a.Beta, a.Gamma, a.nf = L.fptr(keep[4]), L.fptr(keep[5]), L.iptr(keep[6])
    a.nfmax[0] = nf
    a.Lambda[0] = L.fptr(keep[7])
    out = np.zeros(nc + 1 + ns * (1 + 1 + 2))
    return _rc(L.lib().hmsc_variance_partitioning(C.byref(a), L.fptr(out)))


def _ess(device):
    n, p = 40, 3
    x = np.random.default_rng(4).standard_normal(n * p)
    ess, order = np.zeros(p), np.zeros(p, dtype=np.int32)
    return _rc(L.lib().hmsc_effective_size(device, n, p, L.fptr(x), L.fptr(ess), L.iptr(order)))


def _chol(device):
    n = 24
    Xm = np.random.default_rng(5).standard_normal((n, n + 5))
    A = np.asfortranarray(Xm @ Xm.T / n + np.eye(n))
    b, info = np.ones(n), np.zeros(1, dtype=np.int32)
    return _rc(L.lib().hmsc_dense_chol_solve(device, L.fptr(A), n, L.fptr(b), L.iptr(info)))


def _grid(device):
    n, G = 24, 3
    xy = np.asfortranarray(np.random.default_rng(6).random((n, 2)))
    iW, RiW, det = np.zeros(n * n * G), np.zeros(n * n * G), np.zeros(G)
    return _rc(L.lib().hmsc_spatial_full_grid(device, n, 2, L.fptr(xy), None, G, L.fptr(np.array([0.0, 0.3, 0.9])),
                                              L.fptr(iW), L.fptr(RiW), L.fptr(det)))


def _krige(device):
    npo, nn = 24, 3
    xy = np.random.default_rng(7).random((npo + nn, 2))
    keep = [np.ascontiguousarray(xy.T.ravel()), np.array([0.0, 0.3, 0.9]),
            np.random.default_rng(8).standard_normal(2 * 2 * npo), np.array([[2, 3], [3, 2]], dtype=np.int32)]
    a = L.hmsc_krige_args()
    a.device, a.np, a.nn, a.sDim, a.G, a.S, a.nfmax, a.mode, a.nNeighbours, a.level = device, npo, nn, 2, 3, 2, 2, 2, 5, 0
    a.seed = 1
    a.coords, a.alphas, a.Eta, a.alpha = L.fptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2]), L.iptr(keep[3])
    out = np.zeros(2 * 2 * nn)
    return _rc(L.lib().hmsc_krige(C.byref(a), L.fptr(out)))


def _eval(device):
    a, u, x = np.array([-1.0, 0.5, 26.0]), np.array([0.25, 0.5, 0.75]), np.zeros(3)
    return _rc(L.lib().hmsc_debug_eval(device, b"trunc_normal_tab", 3, L.fptr(a), L.fptr(u), L.fptr(x), None))


ONE_SHOTS = dict(predict=_predict, post_omega=_omega, variance_partitioning=_vp, effective_size=_ess,
                 dense_chol_solve=_chol, spatial_full_grid=_grid, krige=_krige, debug_eval=_eval)


@pytest.mark.parametrize("name", list(ONE_SHOTS))
def test_one_shot_call_holds_nothing_afterwards(baseline, name):
    rc, msg = ONE_SHOTS[name](0)
    assert rc == 0, msg
    assert live() == baseline


def test_refused_one_shot_calls_hold_nothing_afterwards(baseline):
    rc, msg = _predict(0, bad_pi=True)              # refused after five uploads
    assert rc == -1 and "predict: Pi out of range" in msg
    assert live() == baseline
    # two new units at identical coordinates (tests/test_gpu_krige.py test_indefinite_w_is_refused)
    xy = np.random.default_rng(6).random((32, 2))
    xy[31] = xy[30]
    rl, names, newn, _ = KC.make_level(30, 2, 0, xy=xy)
    eta, alpha = KC.make_posterior(rl, 30, 6)
    with pytest.raises(L.HmscNativeError, match="W = K22 - K12' K11\\^-1 K12 of the new units is not positive definite"):
        predictLatentFactor(newn, names, eta, rl, postAlpha=alpha, device=0, seed=1)
    assert live() == baseline


def test_one_shot_calls_leave_the_callers_device(baseline):
    n = np.zeros(1, dtype=np.int32)
    L.check(L.lib().hmsc_device_count(L.iptr(n)))
    if n[0] < 2:
        pytest.skip("one visible device")
    hip = C.CDLL("libamdhip64.so")
    cur = C.c_int(-1)
    assert hip.hipSetDevice(0) == 0
    for name, f in ONE_SHOTS.items():
        rc, msg = f(1)
        assert rc == 0, (name, msg)
        assert hip.hipGetDevice(C.byref(cur)) == 0 and cur.value == 0, name
        assert live() == baseline, name


def test_grown_workspace_keeps_one_live_buffer(baseline):
    """updateGammaEta's workspace is sized for nfMin and regrown when updateNf adds a factor
    (the config-3 model of tests/test_gpu_config3.py, which grows within 40 adaptive sweeps):
    the old buffer goes, so the chain holds as many buffers as before."""
    hM = W.vignette3_phylo(ns=300, ny=200)
    ch = H.Chain(hM, 30303, device=0, updater={})
    ch.init([2])
    before = live()
    it = 0
    while int(ch.nf()[0]) <= 2 and it < 40:
        it += 1
        ch.sweep(it, adapt=True)
    assert int(ch.nf()[0]) > 2, "nf never grew: the test did not exercise the regrowth"
    ch.sweep(it + 1)                                # updateGammaEta at the larger nf: the workspace regrown
    ch.sync()
    assert live() == before
    ch.close()
    assert live() == baseline
