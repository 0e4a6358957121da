"""Launch buckets of the fused sweep that no other module pins: each shape runs three complete
sweeps against the oracle and a recorded run as graph replays against the eager launch sequence.

The side chain (side_chain_kernel) is instantiated per wv_bucket_gv(nc nt) = 8, 16, 20, 24, 32.
test_gpu_parity.py holds 8 and 16 (its models' nc nt = 3 .. 12) and 20 (bench_dims: nc = 20) to
the oracle, and the fused Eta kernel's nf buckets are tests/test_gpu_eta_tile_solve.py's; the 24
bucket (nc nt = 21 .. 24) is held here."""
import numpy as np
import pytest

from helpers import H, O, oracle_model, rel_err, synthetic_model
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

UP = {"GammaEta": False}
SEED = 987654321

# nc nt = 22 (side chain bucket 24), K = nc + nf = 27 (BetaLambda bucket 32), nf = 16 (Eta bucket 16)
SHAPES = {
    "side24": dict(ny=160, ns=40, nc=11, nt=2, nf=16, seed=34),
}


@pytest.fixture(scope="module", params=list(SHAPES))
def setup(request):
    """The model, the oracle's state two sweeps in, and its state after sweeps 10 .. 12, once."""
    hM = synthetic_model(**SHAPES[request.param])
    m = oracle_model(hM)
    rng = Rng(SEED)
    st = O.compute_initial_parameters(m, rng)
    for it in (1, 2):
        st = O.sweep(st, m, rng, it, updater=UP)
    rng = Rng(SEED)
    o = st
    for it in range(10, 13):
        o = O.sweep(o, m, rng, it, updater=UP)
    return request.param, hM, st, o


def test_full_sweeps_track_oracle(setup):
    name, hM, st, o = setup
    ch = H.Chain(hM, SEED, device=0, updater=UP)
    ch.init()
    ch.set_state(st)
    for it in range(10, 13):
        ch.sweep(it)
    g = ch.get_state()
    g2bl, eta = ch.debug_get("g2bl", 2), ch.debug_get("eta_fused", 3)
    ch.close()
    assert g2bl[1] > 0 and eta[0] >= 3, "the sweeps did not take the fused launches"
    for k in ("Beta", "Gamma", "iV", "Z"):
        err = rel_err(g[k], o[k])
        print(name, k, err)
        assert err < 1e-7, (name, k, err)


def test_graph_replay_matches_eager(setup, monkeypatch):
    name, hM, _, _ = setup
    out = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("HMSC_NO_GRAPH", no_graph)
        ch = H.Chain(hM, 77, device=0, updater=UP)
        ch.init()
        rec = ch.run(transient=5, samples=9, thin=1, adaptNf=[0])
        rec2 = ch.run(transient=2, samples=3, thin=1, adaptNf=[0], iter0=14)
        out.append((rec, rec2))
        ch.close()
    for i in range(2):
        for k in ("Beta", "Gamma", "iV", "iSigma", "Lambda0", "Eta0", "Delta0", "Psi0"):
            np.testing.assert_array_equal(out[0][i][k], out[1][i][k], err_msg=f"{name} {k}")
