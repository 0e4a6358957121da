"""updateZ's tile-to-tile path at small sizes.

The z kernel issues a workgroup's staging loads and its first tile's operands in one batch and
carries each tile's E operands into the site loop from the tile before.  At small ny the
launcher makes as many site chunks as tiles, so a workgroup never runs a second tile;
HMSC_Z_CHUNKS (read when the chain is created) forces several tiles per workgroup here.
Every case runs with one and with two chunks and is held to test_gpu_parity.py's tolerances:
Z against the oracle's draw at TOL_DRAW, XZ and ZTr against their definitions on the stored Z
at 1e-12.
"""
import numpy as np
import pytest

from helpers import H, O, oracle_model, rel_err, synthetic_model
from oracle.rng import Rng
from test_gpu_parity import MODELS, TOL_DRAW, _state_from_oracle

pytestmark = pytest.mark.gpu

SEED = 987654321

CASES = {
    # one exact tile: no next tile to load operands for
    "one_tile": dict(ny=64, ns=40, nc=4, nf=3),
    # the second tile holds one site: three of the four waves leave the loop after the first
    "ragged_second": dict(ny=65, ns=40, nc=4, nf=3),
    # three tiles in one chunk, the last ragged
    "ragged_last": dict(ny=130, ns=40, nc=4, nf=3),
    # a second species block of one species
    "ragged_species": dict(ny=200, ns=33, nc=3, nf=2),
    # the instantiations by K: NKB = 1 (K = 5), 2 (K = 30, the benchmark's), 8 (K = 70)
    "nkb1": dict(ny=130, ns=40, nc=3, nf=2),
    "nkb2": dict(ny=130, ns=40, nc=20, nf=10, seed=10),
    "nkb8": dict(ny=130, ns=40, nc=60, nf=10, seed=13),
    # HAS_NA: the XZ mask re-reads the Y words; ZTr is formed
    "na": dict(ny=130, ns=40, nc=4, nf=3, na_frac=0.05, seed=3),
    # the generic branch (in-loop stores): normal species, Poisson species
    "mixed_normal": dict(MODELS["mixed_normal"], ny=130),
    "mixed_poisson": dict(MODELS["mixed_poisson"], ny=130),
}

_cache = {}


def _setup(name):
    """Model, oracle model and the oracle's state after two sweeps, computed once per case."""
    if name not in _cache:
        hM = synthetic_model(**CASES[name])
        m = oracle_model(hM)
        st, _ = _state_from_oracle(m, SEED)
        _cache[name] = (hM, m, st)
    return _cache[name]


def _chain(monkeypatch, hM, st, chunks):
    monkeypatch.setenv("HMSC_Z_CHUNKS", str(chunks))
    ch = H.Chain(hM, SEED, device=0, updater={"GammaEta": False})
    ch.init()
    ch.set_state(st)
    n_tiles = (hM.ny + 63) // 64
    assert int(ch.debug_get("dims", 8)[4]) == min(n_tiles, chunks)
    return ch


@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_z_draw_and_contractions(monkeypatch, name, chunks):
    hM, m, st = _setup(name)
    it = 7
    ch = _chain(monkeypatch, hM, st, chunks)
    ch.update("Z", it)
    Z = ch.get_state()["Z"]
    Zo = O.update_z(st, m, Rng(SEED), it)
    ez = rel_err(Z, Zo)
    XEta, _ = O._xeta_and_prior(dict(st, Z=Z), m)
    K = XEta.shape[1]
    Yx = ~np.isnan(m["Y"])
    XZ = ch.debug_get("XZ", K * hM.ns).reshape(hM.ns, K).T
    exz = rel_err(XZ, XEta.T @ np.where(Yx, Z, 0.0))
    eztr = 0.0
    if np.isnan(m["Y"]).any():  # Z Tr is formed only where it is consumed (NA models)
        ZTr = ch.debug_get("ZTr", hM.ny * hM.nt).reshape(hM.nt, hM.ny).T
        eztr = rel_err(ZTr, Z @ m["Tr"])
    ch.close()
    print(name, chunks, "Z", ez, "XZ", exz, "ZTr", eztr)
    assert ez < TOL_DRAW, (name, chunks, ez)
    assert exz < 1e-12, (name, chunks, exz)
    assert eztr < 1e-12, (name, chunks, eztr)


@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("name", ["ragged_last", "na"])
def test_z_refresh_feeds_gamma2(monkeypatch, name, chunks):
    """DRAW = false: after set_state the contractions of the given Z are formed by the z
    kernel's refresh pass, which updateGamma2 then consumes."""
    hM, m, st = _setup(name)
    it = 7
    ch = _chain(monkeypatch, hM, st, chunks)
    ch.update("Gamma2", it)
    Gm = ch.get_state()["Gamma"]
    ch.close()
    e = rel_err(Gm, O.update_gamma2(st, m, Rng(SEED), it))
    print(name, chunks, "Gamma", e)
    assert e < TOL_DRAW, (name, chunks, e)


def test_z_graph_replay_matches_eager(monkeypatch):
    """Captured sweeps add the pack row and the G row to the z grid: with two site chunks (three
    tiles in the first) a run of graph replays equals the eager launch sequence bit for bit."""
    hM = synthetic_model(ny=300, ns=40, nc=4, nf=3, nt=2, seed=12)
    monkeypatch.setenv("HMSC_Z_CHUNKS", "2")
    monkeypatch.setenv("HMSC_GRAPH_SWEEPS", "4")
    runs = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("HMSC_NO_GRAPH", no_graph)
        ch = H.Chain(hM, 77, device=0, updater={"GammaEta": False})
        ch.init()
        runs.append(ch.run(transient=3, samples=8, thin=1, adaptNf=[0]))
        ch.close()
    for k in ("Beta", "Gamma", "iV", "iSigma", "Lambda0", "Eta0", "Delta0", "Psi0"):
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
