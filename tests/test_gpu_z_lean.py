"""updateZ's lean pair draw (chains without NA cells) against the general one and the oracle.

An all-probit chain without NA cells whose iSigma was never set from outside (unit scale) draws
its pairs by z_probit_pair_lean (z_kernel.h LEAN: signs as sign bits, no NA handling, no sd / isd,
trimmed addresses and guards).  HMSC_Z_GENERAL=1, read when the chain is created, keeps such a
chain on the general draw, and debug_get("zlean") says which one the last launch took (0 general,
1 lean).  The lean draw is the general one bit for bit, so

  * Z and XZ after three sweeps are equal by bytes with the switch off and on, at shapes whose
    last site tile and last wave sub-tile are ragged (ny = 70, 130, 262) and whose last species
    block ends inside a pair (ns = 37), one case per K bucket (K = 10, 30, 40, 60, 70: NKB 1, 2,
    3, 4, 8), one under a forced schedule of two two-tile chunks and a one-tile tail; with iSigma
    set from outside (probit iSigma off 1: sd and isd act) the lean draw is not taken;
  * an all-probit chain (lean draw) and the same data with one normal species added (NORMAL
    kernel, general draw) are each held to the oracle at test_gpu_fullsize.py's tolerance for the Z
    draw, and the probit species' Z is equal by bytes between the two;
  * a chain with NA cells stays on the general draw (zlean == 0) and is held to the oracle, with
    noise and in noise_zero mode;
  * a state built so that every Y pattern of a pair meets E of both signs, with |E| = 30 in one
    cell of the pair and |E| < 2 in the other (alpha > 25 in one cell and not in its partner, in
    either position): the lean and the general draw agree by bytes and with the oracle
    cell by cell at test_gpu_z_tails.py's bound.
"""
import os
import re

import numpy as np
import pandas as pd
import pytest

from helpers import H, O, oracle_model, rel_err, synthetic_model
from oracle.rng import Rng
from test_gpu_parity import TOL_DRAW, _state_from_oracle
from test_gpu_z_tails import TOL_X

pytestmark = pytest.mark.gpu

SEED, IT = 24681357, 5
UP = {"GammaEta": False}
KNOBS = ("HMSC_Z_SCHED", "HMSC_Z_CHUNKS", "HMSC_Z_GENERAL")


def _fullsize_tol():
    """The tolerance test_gpu_fullsize.py holds the Z draw to, read from its source."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_fullsize.py")).read()
    return float(re.search(r'locals\(\)\.get\("tol", ([0-9.e-]+)\)', src).group(1))


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _zlean(ch):
    return int(ch.debug_get("zlean", 1)[0])


def _xz(ch, hM):
    K = int(ch.debug_get("dims", 8)[0])
    return ch.debug_get("XZ", K * hM.ns)


CASES = {
    "k10": (dict(ny=70, ns=37, nc=4, nf=6), {}),
    "k30": (dict(ny=130, ns=37, nc=20, nf=10), {}),
    "k40": (dict(ny=70, ns=37, nc=30, nf=10), {}),
    "k60": (dict(ny=70, ns=37, nc=50, nf=10), {}),
    "k70": (dict(ny=130, ns=37, nc=60, nf=10), {}),
    # five tiles, the last with six sites: two chunks of two tiles (tile-ahead loads), a one-tile tail
    "k30_sched": (dict(ny=262, ns=37, nc=20, nf=10), {"HMSC_Z_SCHED": "2x2,1x1"}),
}
_models = {}


def _three_sweeps(monkeypatch, hM, env, isig):
    _env(monkeypatch, env)
    ch = H.Chain(hM, SEED, device=0, updater=UP)
    ch.init()
    if isig is not None:
        ch.set_state({"iSigma": isig})
    for it in range(1, 4):
        ch.sweep(it)
    out = (_zlean(ch), int(ch.debug_get("dims", 8)[4]), ch.get_state()["Z"], _xz(ch, hM))
    ch.close()
    return out


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("name", list(CASES))
def test_lean_equals_general(monkeypatch, name, scaled):
    spec, env = CASES[name]
    if name not in _models:
        _models[name] = synthetic_model(**spec)
    hM = _models[name]
    isig = np.random.default_rng(3).uniform(0.5, 2.0, hM.ns) if scaled else None
    lean, nchunk, Z, XZ = _three_sweeps(monkeypatch, hM, env, isig)
    lean_g, nchunk_g, Zg, XZg = _three_sweeps(monkeypatch, hM, dict(env, HMSC_Z_GENERAL="1"), isig)
    want = 0 if scaled else 1  # (iSigma set from outside: not known to be 1)
    print(name, "scaled" if scaled else "unit", "zlean", lean, lean_g, "chunks", nchunk)
    assert lean == want and lean_g == 0
    assert nchunk == nchunk_g and (not env or nchunk == 3)
    assert np.isfinite(Z).all()
    assert Z.tobytes() == Zg.tobytes()
    assert XZ.tobytes() == XZg.tobytes()


def _draw(monkeypatch, hM, st, env=None, noise_zero=False):
    _env(monkeypatch, env or {})
    ch = H.Chain(hM, SEED, device=0, updater=UP)
    ch.init()
    ch.set_state(st)
    if noise_zero:
        ch.set_noise_mode(1)
    ch.update("Z", IT)
    out = (_zlean(ch), ch.get_state()["Z"], _xz(ch, hM))
    ch.close()
    return out


def _without_sigma(st):
    return {k: v for k, v in st.items() if k not in ("iSigma", "sigma")}


def test_unit_scale_and_normal_neighbour(monkeypatch):
    tol = _fullsize_tol()
    assert tol == TOL_DRAW
    hA = synthetic_model(ny=130, ns=37, nc=4, nf=3, seed=5)
    mA = oracle_model(hA)
    stA, _ = _state_from_oracle(mA, SEED)
    assert np.all(stA["iSigma"] == 1.0)
    # the same data with one normal species appended (species 37: the probit species keep
    # their Philox blocks and, from the same state, their E)
    rng = np.random.default_rng(11)
    yn = rng.standard_normal(hA.ny) * 2.0 + 1.0
    units = np.asarray(hA.studyDesign["lev0"])
    rl = H.HmscRandomLevel(units=units)
    H.setPriors(rl, nfMin=3, nfMax=3)
    hB = H.Hmsc(Y=np.column_stack([hA.Y, yn]), X=hA.X, covNames=list(hA.covNames), XScale=True, YScale=False,
                distr=["probit"] * hA.ns + ["normal"], studyDesign=pd.DataFrame({"lev0": units}),
                ranLevels={"lev0": rl})
    mB = oracle_model(hB)
    np.testing.assert_array_equal(mB["X"], mA["X"])
    np.testing.assert_array_equal(mB["Pi"], mA["Pi"])
    stB = dict(stA)
    col = lambda a, v: np.column_stack([a, np.full(a.shape[0], v)])  # noqa: E731
    stB["Beta"] = col(stA["Beta"], 0.25)
    stB["Lambda"] = [col(stA["Lambda"][0], -0.5)]
    stB["Psi"] = [col(stA["Psi"][0], 1.0)]
    stB["iSigma"] = np.append(stA["iSigma"], 0.7)
    stB["Z"] = np.column_stack([stA["Z"], yn])

    leanA, ZA, _ = _draw(monkeypatch, hA, _without_sigma(stA))
    leanB, ZB, _ = _draw(monkeypatch, hB, stB)
    ZoA = O.update_z(stA, mA, Rng(SEED), IT)
    ZoB = O.update_z(stB, mB, Rng(SEED), IT)
    eA, eB = rel_err(ZA, ZoA), rel_err(ZB, ZoB)
    print("all probit zlean", leanA, "Z", eA, "| with a normal species zlean", leanB, "Z", eB)
    assert leanA == 1 and leanB == 0
    assert eA < tol and eB < tol
    np.testing.assert_array_equal(ZB[:, -1], mB["Y"][:, -1])
    assert ZB[:, :hA.ns].tobytes() == ZA.tobytes()


@pytest.mark.parametrize("noise_zero", [False, True], ids=["noise", "noise_zero"])
def test_na_chain_keeps_general_draw(monkeypatch, noise_zero):
    hM = synthetic_model(ny=130, ns=37, nc=4, nf=3, na_frac=0.05, seed=3)
    m = oracle_model(hM)
    st, _ = _state_from_oracle(m, SEED)
    lean, Z, _ = _draw(monkeypatch, hM, st, noise_zero=noise_zero)
    Zo = O.update_z(st, m, Rng(SEED), IT)
    na = np.isnan(m["Y"])
    assert na.sum() > 100
    if noise_zero:  # an NA cell's draw without its noise is E
        Zo[na] = O.linear_predictor(st, m)[na]
    e = rel_err(Z, Zo)
    print("NA chain zlean", lean, "noise_zero", noise_zero, "Z", e)
    assert lean == 0
    assert e < TOL_DRAW


def test_pair_patterns_signs_and_deep_partner(monkeypatch):
    """E = b0_j + small terms with b0 = (+30, 0.3 | -0.5, -30 | -30, 0.3 | 0.5, +30 | 0.4, -0.6) over
    five pairs: the first cell of a pair is deep (alpha > 25) where E = +30 meets y = 0 or E = -30
    meets y = 1, likewise the second, the partner never, and the fifth pair stays on the table
    path; Y is independent of E, so every pattern meets each kind of pair."""
    hM = synthetic_model(ny=70, ns=37, nc=4, nf=3, seed=9)
    m = oracle_model(hM)
    st = O.compute_initial_parameters(m, Rng(SEED))
    b0 = np.array([30.0, 0.3, -0.5, -30.0, -30.0, 0.3, 0.5, 30.0, 0.4, -0.6])[np.arange(hM.ns) % 10]
    st["Beta"] = np.vstack([b0, 0.2 * np.cos(np.arange(3 * hM.ns)).reshape(3, hM.ns)])
    st["Lambda"] = [np.zeros_like(st["Lambda"][0])]
    E = O.linear_predictor(st, m)
    Y = m["Y"]
    alpha = -np.where(Y == 1, 1.0, -1.0) * E
    deep = alpha > 25.0
    npair = hM.ns // 2
    y0, y1 = Y[:, 0:2 * npair:2], Y[:, 1:2 * npair:2]
    d0, d1 = deep[:, 0:2 * npair:2], deep[:, 1:2 * npair:2]
    e0, e1 = E[:, 0:2 * npair:2], E[:, 1:2 * npair:2]
    for a in (0, 1):
        for b in (0, 1):
            pat = (y0 == a) & (y1 == b)
            assert (pat & d0 & ~d1).any() and (pat & ~d0 & d1).any(), (a, b)
            assert (pat & ~d0 & ~d1).any(), (a, b)
            assert (pat & (e0 > 0)).any() and (pat & (e0 < 0)).any(), (a, b)
            assert (pat & (e1 > 0)).any() and (pat & (e1 < 0)).any(), (a, b)
    assert (d0 & ~d1).any() and (~d0 & d1).any()
    Zo = O.update_z(st, m, Rng(SEED), IT)
    lean2, Z2, XZ2 = _draw(monkeypatch, hM, _without_sigma(st))
    lean1, Z1, XZ1 = _draw(monkeypatch, hM, st)   # iSigma set (to 1): the general draw
    lean0, Z0, XZ0 = _draw(monkeypatch, hM, _without_sigma(st), env={"HMSC_Z_GENERAL": "1"})
    assert (lean2, lean1, lean0) == (1, 0, 0)
    xref = Zo - E
    err = np.abs(Z2 - Zo) / np.maximum(1.0, np.abs(xref))
    bound = TOL_X + 2 * np.spacing(np.abs(E)) / np.maximum(1.0, np.abs(xref))
    k = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    print("worst cell", k, "err", err[k], "bound", bound[k], "deep cells", int(deep.sum()), "normwise", rel_err(Z2, Zo))
    assert np.isfinite(Z2).all()
    assert (err <= bound).all(), (k, err[k], bound[k])
    assert rel_err(Z2, Zo) < TOL_DRAW
    assert Z2.tobytes() == Z0.tobytes() and Z1.tobytes() == Z0.tobytes()
    assert XZ2.tobytes() == XZ0.tobytes() and XZ1.tobytes() == XZ0.tobytes()
