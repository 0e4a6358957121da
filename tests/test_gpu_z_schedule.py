"""updateZ's launch: the site-chunk schedule, the timer record and the padded species block.

The z grid's site chunks follow a schedule of segments (n chunks of t tiles, t descending);
HMSC_Z_SCHED forces one when the chain is created, HMSC_Z_CHUNKS a uniform one.  A draw depends
on its site and species only, so Z is bit-equal between schedules; XZ moves by the grouping of
its partial sums and is held to its definition on the stored Z at 1e-12, as
test_gpu_z_pipeline.py holds it.  The live timer counts one launch per sweep on a grid of any
size, and a shard must start at a species quad.
"""
import time

import numpy as np
import pytest

from helpers import H, O, oracle_model, rel_err, synthetic_model
from hmsc_amd import _lib as L
from oracle.rng import Rng
from test_gpu_parity import MODELS, TOL_DRAW, _state_from_oracle

pytestmark = pytest.mark.gpu

SEED = 987654321
IT = 7
KNOBS = ("HMSC_Z_SCHED", "HMSC_Z_CHUNKS", "HMSC_DEBUG_SHARD_START")

SCHED_CASES = {
    "t1": dict(ny=64, ns=40, nc=4, nf=3),
    "t2_ragged": dict(ny=65, ns=40, nc=4, nf=3),
    "t3_ragged": dict(ny=130, ns=40, nc=4, nf=3),
    "t9_ragged": dict(ny=64 * 8 + 5, ns=40, nc=4, nf=3),
    "k30": dict(ny=130, ns=40, nc=20, nf=10, seed=10),
    "na": dict(ny=64 * 8 + 5, ns=40, nc=4, nf=3, na_frac=0.05, seed=3),
}
# the last: a list longer than any case's tiles
SCHEDULES = ["2x3,1x2,1x1", "1x4,1", "1x1", "1x4,2x2,3x1,64x1"]

PAD_MODELS = {
    "probit": dict(nc=4, nf=3),
    "mixed_normal": dict(MODELS["mixed_normal"]),
    "mixed_poisson": dict(MODELS["mixed_poisson"]),
    "na": dict(nc=4, nf=3, na_frac=0.05, seed=3),
}

_cache = {}


def _setup(key, spec):
    """Model, oracle model, the oracle's state after two sweeps and its Z draw, once per case."""
    if key not in _cache:
        hM = synthetic_model(**spec)
        m = oracle_model(hM)
        st, _ = _state_from_oracle(m, SEED)
        _cache[key] = (hM, m, st, O.update_z(st, m, Rng(SEED), IT))
    return _cache[key]


def _expected_chunks(sched, n_tiles):
    """The schedule cut where the tiles end, its last segment extended to cover them: chunk
    count, and the tiles of every chunk (none empty)."""
    segs = []
    for item in sched.split(","):
        n, t = (int(v) for v in item.split("x")) if "x" in item else (1, int(item))
        segs.append((n, t))
    chunks, rem = [], n_tiles
    for g, (n, t) in enumerate(segs):
        if rem <= 0:
            break
        need = -(-rem // t)
        for _ in range(need if (g == len(segs) - 1 or n >= need) else n):
            chunks.append(min(t, rem))
            rem -= chunks[-1]
    assert rem == 0 and all(c > 0 for c in chunks) and sum(chunks) == n_tiles
    return len(chunks)


def _draw(monkeypatch, hM, m, st, env):
    """One updateZ from the oracle's state under the given create-time knobs: Z, the errors of XZ
    and ZTr against their definitions on that Z, and dims[4]."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ch = H.Chain(hM, SEED, device=0, updater={"GammaEta": False})
    ch.init()
    ch.set_state(st)
    nchunk = int(ch.debug_get("dims", 8)[4])
    ch.update("Z", IT)
    Z = ch.get_state()["Z"]
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
    return Z, exz, eztr, nchunk


def _uniform(monkeypatch, key, spec):
    """The case under HMSC_Z_CHUNKS=1, held to the oracle's draw; computed once."""
    hM, m, st, Zo = _setup(key, spec)
    if ("uniform", key) not in _cache:
        Z, exz, eztr, nchunk = _draw(monkeypatch, hM, m, st, {"HMSC_Z_CHUNKS": "1"})
        ez = rel_err(Z, Zo)
        print(key, "uniform Z", ez, "XZ", exz, "ZTr", eztr)
        assert nchunk == 1
        assert ez < TOL_DRAW and exz < 1e-12 and eztr < 1e-12, (key, ez, exz, eztr)
        _cache[("uniform", key)] = Z
    return _cache[("uniform", key)]


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("name", list(SCHED_CASES))
def test_schedule_draws_and_contractions(monkeypatch, name, sched):
    hM, m, st, Zo = _setup(name, SCHED_CASES[name])
    Zu = _uniform(monkeypatch, name, SCHED_CASES[name])
    Z, exz, eztr, nchunk = _draw(monkeypatch, hM, m, st, {"HMSC_Z_SCHED": sched})
    ez = rel_err(Z, Zo)
    print(name, sched, "chunks", nchunk, "Z", ez, "XZ", exz, "ZTr", eztr)
    assert nchunk == _expected_chunks(sched, (hM.ny + 63) // 64), (name, sched, nchunk)
    np.testing.assert_array_equal(Z, Zu)
    assert ez < TOL_DRAW, (name, sched, ez)
    assert exz < 1e-12, (name, sched, exz)
    assert eztr < 1e-12, (name, sched, eztr)


def test_schedule_rejects_increasing_tiles(monkeypatch):
    hM, m, st, _ = _setup("t3_ragged", SCHED_CASES["t3_ragged"])
    monkeypatch.setenv("HMSC_Z_SCHED", "1x1,1x2")
    with pytest.raises(L.HmscNativeError, match="must not increase"):
        H.Chain(hM, SEED, device=0, updater={"GammaEta": False}).close()


def test_default_schedule_small_grid(monkeypatch):
    """Fewer tiles than one round of resident workgroups: one tile per workgroup."""
    name = "t9_ragged"
    hM, m, st, Zo = _setup(name, SCHED_CASES[name])
    Zu = _uniform(monkeypatch, name, SCHED_CASES[name])
    Z, exz, eztr, nchunk = _draw(monkeypatch, hM, m, st, {})
    assert nchunk == (hM.ny + 63) // 64
    np.testing.assert_array_equal(Z, Zu)
    assert exz < 1e-12, exz


def test_default_schedule_two_rounds(monkeypatch):
    """70 tiles x 32 species blocks, more than twice the 1024 z workgroups an MI355X holds at
    once: the default takes two tiles per workgroup in its first round (32 rows of 2, then 6 of
    1), and nothing but XZ's summation order moves against one tile per workgroup."""
    hM = synthetic_model(ny=64 * 70, ns=1000, nc=4, nf=3)
    out = []
    for env in ({"HMSC_Z_CHUNKS": "70"}, {}):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ch = H.Chain(hM, SEED, device=0, updater={"GammaEta": False})
        ch.init()
        nchunk = int(ch.debug_get("dims", 8)[4])
        ch.update("Z", IT)
        K = int(ch.debug_get("dims", 8)[0])
        out.append((nchunk, ch.get_state()["Z"], ch.debug_get("XZ", K * hM.ns)))
        ch.close()
    print("chunks", out[0][0], out[1][0], "XZ", rel_err(out[1][2], out[0][2]))
    assert out[0][0] == 70 and 2 <= out[1][0] < 70
    np.testing.assert_array_equal(out[1][1], out[0][1])
    assert rel_err(out[1][2], out[0][2]) < 1e-12


@pytest.mark.parametrize("ns", [33, 36, 40, 48])
@pytest.mark.parametrize("model", list(PAD_MODELS))
def test_padded_species_block(monkeypatch, model, ns):
    """A last species block of 1, 4, 8 and 16 species: the padded columns are drawn and dropped,
    and leave the valid cells and the contractions as they are defined."""
    spec = dict(PAD_MODELS[model], ny=130, ns=ns)
    hM, m, st, Zo = _setup(("pad", model, ns), spec)
    Z, exz, eztr, _ = _draw(monkeypatch, hM, m, st, {})
    ez = rel_err(Z, Zo)
    print(model, ns, "Z", ez, "XZ", exz, "ZTr", eztr)
    assert ez < TOL_DRAW, (model, ns, ez)
    assert exz < 1e-12, (model, ns, exz)
    assert eztr < 1e-12, (model, ns, eztr)


@pytest.mark.parametrize("shape", [dict(ny=130, ns=40), dict(ny=64 * 40, ns=64)], ids=["under8", "over8"])
def test_timer_counts_launches(monkeypatch, shape):
    """Three launches, each with a start and an end no further apart than the run's wall time,
    on a grid of 6 workgroups and on one of 80."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    hM = synthetic_model(nc=4, nf=3, **shape)
    ch = H.Chain(hM, SEED, device=0, updater={"GammaEta": False})
    ch.init()
    ch.sync()
    ch.kernel_timing(True)
    its = (5, 6, 7)
    t0 = time.perf_counter()
    for it in its:
        ch.update("Z", it)
    ch.sync()
    wall_us = (time.perf_counter() - t0) * 1e6
    total_us, n = ch.kernel_timing_get("z")
    KT_SLOTS, KT_N = 8192, 7
    kt = ch.debug_get("kt", KT_N * 2 * KT_SLOTS).reshape(KT_N, 2, KT_SLOTS)
    ch.close()
    dur_us = (kt[0, 1, list(its)] - kt[0, 0, list(its)]) * 0.01  # 100 MHz wall clock
    print(shape, "launches", n, "total", total_us, "each", dur_us, "wall", wall_us)
    assert n == 3
    assert np.all(dur_us > 0.0) and np.all(dur_us <= wall_us), (dur_us, wall_us)
    assert 0.0 < total_us <= wall_us


def test_shard_start_guard(monkeypatch):
    """A species shard must start at a species quad (the Philox block index is (sp0 + j) >> 2)."""
    hM = synthetic_model(ny=64, ns=40, nc=4, nf=3)
    monkeypatch.setenv("HMSC_DEBUG_SHARD_START", "2")
    with pytest.raises(L.HmscNativeError, match="multiple of 4 species"):
        H.Chain(hM, SEED, device=0, updater={"GammaEta": False}).close()
    monkeypatch.setenv("HMSC_DEBUG_SHARD_START", "4")
    H.Chain(hM, SEED, device=0, updater={"GammaEta": False}).close()
