"""updateZ's draws cell by cell, tails and table edges included.

The parity tests compare Z with the oracle at fitted states, where |E| is a few units, by the
normwise rel_err at 1e-9: most rows of the z kernel's tables, the hand-over at alpha = 25, the
clamp at a = 17.99 and AS241's tail are visited by no cell there, and an absolute error of
1e-9 max|Z| would pass on every cell.  Here the state is built so that one updateZ visits all
of them (draw_reference.tails_design: E = b0_j + b1_j x_i spans +-8 on even and +-30 on odd
species, Lambda = 0, Y a fixed 0/1 pattern independent of E, so alpha = -+E takes both signs
everywhere), and every cell is compared on the standardised variate:

    |Z - Z_ref| / (sd max(1, |x_ref|)),   x_ref = (Z_ref - E) / sd,   Z_ref = oracle update_z

The bound is that of the draw functions (test_gpu_draw_functions.py: 1e-12 per draw, held there
against mpmath; the oracle itself is held to mpmath at 1e-13 in test_oracle_rng.py) plus two ulp
of |E| for the device's own summation of E.  No cell is excluded.

Before any comparison the coverage is asserted on the CPU from the oracle's own p and w, with
the segmentation of z_tables.h restated in draw_reference (width 1/4 in a = min(|alpha| / sqrt 2,
17.99), width 1/4 in w = -log(4 p (1 - p))): every one of the 72 erfcx segments holds at least 10
and every one of the 64 quantile segments at least 5 of the cells that take the table path.

Variants: all probit; 5 % NA (HAS_NA, alpha = -inf); with normal species (NORMAL); with Poisson
species, where the probit cells go through z_probit_draw / rng.h instead and the Poisson cells'
previous Z sweeps zPrev - log 1000 over the branches of pg_moments.  Each with one and with two
site chunks (four and two tiles per workgroup).

Measured on an MI355X (worst cell, the same for both chunkings; bound 1e-12 + 2 ulp|E|):
    probit, probit_na, normal 1.9e-14 (the partner of a deep cell, on the scalar path);
    poisson: probit cells 1.2e-13; Poisson cells |dZ| <= 8.9e-16, 2 % of the cell's bound
    (rel_err_elem 5.8e-14 against a derived 2.7e-11); XZ 9e-16; the two pinned upper-tail
    cells 3e-16 (the earlier formula is 5.5e-11 off at the second: 1 - p from the rounded p).
"""
import numpy as np
import pandas as pd
import pytest

import draw_reference as D
from helpers import H, O, oracle_model, rel_err, rel_err_elem
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

SEED, IT = D.TAILS_SEED, D.TAILS_IT
NY, NS = D.TAILS_NY, D.TAILS_NS
TOL_X = 1e-12          # the draw functions' bound (test_gpu_draw_functions.py)
N_OTHER = 8            # normal / Poisson species of the mixed variants (species 0 .. 7)
VARIANTS = ["probit", "probit_na", "normal", "poisson"]

_cache = {}


def _build(variant):
    """(hM, oracle model, state): computed once per variant."""
    if variant in _cache:
        return _cache[variant]
    x, b0, A, Y = D.tails_design()
    Y = Y.copy()
    distr = ["probit"] * NS
    i, j = np.meshgrid(np.arange(NY), np.arange(N_OTHER), indexing="ij")
    if variant == "probit_na":
        Y[np.random.default_rng(6).random(Y.shape) < 0.05] = np.nan
    elif variant == "normal":
        Y[:, :N_OTHER] = np.sin(0.37 * i + j) * 3.0 + 0.5
        distr[:N_OTHER] = ["normal"] * N_OTHER
    elif variant == "poisson":
        Y[:, :N_OTHER] = np.array([0.0, 3.0, 4000.0])[(i + 2 * j) % 3]   # b = y + 1000 in {1000, 1003, 5000}
        distr[:N_OTHER] = ["poisson"] * N_OTHER
    units = np.array([f"u{k:04d}" for k in range(NY)])
    rl = H.HmscRandomLevel(units=units)
    H.setPriors(rl, nfMin=2, nfMax=2)
    hM = H.Hmsc(Y=Y, X=np.column_stack([np.ones(NY), x]), covNames=["(Intercept)", "x1"], XScale=True, YScale=False,
                distr=distr, studyDesign=pd.DataFrame({"lev0": units}), ranLevels={"lev0": rl})
    m = oracle_model(hM)
    st = O.compute_initial_parameters(m, Rng(SEED))
    _, b1 = D.tails_linear_predictor(m["X"][:, 1])
    st["Beta"] = np.vstack([b0, b1])
    st["Lambda"] = [np.zeros_like(st["Lambda"][0])]
    if variant == "poisson":   # zPrev - log r sweeps the |c| list of pg_moments, both signs
        c = np.concatenate([D.PG_ABS_C, -D.PG_ABS_C])
        st["Z"] = st["Z"].copy()
        st["Z"][:, :N_OTHER] = D.LOG_R + c[(i * N_OTHER + j) % len(c)]
    _cache[variant] = (hM, m, st)
    return _cache[variant]


def _cells(variant):
    """Per-cell quantities of the oracle's draw: E, sd, alpha, u, p, w, the probit mask and the
    mask of cells whose pair takes the table path."""
    from scipy.special import erfc
    hM, m, st = _build(variant)
    E = O.linear_predictor(st, m)
    sd = np.broadcast_to(st["iSigma"] ** -0.5, E.shape)
    Y = m["Y"]
    fam = np.broadcast_to(m["distr"][:, 0][None, :], E.shape)
    na = np.isnan(Y)
    alpha = np.where(na, -np.inf, -np.where(Y == 1, 1.0, -1.0) * E / sd)
    _, u = D.tails_uniforms(SEED, IT)
    drawn = (fam == 2) | na                     # truncated-normal cells (NA cells of any family)
    deep = alpha > D.TAIL_ALPHA
    pair_deep = deep | deep.reshape(NY, NS // 2, 2)[:, :, ::-1].reshape(NY, NS)   # species 2m, 2m + 1
    p = u * 0.5 * erfc(alpha / D.SQRT2)
    w = D.quantile_w(p)
    return dict(E=E, sd=sd, alpha=alpha, u=u, p=p, w=w, drawn=drawn, table=drawn & ~pair_deep, deep=deep,
                partner=drawn & pair_deep & ~deep)


def _assert_coverage(variant, c):
    if variant == "poisson":   # rng.h: every branch of trunc_normal_lower / qnorm_fast, and of pg_moments
        d = c["drawn"]
        n = [np.sum(d & c["deep"]), np.sum(d & ~c["deep"] & (c["w"] < 6.25)),
             np.sum(d & ~c["deep"] & (c["w"] >= 6.25) & (c["w"] < 16)), np.sum(d & ~c["deep"] & (c["w"] >= 16))]
        print(variant, "cells by branch (alpha > 25, w < 6.25, w < 16, AS241 tail):", n)
        assert min(n) >= 100
        return
    t = c["table"]
    ne = np.bincount(D.erfcx_segment(c["alpha"][t]), minlength=D.E_SEG)
    qs = D.quantile_segment(c["w"][t])
    nq = np.bincount(qs[qs >= 0], minlength=D.Q_SEG)
    print(variant, "table cells", int(t.sum()), "min per erfcx segment", ne.min(), "per quantile segment", nq.min(),
          "AS241 tail", int(np.sum(qs < 0)), "alpha > 25", int(np.sum(c["deep"] & c["drawn"])),
          "partners on the scalar path", int(c["partner"].sum()), "clamped a", int(np.sum(t & (c["alpha"] < -25.45))))
    assert ne.min() >= 10, ne
    assert nq.min() >= 5, nq
    assert np.sum(qs < 0) >= 100 and c["partner"].sum() >= 100
    assert np.sum(t & (c["alpha"] < -25.45) & np.isfinite(c["alpha"])) >= 10   # the a = 17.99 clamp
    assert np.sum(t & (c["alpha"] < 0) & (c["p"] > 0.5)) >= 100               # p = u (1 - r)


def _chain(monkeypatch, hM, st, chunks):
    monkeypatch.setenv("HMSC_Z_CHUNKS", str(chunks))
    ch = H.Chain(hM, SEED, device=0, updater={"GammaEta": False})
    ch.init()
    ch.set_state(st)
    assert int(ch.debug_get("dims", 8)[4]) == min((NY + 63) // 64, chunks)
    return ch


def _poisson_bound(c, st, m, cols):
    """Per-cell bound on |dZ| of a Poisson cell from the bounds of its parts (1e-13 relative on
    the PG mean m and variance v, 1e-12 max(1, |q|) on each normal quantile q):
        omega = m + sqrt(v) q1:   d_omega / omega <= 1e-13 + sqrt(v) / m (0.5e-13 |q1| + 1e-12 max(1, |q1|))
        sigz = 1 / (prec + omega):  d_sigz / sigz <= d_omega / omega
        Z = log r + sigz A + sqrt(sigz) q2,  A = (y - r) / 2 + prec (E - log r):
        |dZ| <= |sigz A| d_sigz / sigz + sigz prec 2 ulp|E|
                + sqrt(sigz) (0.5 |q2| d_sigz / sigz + 1e-12 max(1, |q2|)) + 4 ulp|Z|."""
    from oracle import rng as R
    y, E, sd = m["Y"][:, cols], c["E"][:, cols], c["sd"][:, cols]
    cell = (np.arange(NY)[:, None] + NY * cols[None, :]).astype(np.uint64)
    u1, u2 = Rng(SEED).uniforms(cell, 0, R.S_ZPOIS, IT)
    q1, q2 = np.abs(R.qnorm_as241(u1.ravel()).reshape(u1.shape)), np.abs(R.qnorm_as241(u2.ravel()).reshape(u2.shape))
    pm, pv = O.pg_moments(y + 1000.0, st["Z"][:, cols] - D.LOG_R)
    omega = pm + np.sqrt(pv) * R.qnorm_as241(u1.ravel()).reshape(u1.shape)
    prec = sd ** -2.0
    sigz = 1.0 / (prec + omega)
    A = (y - 1000.0) / 2.0 + prec * (E - D.LOG_R)
    d_om = 1e-13 + np.sqrt(pv) / pm * (0.5e-13 * q1 + 1e-12 * np.maximum(1.0, q1))
    Zabs = np.abs(D.LOG_R + sigz * A) + np.sqrt(sigz) * q2
    return (np.abs(sigz * A) * d_om + sigz * prec * 2 * np.spacing(np.abs(E))
            + np.sqrt(sigz) * (0.5 * q2 * d_om + 1e-12 * np.maximum(1.0, q2)) + 4 * np.spacing(Zabs))


@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("variant", VARIANTS)
def test_z_cell_by_cell(monkeypatch, variant, chunks):
    hM, m, st = _build(variant)
    c = _cells(variant)
    _assert_coverage(variant, c)
    Zo = O.update_z(st, m, Rng(SEED), IT)

    ch = _chain(monkeypatch, hM, st, chunks)
    ch.update("Z", IT)
    Z = ch.get_state()["Z"]
    XEta, _ = O._xeta_and_prior(dict(st, Z=Z), m)
    K = XEta.shape[1]
    XZ = ch.debug_get("XZ", K * NS).reshape(NS, K).T
    ch.close()

    assert np.isfinite(Z).all()
    E, sd, d = c["E"], c["sd"], c["drawn"]
    xref = (Zo - E) / sd
    err = np.abs(Z - Zo) / (sd * np.maximum(1.0, np.abs(xref)))
    bound = TOL_X + 2 * np.spacing(np.abs(E)) / (sd * np.maximum(1.0, np.abs(xref)))
    ratio = np.where(d, err / bound, 0.0)
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{variant} chunks={chunks}: worst drawn cell {k} err {err[k]:.3e} (bound {bound[k]:.3e}) "
          f"alpha={c['alpha'][k]!r} u={c['u'][k]!r} branch={D.branch_name(c['alpha'][k], c['u'][k])}"
          f"{' (partner of a deep cell)' if c['partner'][k] else ''}; max err {np.max(err[d]):.3e}")
    fam = m["distr"][:, 0]
    normal = np.broadcast_to((fam == 1)[None, :], Z.shape) & ~np.isnan(m["Y"])
    pois = np.nonzero(fam == 3)[0]
    exz = rel_err(XZ, XEta.T @ np.where(~np.isnan(m["Y"]), Z, 0.0))
    print(f"{variant} chunks={chunks}: XZ {exz:.3e}")
    assert (d | normal).sum() + NY * len(pois) == Z.size   # every cell is compared
    assert ratio.max() <= 1.0, (variant, chunks, k, err[k], bound[k])
    np.testing.assert_array_equal(Z[normal], m["Y"][normal])
    if len(pois):
        pb = _poisson_bound(c, st, m, pois)
        dz = np.abs(Z[:, pois] - Zo[:, pois])
        kp = np.unravel_index(int(np.argmax(dz / pb)), dz.shape)
        scale = np.maximum(np.abs(Zo[:, pois]), 1e-3 * np.max(np.abs(Zo[:, pois])))
        ree = rel_err_elem(Z[:, pois], Zo[:, pois])
        print(f"{variant} chunks={chunks}: Poisson cells worst {kp} |dZ| {dz[kp]:.3e} of bound {pb[kp]:.3e}, "
              f"c={st['Z'][:, pois][kp] - D.LOG_R!r} y={m['Y'][:, pois][kp]}; rel_err_elem {ree:.3e} "
              f"(bound {np.max(pb / scale):.3e})")
        assert np.all(dz <= pb), (variant, chunks, kp, dz[kp], pb[kp])
        assert ree <= np.max(pb / scale)
    assert exz < 1e-12, (variant, chunks, exz)


# Cells of the probit variant whose 32-bit uniform lies within 2.8e-8 of 1 while alpha < -6: the
# upper-tail side of AS241's tail branch (p = u (1 - r) > 1 - 2.8e-8), about one cell in 1e8.
# Found by a search of the sweep counter with the oracle's Philox on the CPU (46 and 580 million
# cells); the test re-derives u and checks that the cell qualifies.  The second cell sits where
# 1 - p cannot be formed from the rounded p (alpha = -6.4: that formula is off by 5.5e-11 of
# max(1, |x|); the draws form the complement on its own, rng.h trunc_normal_lower_t); both are
# compared with the exact inverse in mpmath as well as with the oracle.
UPPER_TAIL_CELLS = [(2718, 10, 3), (35333, 24, 48)]


@pytest.mark.parametrize("it,i,j", UPPER_TAIL_CELLS)
def test_upper_tail_as241_cell(monkeypatch, it, i, j):
    hM, m, st = _build("probit")
    E = O.linear_predictor(st, m)
    s = 1.0 if m["Y"][i, j] == 1 else -1.0
    alpha = -s * E[i, j]
    _, u = D.tails_uniforms(SEED, it)
    u = u[i, j]
    assert u > 1 - 2.8e-8 and alpha < -6.0, (u, alpha)
    assert D.branch_name(alpha, u).endswith("as241-tail")
    Zo = O.update_z(st, m, Rng(SEED), it)
    ch = _chain(monkeypatch, hM, st, 1)
    ch.update("Z", it)
    Z = ch.get_state()["Z"]
    ch.close()
    x_dev, x_orc = s * (Z[i, j] - E[i, j]), s * (Zo[i, j] - E[i, j])
    x_ref = D.tn_exact_one(alpha, u, x_orc)
    err = float(abs(x_dev - x_ref)) / max(1.0, abs(float(x_ref)))
    err_orc = float(abs(x_orc - x_ref)) / max(1.0, abs(float(x_ref)))
    bound = TOL_X + 2 * np.spacing(abs(E[i, j])) / max(1.0, abs(float(x_ref)))
    print(f"upper tail it={it} cell ({i}, {j}): alpha={alpha!r} u={u!r} x={x_dev!r} exact={float(x_ref)!r} "
          f"device err {err:.3e} oracle err {err_orc:.3e} (bound {bound:.3e})")
    assert err_orc <= 1e-13
    assert err <= bound
    allerr = np.abs(Z - Zo) / np.maximum(1.0, np.abs(Zo - E))
    assert allerr.max() <= TOL_X + 2 * np.spacing(np.abs(E)).max()
