"""predict's kernel (hmsc_amd/csrc/predict.hip) against an extended-precision reference of the same
operation, cell by cell (tests/predict_reference.py): every species tile, every K up to 128, the
tails of pnorm and exp, the draws of every family, and the edges of the C ABI's contract.

Each case fills hmsc_predict_args from arrays (no model, no chain: one small launch).  Every
assertion is per cell; a failure names the worst cell with its (s, i, j), its tile and K.  Bounds
are derived, not tuned:

  L           |out - L_ref| <= 1.01 K 2^-53 A, A = sum_k |a_k| |b_k|: the forward error gamma_K of a
              K-term fma chain (a dropped or misplaced term is 1e13 times larger)
  pnorm       relative 2e-13 + (L^2 + 2) 2^-53: erfc_fast's bound (test_gpu_draw_functions'
              test_erfc) and the L^2 delta by which a relative rounding delta of -L / sqrt 2 moves
              erfc; below the normal range one subnormal spacing on top
  exp         relative |L + sigma/2| 2^-53 for the rounded sum, plus the device exp's own error:
              EXP_ULP_BOUND spacings of the result (see there)
  normal draw sqrt(sigma) 1e-12 max(1, |q|) (test_qnorm's bound) + the bound of L + 2^-52 |out|
  indicator   1[z_ref > 0] wherever |z_ref| exceeds the normal draw's bound
  counts      <= 1e-3 of a column's cells differ from the oracle's sampler on the same uniforms
              (the cap of test_gpu_predict.py), and the device's own counts pass the chi-square
              test the oracle's pass (tests/test_host_predict_reference.py)
"""
import numpy as np
import pytest

import predict_reference as PR
from predict_reference import U

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (63, 31), (64, 32), (65, 33), (130, 65)]
# nc, nf per level.  (64 (K | 1) + 32 K) 8 bytes of LDS: 65,280 at K = 85, the largest within 64 KB
LAYOUTS = {"K1": (1, ()), "K7": (3, (2, 2)), "K30": (20, (10,)), "K9_8levels": (1, (1,) * 8), "K85": (60, (25,)),
           "K86": (60, (26,)), "K127": (64, (32, 31)), "K128": (64, (32, 31, 1))}

# The device exp's own error.  The installed ROCm documentation states no bound for the double
# exp, so it is measured: the worst on test_exp_tails' grid, on the sigma = 0 columns (where
# L + sigma/2 is exact), is EXP_ULP_MEASURED spacings of the true value; the tests assert at twice
# that, and never looser than 4.
EXP_ULP_MEASURED = 0.771
EXP_ULP_BOUND = min(4.0, 2.0 * EXP_ULP_MEASURED)


def _check(name, err, bound, K, describe=lambda k: ""):
    """err <= bound in every cell of (S, ny, ns) arrays; prints the worst ratio, and on failure
    names the worst cell."""
    err, bound = np.asarray(err), np.asarray(bound)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio).astype(np.float64)
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    s, i, j = (int(v) for v in k[-3:])
    msg = (f"{name}: worst |err| / bound = {ratio[k]:.3g} (err {float(err[k]):.3e}, bound {float(bound[k]):.3e}) at "
           f"(s, i, j) = ({s}, {i}, {j}), {PR.tile_of(i, j)}, K = {K} {describe(k)}")
    print(msg)
    assert ratio[k] <= 1.0, msg
    return float(ratio[k])


def _run(inp, expected, seed=0):
    out, rc = PR.predict_inputs(inp, expected, seed)
    assert rc == 0, f"hmsc_predict returned {rc}: {PR.last_error()} (K = {inp['K']})"
    return out


# ---------------------------------------------------------------------------------------------
# a. the linear predictor at tile and K edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_linear_predictor(shape, layout):
    """Family 1, expected, YScalePar (0, 1): out is L itself.  One site and one species, one short
    of a tile, a full tile, one over, and two tiles and a bit on both axes; K from 1 to 128 with 0 to
    8 levels, either side of the 64 KB of LDS; every level once with np < ny and once with np = ny."""
    (ny, ns), (nc, nfs) = shape, LAYOUTS[layout]
    for mode in ("lt", "eq") if nfs else ("lt",):
        inp = PR.build_inputs(ny, ns, nc, nfs, seed=1, np_mode=mode)
        out = _run(inp, 1)
        Lr, A = PR.linear_predictor(inp)
        with np.errstate(invalid="ignore"):
            err = np.where(np.isfinite(out), np.abs(out.astype(np.longdouble) - Lr).astype(np.float64), np.inf)
        _check(f"L {ny}x{ns} {layout} np {mode}", err, PR.l_bound(inp, A), inp["K"])


# ---------------------------------------------------------------------------------------------
# b, c. pnorm and exp on exact L
# ---------------------------------------------------------------------------------------------
GRID_NY, GRID_NS = 130, 33


def _exact_l_grid(x, family, sigma):
    """x (any length) through the kernel with nc = 1, nr = 0, Beta = 1, so L = x exactly: launches
    of 130 sites x 33 species x 3 samples, every species column and sample repeating the site's x,
    so both tile axes take part.  Returns (x padded to the launches, out: launches x 3 x 130 x 33)."""
    nl = -(-len(x) // GRID_NY)
    xp = np.concatenate([x, np.full(nl * GRID_NY - len(x), x[-1])])
    outs = []
    for b in range(nl):
        inp = PR.build_inputs(GRID_NY, GRID_NS, 1, family=family, sigma=sigma)
        inp["X"] = xp[b * GRID_NY:(b + 1) * GRID_NY].reshape(-1, 1)
        inp["Beta"][:] = 1.0
        outs.append(_run(inp, 1))
    return xp.reshape(nl, GRID_NY), np.stack(outs)


def test_pnorm_tails():
    """pnorm(L) on [-38.5, 9] in 2000 steps with +-0, +-1e-300, -37.5 (the last normal results),
    8.2, 8.3 and 40: relative to mpmath per cell, exactly 1 from 8.3 upward, inside [0, 1]."""
    x = np.concatenate([np.linspace(-38.5, 9.0, 2000), [0.0, -0.0, 1e-300, -1e-300, -37.5, 8.2, 8.3, 40.0]])
    xs, out = _exact_l_grid(x, 2, 1.0)
    ref = PR.mp_map(PR.mp_pnorm, xs)[:, None, :, None]
    refw = PR.mp_to_wide(ref)
    err = PR.abs_err(out, refw)
    rel = (2e-13 + (xs * xs + 2.0) * U)[:, None, :, None]
    sub = refw < np.longdouble(2.0) ** -1022
    assert sub.sum() > 10 and (~sub).sum() > 1900
    bound = rel * refw + np.where(sub, np.longdouble(2.0) ** -1074, 0)
    _check("pnorm", err, np.broadcast_to(bound, err.shape), 1,
           lambda k: f"L = {xs[k[0], k[2]]!r} out = {out[k]!r} launch {k[0]}")
    assert np.all((out >= 0.0) & (out <= 1.0))
    one = np.broadcast_to((xs >= 8.3)[:, None, :, None], out.shape)
    assert one.sum() >= 3 * GRID_NS * 30 and np.all(out[one] == 1.0)


def test_exp_tails():
    """exp(L + sigma/2) on [-745, 709] in 2000 steps with 709.7 (the last finite results), 710,
    -746 and +-0, sigma = 0, 1e-3, 1, 2.5 by species: relative to mpmath per cell; overflow is inf
    on both sides; below the normal range the bound holds with one subnormal spacing on top.
    Measured on an MI355X: the device exp alone (sigma = 0, where the sum is exact) is within 0.771
    spacings of the true value, worst at L = 629.717...; asserted at twice that (EXP_ULP_BOUND)."""
    import mpmath as mp
    x = np.concatenate([np.linspace(-745.0, 709.0, 2000), [709.7, 710.0, -746.0, 0.0, -0.0]])
    sg = np.array([0.0, 1e-3, 1.0, 2.5])[np.arange(GRID_NS) % 4]
    xs, out = _exact_l_grid(x, 3, sg)
    with mp.workdps(PR.D.DPS):
        arg = np.array([[mp.mpf(float(v)) + mp.mpf(float(s)) / 2 for s in sg[:4]] for v in xs.ravel()], dtype=object)
        ref4 = PR.mp_map(mp.exp, arg)
        over4 = np.array([r >= mp.mpf(2) ** 1024 * (1 - mp.mpf(2) ** -54) for r in ref4.ravel()]).reshape(ref4.shape)
    nl = xs.shape[0]
    col = np.arange(GRID_NS) % 4
    ref = PR.mp_to_wide(ref4).reshape(nl, GRID_NY, 4)[:, :, col][:, None]   # launches x 1 x 130 x 33
    over = np.broadcast_to(over4.reshape(nl, GRID_NY, 4)[:, :, col][:, None], out.shape)
    absarg = np.abs(PR.mp_to_double(arg)).reshape(nl, GRID_NY, 4)[:, :, col][:, None]
    assert over.any() and np.all(np.isposinf(out[over])), "overflow must be inf"
    assert np.all(np.isfinite(out[~over])), "inf where the true value is finite"
    refw = np.broadcast_to(ref, out.shape)
    with np.errstate(over="ignore"):
        refd = np.where(over, np.inf, refw.astype(np.float64))
    fin = ~over
    err = PR.abs_err(np.where(fin, out, 0.0), ref)
    with np.errstate(invalid="ignore"):
        spacing = np.spacing(np.where(fin, np.abs(refd), 1.0)).astype(np.longdouble)
    ulps = np.where(fin, err / spacing, 0).astype(np.float64)
    exact = fin & np.broadcast_to((sg == 0.0)[None, None, None, :], out.shape) & (refd >= 2.0 ** -1022)
    k = np.unravel_index(int(np.argmax(np.where(exact, ulps, 0.0))), ulps.shape)
    print(f"device exp alone (sigma = 0, normal results): worst {ulps[k]:.3f} spacings at L = {xs[k[0], k[2]]!r}")
    bound = np.broadcast_to(absarg, out.shape) * U * refw + np.maximum(EXP_ULP_BOUND, 1.0) * spacing
    _check("exp", np.where(fin, err, 0), np.where(fin, bound, 1), 1,
           lambda k: f"L = {xs[k[0], k[2]]!r} sigma = {sg[k[3]]!r} out = {out[k]!r} launch {k[0]}")
    assert np.max(np.where(exact, ulps, 0.0)) <= EXP_ULP_BOUND


# ---------------------------------------------------------------------------------------------
# d, e. normal and probit draws
# ---------------------------------------------------------------------------------------------
def _draw_case(ny, ns, family):
    sg = np.random.default_rng([ny, ns]).uniform(0.1, 4.0, (3, ns))      # per sample and species
    return PR.build_inputs(ny, ns, 3, (2, 2), seed=2, np_mode=("lt", "eq"), family=family, sigma=sg)


def _z_bound(inp, ref, zabs):
    """The bound of a normal draw z = fma(sqrt(sigma), q, L): qnorm's 1e-12 max(1, |q|) scaled, the
    bound of L, and two roundings (sqrt and the fma) of |z|."""
    sq = np.sqrt(inp["sigma"])[:, None, :]
    return sq * 1e-12 * np.maximum(1.0, np.abs(ref["q"])) + PR.l_bound(inp, ref["A"]) + 2.0 * U * zabs


@pytest.mark.parametrize("shape", [(65, 33), (130, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_normal_draws(shape):
    """out = L + sqrt(sigma) q with q the AS241 normal of the cell's first uniform: pins
    cell = i + ny j and the sample counter in every tile.  Under a second key out changes, and
    matches its own reference again."""
    inp = _draw_case(*shape, 1)
    outs = []
    for seed in (977, 2 ** 40 + 5):
        out = _run(inp, 0, seed)
        ref = PR.reference(inp, False, seed)
        with np.errstate(invalid="ignore"):
            err = np.where(np.isfinite(out), np.abs(out.astype(np.longdouble) - ref["z"]).astype(np.float64), np.inf)
        _check(f"normal draw {shape} seed {seed}", err, _z_bound(inp, ref, np.abs(out)), inp["K"],
               lambda k: f"q = {ref['q'][k]!r}")
        outs.append(out)
    assert np.mean(outs[0] != outs[1]) > 0.999


@pytest.mark.parametrize("shape", [(65, 33), (130, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_probit_draws(shape):
    """out = 1[z_ref > 0] in every cell whose |z_ref| exceeds the normal draw's bound; at most one
    cell may lie inside it (about 25,000 cells with a bound near 1e-11: 1e-7 expected)."""
    inp = _draw_case(*shape, 2)
    out = _run(inp, 0, 977)
    ref = PR.reference(inp, False, 977)
    zabs = np.abs(ref["z"]).astype(np.float64)
    decided = zabs > _z_bound(inp, ref, zabs)
    assert (~decided).sum() <= 1
    bad = decided & (out != (ref["z"] > 0))
    k = np.unravel_index(int(np.argmax(bad)), bad.shape)
    assert not bad.any(), (f"{int(bad.sum())} indicators differ, first at (s, i, j) = {k}, {PR.tile_of(k[1], k[2])}, "
                           f"K = {inp['K']}: out {out[k]!r}, z_ref {float(ref['z'][k])!r}")
    assert np.all((out == 0.0) | (out == 1.0))


# ---------------------------------------------------------------------------------------------
# f. Poisson draws at fixed rates
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_counts():
    return PR.oracle_poisson_counts()


def test_poisson_draws_at_fixed_rates(oracle_counts):
    """20000 sites, one column per rate (X = 1, Beta_j = log lambda_j, sigma = 0, one sample), on
    both sides of the lam < 10 switch: integer counts, <= 1e-3 of a column differing from the oracle
    on the same uniforms, and the device's own counts Poisson by the chi-square test at p >= 1e-3
    (the oracle's own pass at 0.01; up to 20 cells may differ by a boundary flip).
    Measured on an MI355X: no cell differs up to lambda = 1e9; 19 of 20000 differ at 1e12, where
    lgamma(k + 1) = 2.7e13 is spaced 4e-3 apart and decides PTRS' slow acceptance on both sides; the
    device's p-values lie between 0.17 and 0.999."""
    lam = np.array(PR.POIS_LAMBDAS)
    ns = len(lam)
    inp = PR.build_inputs(PR.POIS_NY, ns, 1, S=1, family=3, sigma=0.0)
    inp["X"][:] = 1.0
    inp["Beta"][0, 0, :] = np.log(lam)
    out = _run(inp, 0, PR.POIS_SEED)[0]
    assert np.all(out >= 0) and np.all(out == np.round(out))
    fails = []
    for j in range(ns):
        diff = float(np.mean(out[:, j] != oracle_counts[:, j]))
        p, stat, nb = PR.poisson_gof_pvalue(out[:, j], PR.poisson_rates()[j])
        print(f"lambda = {lam[j]:g}: {diff:.2e} of the cells differ from the oracle; chi2 = {stat:.1f} on {nb} bins, "
              f"p = {p:.4f}")
        if diff > 1e-3 or p < 1e-3:
            fails.append((lam[j], diff, p))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------
# g. lognormal Poisson, mixed families, YScalePar
# ---------------------------------------------------------------------------------------------
YSCALE_CYCLE = [(0.0, 1.0), (2.5, 1.0), (0.0, 0.3), (-1.2, 3.0)]


@pytest.fixture(scope="module")
def mixed():
    ny, ns = 65, 33
    fam = 1 + np.arange(ns) % 3
    ysp = np.vstack([np.zeros(ns), np.ones(ns)])
    for n, j in enumerate(np.nonzero(fam == 1)[0]):
        ysp[:, j] = YSCALE_CYCLE[n % 4]
    sg = np.random.default_rng(12).uniform(0.1, 2.0, (3, ns))
    return PR.build_inputs(ny, ns, 3, (2, 2), seed=3, np_mode=("lt", "eq"), family=fam, sigma=sg, yscale=ysp)


def test_mixed_families_expected(mixed):
    """Family by column 1, 2, 3, sigma > 0 (lognormal Poisson), YScalePar on the normal columns
    through (0, 1), (2.5, 1), (0, 0.3), (-1.2, 3): the bounds of L, pnorm and exp with the error of L
    carried through (phi(L) dL for pnorm, dL relative for exp), and one fma's 2^-53 |out| where
    the back-transform applies."""
    from scipy.stats import norm
    inp = mixed
    out = _run(inp, 1)
    ref = PR.reference(inp, True, 0)
    fam, lb = inp["family"], PR.l_bound(inp, ref["A"])
    Ld = ref["L"].astype(np.float64)
    m, sd = inp["YScalePar"]
    sel = fam == 1
    with np.errstate(invalid="ignore"):
        err = np.abs(out[:, :, sel].astype(np.longdouble) - (ref["L"][:, :, sel] * sd[sel] + m[sel])).astype(float)
    _check("normal expected", np.where(np.isfinite(out[:, :, sel]), err, np.inf),
           np.abs(sd[sel]) * lb[:, :, sel] + U * np.abs(out[:, :, sel]), inp["K"], lambda k: "(normal columns only)")
    sel = fam == 2
    refw = PR.mp_to_wide(ref["mp"][:, :, sel])
    bound = (2e-13 + (Ld[:, :, sel] ** 2 + 2.0) * U) * refw + 1.01 * norm.pdf(Ld[:, :, sel]) * lb[:, :, sel]
    _check("probit expected", PR.abs_err(out[:, :, sel], ref["mp"][:, :, sel]), bound, inp["K"],
           lambda k: "(probit columns only)")
    sel = fam == 3
    refw = PR.mp_to_wide(ref["mp"][:, :, sel])
    arg = np.abs(Ld[:, :, sel] + inp["sigma"][:, None, sel] / 2)
    bound = (arg * U + 1.01 * lb[:, :, sel]) * refw + EXP_ULP_BOUND * np.spacing(refw.astype(np.float64))
    _check("Poisson expected", PR.abs_err(out[:, :, sel], ref["mp"][:, :, sel]), bound, inp["K"],
           lambda k: "(Poisson columns only)")


def test_mixed_families_draws(mixed):
    """The same model's draws: normal columns to the draw's bound through the back-transform's fma,
    probit columns the indicator of z_ref, Poisson columns the oracle's counts on the reference's
    own exp(z_ref) (<= 1e-3 of a column differing, integer and >= 0)."""
    inp, seed = mixed, 31337
    out = _run(inp, 0, seed)
    ref = PR.reference(inp, False, seed)
    fam = inp["family"]
    m, sd = inp["YScalePar"]
    zabs = np.abs(ref["z"]).astype(np.float64)
    zb = _z_bound(inp, ref, zabs * (1 + 1e-9))
    sel = fam == 1
    with np.errstate(invalid="ignore"):
        err = np.abs(out[:, :, sel].astype(np.longdouble) - (ref["z"][:, :, sel] * sd[sel] + m[sel])).astype(float)
    _check("normal draw, back-transformed", np.where(np.isfinite(out[:, :, sel]), err, np.inf),
           np.abs(sd[sel]) * zb[:, :, sel] + U * np.abs(out[:, :, sel]), inp["K"], lambda k: "(normal columns only)")
    sel = fam == 2
    decided = zabs[:, :, sel] > zb[:, :, sel]
    assert (~decided).sum() <= 1
    assert np.array_equal(out[:, :, sel][decided], (ref["z"][:, :, sel] > 0).astype(float)[decided])
    for j in np.nonzero(fam == 3)[0]:
        assert np.all(out[:, :, j] >= 0) and np.all(out[:, :, j] == np.round(out[:, :, j])), j
        diff = np.mean(out[:, :, j] != ref["out"][:, :, j])
        assert diff <= 1e-3, (f"Poisson column {j} ({PR.tile_of(0, j)}): {diff:.3e} of the cells differ from the "
                              f"oracle, first at (s, i) = {np.argwhere(out[:, :, j] != ref['out'][:, :, j])[0]}")


# ---------------------------------------------------------------------------------------------
# h. edges of the contract
# ---------------------------------------------------------------------------------------------
def _refused(match, **kw):
    """A call that must be refused with `match` in the message, holding no resource afterwards."""
    before = PR.live_resources()
    a = dict(ny=1, ns=1, nc=1, nr=0, nsamples=1, expected=1, seed=1, X=[0.0], Beta=[0.0], sigma=[1.0], family=[1],
             yscale=[0.0, 1.0], Pi=None, nps=[], nfs=[], Eta=[], Lambda=[], out=np.full(1, 7.25))
    a.update(kw)
    rc = PR.call_raw(**a)
    assert rc != 0 and match in PR.last_error(), (rc, PR.last_error())
    assert PR.live_resources() == before
    assert np.all(a["out"] == 7.25)


def test_poisson_draw_of_a_non_finite_rate():
    """L = 800 (exp overflows) and L = NaN on a Poisson column give NaN, as R's rpois gives;
    L = -800 (exp underflows to 0) gives 0."""
    inp = PR.build_inputs(3, 1, 1, S=1, family=3, sigma=0.0)
    inp["X"][:, 0] = [800.0, np.nan, -800.0]
    inp["Beta"][:] = 1.0
    out = _run(inp, 0, 5)[0, :, 0]
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 0.0, out


def test_refusals_hold_nothing():
    """K = 129, a Pi entry of 0 or np + 1, and ny ns >= 2^32 (checked before any array is read:
    the arrays here are 1-element dummies) are refused by name, leave out untouched and leave
    hmsc_debug_live_resources as it was."""
    _refused("<= 128", nc=129)
    _refused("<= 128", nc=1, nr=8, nps=[1] * 8, nfs=[16] * 8, Eta=[[0.0]] * 8, Lambda=[[0.0]] * 8, Pi=[1] * 8)
    _refused("32-bit cell counters", ny=65536, ns=65536)
    for bad in (0, 4):
        _refused("Pi out of range", ny=3, nr=1, X=[0.0] * 3, Pi=[1, bad, 3], nps=[3], nfs=[1], Eta=[[0.0] * 3],
                 Lambda=[[0.0]], out=np.full(3, 7.25))


def test_no_samples_is_a_no_op():
    before = PR.live_resources()
    out = np.full(4, 7.25)
    rc = PR.call_raw(ny=2, ns=2, nc=1, nr=0, nsamples=0, expected=1, seed=1, X=[0.0, 0.0], Beta=[0.0], sigma=[1.0],
                     family=[1, 1], yscale=[0.0, 1.0, 0.0, 1.0], Pi=None, nps=[], nfs=[], Eta=[], Lambda=[], out=out)
    assert rc == 0, PR.last_error()
    assert np.all(out == 7.25) and PR.live_resources() == before
