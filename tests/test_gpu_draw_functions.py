"""The scalar functions behind every draw of the sweep, on the device, against mpmath.

hmsc_debug_eval runs one function elementwise on arrays built here, so each branch, table row
and segment edge is visited on purpose instead of by whatever cells a fitted model happens to
hold, and the error is measured per element: |dx| / max(1, |x_ref|) for the draws and the
quantile, relative error for erfc, exp and the Polya-Gamma moments, ulps for the logarithm.
Bounds are the documented fit budgets (rng.h, z_tables.h), not what the code happens to give.

Bound, and the maximum measured on an MI355X (profiles/draw_functions_measure.txt):

    trunc_normal        1e-12    1.3e-13   rng.h trunc_normal_lower (Poisson chains, tails)
    trunc_normal_tab    1e-12    8.4e-14   the z kernel's table draw, z_probit_pair_tab
    trunc_normal_poly   1e-12    1.3e-13   the polynomial pair draw, z_probit_pair
    qnorm               1e-12    1.0e-13   qnorm_fast
    erfc                2e-13    1.5e-13   erfc_fast, relative
    log                 4 ulp    0.70 ulp  log_fast, of max(1, |log x|)
    exp_small           1e-14    8.6e-15   relative, where the result is normal
    pg_moments          1e-13    1.0e-16 (mean), 1.1e-15 (variance), relative

Finding: before the draws formed the complement 1 - p on its own (rng.h trunc_normal_lower_t)
the oracle, whose formula all three draws shared, missed the bound on 984 cells of the grid, all
with alpha in (-9, -4) and u >= 1 - 3 2^-33, by up to 1.1e-8.

The draw grid's 89,901 references are recorded (tests/golden/draw_grid_ref.npy, see
draw_reference.draw_grid_reference); the other references are computed here.
"""
import ctypes

import mpmath as mp
import numpy as np
import pytest

import draw_reference as D
from helpers import H  # noqa: F401  (puts the repository root on sys.path)
from hmsc_amd import _lib as L

pytestmark = pytest.mark.gpu

CHUNK = 20000   # elements per hook call
SQRT2 = np.sqrt(2.0)


def device_eval(what, in0, in1=None, two_out=False):
    in0 = L.f64(in0)
    in1 = None if in1 is None else L.f64(in1)
    out0 = np.full(in0.shape, np.nan)
    out1 = np.full(in0.shape, np.nan) if two_out else None
    for s in range(0, in0.size, CHUNK):
        e = min(in0.size, s + CHUNK)
        a, b = in0[s:e], None if in1 is None else in1[s:e]
        o0, o1 = out0[s:e], None if out1 is None else out1[s:e]
        L.check(L.lib().hmsc_debug_eval(0, what.encode(), e - s, L.fptr(a), L.fptr(b), L.fptr(o0), L.fptr(o1)))
    return (out0, out1) if two_out else out0


def _live():
    out = (ctypes.c_int64 * 4)()
    L.check(L.lib().hmsc_debug_live_resources(out))
    return list(out)


def _report(name, err, bound, describe):
    k = int(np.argmax(err))
    print(f"{name}: max {err[k]:.3e} (bound {bound:g}) at {describe(k)}")
    return err[k]


def _draw_err(x, ref):
    with np.errstate(invalid="ignore"):
        e = np.abs(x - ref) / np.maximum(1.0, np.abs(ref))
    return np.where(np.isfinite(x), e, np.inf)


@pytest.fixture(scope="module")
def grid():
    a, u = D.draw_grid_cells()
    return a, u, D.draw_grid_reference()


def _pair_layout(a, u, ref):
    """The pair draws take elements 2k, 2k + 1 as one pair.  The grid in order (so neighbouring
    cells share a pair, and a cell just past alpha = 25 sits beside one just short of it), then
    every alpha > 25 cell once with a partner at alpha = 0.3 and once at alpha = -7: the partner
    is drawn by the scalar path because of its neighbour, and is compared too."""
    from oracle.rng import trunc_normal_lower
    tail = np.nonzero(a > D.TAIL_ALPHA)[0]
    aa, uu, rr = [a], [u], [ref]
    if len(a) % 2:   # keep the appended pairs aligned
        aa.append(a[:1]), uu.append(u[:1]), rr.append(ref[:1])
    ug = D.u_grid()
    for partner in (0.3, -7.0):
        pref = D.as_double(D.tn_reference(np.full(len(ug), partner), ug, trunc_normal_lower(partner, ug)))
        pu = np.arange(len(tail)) % len(ug)   # the partner's own uniform cycles through the grid's
        for order in (0, 1):                  # the deep cell as the pair's first and as its second cell
            pa = np.empty(2 * len(tail)), np.empty(2 * len(tail)), np.empty(2 * len(tail))
            pa[0][order::2], pa[1][order::2], pa[2][order::2] = a[tail], u[tail], ref[tail]
            pa[0][1 - order::2], pa[1][1 - order::2], pa[2][1 - order::2] = partner, ug[pu], pref[pu]
            aa.append(pa[0]), uu.append(pa[1]), rr.append(pa[2])
    return np.concatenate(aa), np.concatenate(uu), np.concatenate(rr)


@pytest.mark.parametrize("what", ["trunc_normal", "trunc_normal_tab", "trunc_normal_poly"])
def test_truncated_normal_draws(grid, what):
    """Both implementations of the probit draw (and the callerless polynomial pair draw, kept
    for the microbenchmarks) on alpha in [-30, 30] by 1/64, every erfcx segment edge +- 1 ulp,
    the hand-over at 25, the clamp at 17.99 sqrt 2 = 25.44 and NA cells, crossed with the extreme
    32-bit uniforms and 16 log-spaced ones.  1e-12 = ten times the 1e-13 fit budget of rng.h
    and z_tables.h."""
    a, u, ref = grid if what == "trunc_normal" else _pair_layout(*grid)
    before = _live()
    x = device_eval(what, a, u)
    assert _live() == before
    err = _draw_err(x, ref)
    worst = _report(what, err, 1e-12, lambda k: f"alpha={a[k]!r} u={u[k]!r} x={x[k]!r} ref={ref[k]!r} "
                                                f"branch={D.branch_name(a[k], u[k])}")
    assert worst <= 1e-12


def _mp_err(x, ref, floor=None):
    """|x - ref| / max(floor, |ref|) (floor None: relative), the difference taken in mpmath."""
    out = np.empty(len(x))
    with mp.workdps(D.DPS):
        for k, (v, r) in enumerate(zip(x, ref)):
            if not np.isfinite(v):
                out[k] = np.inf
                continue
            den = abs(r) if floor is None else max(mp.mpf(floor), abs(r))
            out[k] = float(abs(mp.mpf(float(v)) - r) / den)
    return out


def _p_at_w(w):
    """The lower-tail p with -log(4 p (1 - p)) = w."""
    with mp.workdps(D.DPS):
        return float((1 - mp.sqrt(1 - mp.exp(-mp.mpf(w)))) / 2)


def test_qnorm():
    """qnorm_fast on p log-spaced from 1e-300 to 1/2 and mirrored as 1 - p down to 2^-53, and
    around the p where w = -log(4 p (1 - p)) crosses the branch points 6.25 and 16 (the p of each
    crossing with its four neighbouring doubles, on both tails)."""
    lo = np.concatenate([np.logspace(-300, -16, 700), np.logspace(-16, np.log10(0.5), 500), [0.5]])
    up = 1.0 - np.concatenate([2.0 ** -np.arange(53, 1, -1.0), np.logspace(-15.9, np.log10(0.5), 300)])
    edge = []
    for w in (6.25, 16.0):
        p = _p_at_w(w)
        for k in range(-2, 3):
            q = p
            for _ in range(abs(k)):
                q = np.nextafter(q, np.inf if k > 0 else -np.inf)
            edge += [q, 1.0 - q]
    p = np.concatenate([lo, up, edge])
    assert p.min() > 0 and p.max() < 1
    x = device_eval("qnorm", p)
    err = _mp_err(x, D.qnorm_reference(p), floor=1.0)
    assert _report("qnorm", err, 1e-12, lambda k: f"p={p[k]!r} q={x[k]!r} w={D.quantile_w(p[k])!r}") <= 1e-12


def _below_normal_ok(y, ref, sub, rel):
    """Where the true value is subnormal a double cannot hold it to a relative bound: there the
    result must lie within the same relative bound plus one subnormal spacing, 2^-1074."""
    with mp.workdps(D.DPS):
        return all(abs(mp.mpf(float(v)) - r) <= rel * r + mp.mpf(2) ** -1074
                   for v, r in zip(y[sub], np.array(ref, dtype=object)[sub]))


def test_erfc():
    """erfc_fast on [-6, 27], relative: 1.3e-13 fit + 5e-14 from rounding -z^2 + g near 18.
    (erfc z is a subnormal double beyond z = 26.54: see _below_normal_ok.)"""
    z = np.concatenate([np.linspace(-6.0, 27.0, 2113), [0.0, -0.0, 18.0, np.nextafter(18.0, 0), 26.5]])
    y = device_eval("erfc", z)
    with mp.workdps(D.DPS):
        ref = [mp.erfc(mp.mpf(float(v))) for v in z]
    normal = np.array([r >= mp.mpf(2) ** -1022 for r in ref])
    assert z[normal].max() > 26.5 and (~normal).sum() > 10
    err = _mp_err(y, ref)
    worst = _report("erfc", err[normal], 2e-13, lambda k: f"z={z[normal][k]!r} erfc={y[normal][k]!r}")
    assert worst <= 2e-13
    assert _below_normal_ok(y, ref, ~normal, 2e-13), "erfc_fast below the normal range"


def test_log():
    """log_fast on every binade from 1e-300 to 1e300, mantissas just below and above sqrt 2
    (where the reduction switches exponent), at 1 -+ ulp, and at the ends and middle of [1, 2):
    absolute error within 4 ulp of max(1, |log x|)."""
    s2 = 1.4142135623730951
    mant = np.array([1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), np.nextafter(s2, 1.0), s2,
                     np.nextafter(s2, 2.0), 1.25, 1.75])
    ex = np.arange(-996, 997)   # 2^-996 = 1.5e-300 .. 2^996 = 6.7e299
    x = (mant[None, :] * 2.0 ** ex[:, None]).ravel()
    x = np.concatenate([x, [np.nextafter(1.0, 0.0), 1e-300, 1e300]])
    y = device_eval("log", x)
    with mp.workdps(D.DPS):
        ref = [mp.log(mp.mpf(float(v))) for v in x]
        err = np.array([float(abs(mp.mpf(float(v)) - r)) if np.isfinite(v) else np.inf for v, r in zip(y, ref)])
    ulp = np.spacing(np.maximum(1.0, np.abs(np.array([float(r) for r in ref]))))
    e = err / ulp
    assert _report("log", e, 4, lambda k: f"x={x[k]!r} log={y[k]!r} (ulps)") <= 4.0


def test_exp_small():
    """exp_small on [-745, 0]: relative error within 1e-14 (6e-15 truncation of the degree-11
    Taylor polynomial) wherever the result is a normal double (below: _below_normal_ok)."""
    x = np.concatenate([np.linspace(-745.0, 0.0, 2981), -np.logspace(-300, 0, 200), [-0.0, -0.34657359027997264,
                        -708.3964185322641, -708.5]])
    y = device_eval("exp_small", x)
    with mp.workdps(D.DPS):
        ref = [mp.exp(mp.mpf(float(v))) for v in x]
    normal = np.array([r >= mp.mpf(2) ** -1022 for r in ref])
    err = _mp_err(y, ref)
    assert _report("exp_small", err[normal], 1e-14,
                   lambda k: f"x={x[normal][k]!r} exp={y[normal][k]!r}") <= 1e-14
    assert (~normal).sum() > 50
    assert _below_normal_ok(y, ref, ~normal, 1e-14), "exp_small below the normal range"


def pg_cases():
    """b = y + 1000 for counts 0, 3, 4000; |c| over the three branches of pg_moments (x < 1e-4,
    x < 1, the rest) with the doubles either side of each threshold, and large |c| (cosh^2
    overflows a double beyond 710: sech^2 must go to zero, not to NaN)."""
    ulp = lambda v, s: np.nextafter(v, v + s)  # noqa: E731
    cabs = np.array([0.0, 1e-5, ulp(1e-4, -1), 1e-4, ulp(1e-4, 1), 0.5, ulp(1.0, -1), 1.0, ulp(1.0, 1), 5.0, 30.0,
                     800.0, 1500.0])
    c = np.concatenate([cabs, -cabs])
    b, c = np.meshgrid([1000.0, 1003.0, 5000.0], c, indexing="ij")
    return b.ravel(), c.ravel()


def test_pg_moments():
    b, c = pg_cases()
    m, v = device_eval("pg_moments", b, c, two_out=True)
    rm, rv = D.pg_reference(b, c)
    em, ev = _mp_err(m, rm.ravel()), _mp_err(v, rv.ravel())
    wm = _report("pg_moments mean", em, 1e-13, lambda k: f"b={b[k]!r} c={c[k]!r} mean={m[k]!r}")
    wv = _report("pg_moments var", ev, 1e-13, lambda k: f"b={b[k]!r} c={c[k]!r} var={v[k]!r}")
    assert wm <= 1e-13 and wv <= 1e-13


def test_unknown_function_is_an_error():
    x = np.ones(4)
    rc = L.lib().hmsc_debug_eval(0, b"no_such_function", 4, L.fptr(x), None, L.fptr(x.copy()), None)
    assert rc != 0 and b"unknown function" in L.lib().hmsc_last_error()
    rc = L.lib().hmsc_debug_eval(0, b"trunc_normal", 4, L.fptr(x), None, L.fptr(x.copy()), None)
    assert rc != 0
