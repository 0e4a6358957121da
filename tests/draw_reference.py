"""mpmath references (50 digits) of the scalar functions behind updateZ's draws, and the grids
the draw tests evaluate them on (tests/test_oracle_rng.py, tests/test_gpu_draw_functions.py,
tests/test_gpu_z_tails.py).  Test infrastructure only.

The truncated-normal reference is the exact inverse: the x with Phic(x) = u Phic(alpha), found
by Newton on log Phic from a double-precision starting value.  Beyond alpha > 25 the oracle and
the device both *define* the draw by the tail expansion alpha - ln(u) / alpha (an approximation
of the distribution, not of the inversion), so there the reference is that formula in mpmath.
"""
import functools
import os

import mpmath as mp
import numpy as np

DPS = 50
SQRT2 = np.sqrt(2.0)
TAIL_ALPHA = 25.0          # rng.h trunc_normal_lower: alpha > 25 takes the expansion
# the z kernel's tables (z_tables.h): erfcx on segments of width 1/4 in a = min(|alpha| / sqrt 2,
# 17.99) over [0, 18), F(w) on segments of width 1/4 in w = -log(4 p (1 - p)) over [0, 16)
E_PER_UNIT, E_SEG, E_CLAMP = 4, 72, 17.99
Q_PER_UNIT, Q_SEG, Q_MAX = 4, 64, 16.0


def _phic(x):
    return mp.erfc(x / mp.sqrt(2)) / 2


@functools.lru_cache(maxsize=None)
def _log_phic_of(alpha):
    """log Phic(alpha) for a double alpha (0 at -inf), once per distinct value."""
    return mp.mpf(0) if alpha == -np.inf else mp.log(_phic(mp.mpf(alpha)))


# Newton's step s leaves an error of about s^2 |x| / 2: a step below 1e-12 ends the iteration
# 1e-23 from the root
_STEP_END = mp.mpf(10) ** -12


def tn_exact_one(alpha, u, x0):
    """x with Phic(x) = u Phic(alpha) (alpha = -inf: Phic(x) = u), by Newton on log Phic from x0."""
    with mp.workdps(DPS):
        lt = mp.log(mp.mpf(u)) + _log_phic_of(float(alpha))
        x = mp.mpf(x0)
        for _ in range(60):
            pc = _phic(x)
            step = (mp.log(pc) - lt) * pc / mp.npdf(x)   # h / |h'|, h' = -phi / Phic
            x += step
            if abs(step) < _STEP_END:
                return x
        raise RuntimeError(f"Newton did not converge at alpha={alpha!r} u={u!r}")


def tn_tail_one(alpha, u):
    """The draw's definition beyond alpha > 25: alpha - ln(u) / alpha."""
    with mp.workdps(DPS):
        a = mp.mpf(alpha)
        return a - mp.log(mp.mpf(u)) / a


def tn_reference(alpha, u, x0):
    """Reference of trunc_normal_lower over arrays (mpf objects): the exact inverse for
    alpha <= 25, the tail formula beyond.  x0: double-precision starting values."""
    alpha, u, x0 = np.broadcast_arrays(np.asarray(alpha, float), np.asarray(u, float), np.asarray(x0, float))
    out = np.empty(alpha.shape, dtype=object)
    flat = out.reshape(-1)
    for k, (a, uu, s) in enumerate(zip(alpha.ravel(), u.ravel(), x0.ravel())):
        flat[k] = tn_tail_one(a, uu) if a > TAIL_ALPHA else tn_exact_one(a, uu, s)
    return out


def err_vs(x, ref, floor=1.0):
    """|x - ref| / max(floor, |ref|) per element, the difference taken in mpmath."""
    x = np.asarray(x, float)
    e = np.empty(x.shape)
    ef, rf = e.reshape(-1), np.asarray(ref, dtype=object).reshape(-1)
    with mp.workdps(DPS):
        for k, v in enumerate(x.ravel()):
            r = rf[k]
            ef[k] = float(abs(mp.mpf(float(v)) - r) / max(mp.mpf(floor), abs(r))) if np.isfinite(v) else np.inf
    return e


def qnorm_reference(p):
    """Phi^-1(p), p a double array: Newton from scipy's ndtri on the tail nearer to p."""
    from scipy.special import ndtri
    p = np.asarray(p, float)
    out = np.empty(p.shape, dtype=object)
    flat = out.reshape(-1)
    with mp.workdps(DPS):
        for k, (pp, s) in enumerate(zip(p.ravel(), ndtri(p).ravel())):
            pm = mp.mpf(float(pp))
            if pp <= 0.5:   # Phi(x) = p  <=>  Phic(-x) = p
                flat[k] = -_newton_phic(pm, -s)
            else:           # Phic(x) = 1 - p, exactly in mpmath
                flat[k] = _newton_phic(1 - pm, s)
    return out


def _newton_phic(t, x0):
    lt = mp.log(t)
    x = mp.mpf(float(x0))
    for _ in range(60):
        pc = _phic(x)
        step = (mp.log(pc) - lt) * pc / mp.npdf(x)
        x += step
        if abs(step) < _STEP_END:
            return x
    raise RuntimeError("Newton did not converge")


def pg_reference(b, c):
    """Polya-Gamma PG(b, c) mean b tanh(c/2) / (2c) and variance b (sinh c - c) sech^2(c/2) /
    (4 c^3) (Polson, Scott & Windle 2013), with their limits b/4 and b/24 at c = 0."""
    b, c = np.broadcast_arrays(np.asarray(b, float), np.asarray(c, float))
    m = np.empty(b.shape, dtype=object)
    v = np.empty(b.shape, dtype=object)
    with mp.workdps(120):    # sinh c - c cancels to c^3 / 6 at c = 1e-5; cosh(750)^2 ~ 1e651
        for k, (bb, cc) in enumerate(zip(b.ravel(), c.ravel())):
            B, x = mp.mpf(float(bb)), abs(mp.mpf(float(cc)))
            if x == 0:
                m.reshape(-1)[k], v.reshape(-1)[k] = B / 4, B / 24
            else:
                m.reshape(-1)[k] = B * mp.tanh(x / 2) / (2 * x)
                v.reshape(-1)[k] = B * (mp.sinh(x) - x) / mp.cosh(x / 2) ** 2 / (4 * x ** 3)
    return m, v


# ---------------------------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------------------------
def u_of_word(w):
    """(w + 1/2) 2^-32 (rng.h u32o), exact in double."""
    return (np.asarray(w, dtype=np.float64) + 0.5) * (1.0 / 4294967296.0)


def u_grid():
    """The uniforms of the draw grid: the extreme and middle 32-bit words, and 16 log-spaced
    words between (so u runs over 2^-33 .. 1 - 2^-33 with every decade of the lower tail)."""
    edge = [0, 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    logw = np.unique(np.round(np.logspace(np.log10(3.0), np.log10(2.0 ** 32 - 3), 16)).astype(np.int64))
    assert len(logw) == 16
    return u_of_word(np.array(edge + list(logw), dtype=np.float64))


def alpha_grid():
    """[-30, 30] in steps of 1/64; every erfcx segment edge alpha = +-sqrt2 k / 4 with its two
    neighbouring doubles; +-0, the hand-over at 25 and its next double, the clamp's +-25.44,
    -40 and -inf."""
    base = np.arange(-30 * 64, 30 * 64 + 1) / 64.0
    edges = SQRT2 * np.arange(1, E_SEG + 1) / E_PER_UNIT
    edges = np.concatenate([np.nextafter(edges, -np.inf), edges, np.nextafter(edges, np.inf)])
    special = [0.0, -0.0, 25.0, np.nextafter(25.0, np.inf), 25.44, -25.44, -40.0, -np.inf]
    return np.concatenate([base, edges, -edges, special])


def erfcx_segment(alpha):
    a = np.minimum(np.abs(alpha) / SQRT2, E_CLAMP)
    return np.minimum((a * E_PER_UNIT).astype(np.int64), E_SEG - 1)


def quantile_w(p):
    with np.errstate(divide="ignore"):
        return -np.log(4.0 * p * (1.0 - p))


def quantile_segment(w):
    """Segment of F(w), or -1 for AS241's tail (w >= 16)."""
    return np.where(w >= Q_MAX, -1, np.clip((w * Q_PER_UNIT).astype(np.int64), 0, Q_SEG - 1))


def branch_name(alpha, u):
    """The branch of the table draw a cell takes, from double-precision p and w."""
    from scipy.special import erfc
    if alpha > TAIL_ALPHA:
        return "expansion(alpha>25)"
    p = u * 0.5 * erfc(alpha / SQRT2)
    w = float(quantile_w(np.float64(p)))
    q = "as241-tail" if w >= Q_MAX else f"F-seg{int(quantile_segment(np.float64(w)))}"
    return f"erfcx-seg{int(erfcx_segment(np.float64(alpha)))}{'(clamped)' if abs(alpha) / SQRT2 >= E_CLAMP else ''}/{q}"


GRID_REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_grid_ref.npy")


def draw_grid_cells():
    """(alpha, u) of the draw tests: alpha_grid() x u_grid(), flattened alpha-major."""
    a, u = np.meshgrid(alpha_grid(), u_grid(), indexing="ij")
    return a.ravel(), u.ravel()


def draw_grid_reference():
    """The reference of every cell of draw_grid_cells(), rounded to double.  ~90,000 Newton
    solves at 50 digits take over a minute, so they are recorded (tests/golden/draw_grid_ref.npy,
    written by scripts/make_draw_grid_ref.py from tn_reference) and tests/test_oracle_rng.py
    re-derives a spread sample of the record with mpmath on every run."""
    ref = np.load(GRID_REF)
    assert ref.shape == (len(alpha_grid()) * len(u_grid()),), "draw_grid_ref.npy does not match the grid"
    return ref


def as_double(ref):
    return np.array([float(r) for r in np.asarray(ref, dtype=object).ravel()]).reshape(np.shape(ref))


# ---------------------------------------------------------------------------------------------
# the tails model of tests/test_gpu_z_tails.py: E = b0_j + b1_j x_i reaches +-30 standard
# deviations, so a single updateZ visits every table segment, the hand-over at alpha = 25, the
# clamp and AS241's tail
# ---------------------------------------------------------------------------------------------
TAILS_NY, TAILS_NS = 256, 64
TAILS_SEED, TAILS_IT = 20240607, 7
LOG_R = float(np.log(1000.0))
# zPrev - log r of the Poisson cells: the three branches of pg_moments (x < 1e-4, x < 1, the
# rest) with the doubles either side of each threshold
PG_ABS_C = np.array([0.0, 1e-5, np.nextafter(1e-4, 0.0), 1e-4, np.nextafter(1e-4, 1.0), 0.5, np.nextafter(1.0, 0.0),
                     1.0, np.nextafter(1.0, 2.0), 5.0, 30.0, 800.0, 1500.0])


def tails_design():
    """(x, b0, A, Y): the raw covariate (ny), the species offsets and amplitudes (ns) and the
    fixed 0/1 pattern Y (ny x ns).  With xs the scaled covariate, b1_j = A_j / max|xs| and
    E[i, j] = b0_j + b1_j xs_i spans +-8 (even species) or +-30 (odd species: a pair of the z
    kernel holds one of each, so a deep cell takes a shallow partner onto the scalar path)."""
    ny, ns = TAILS_NY, TAILS_NS
    x = np.linspace(-1.0, 1.0, ny)
    j = np.arange(ns)
    b0 = (j - (ns - 1) / 2.0) / ns * 0.5
    A = np.where(j % 2 == 0, 8.0, 30.0)
    Y = (np.random.default_rng(5).random((ny, ns)) < 0.5).astype(float)
    return x, b0, A, Y


def tails_linear_predictor(xs=None):
    x, b0, A, _ = tails_design()
    if xs is None:
        xs = (x - x.mean()) / x.std(ddof=1)
    b1 = A / np.max(np.abs(xs))
    return b0[None, :] + xs[:, None] * b1[None, :], b1


def tails_uniforms(seed=TAILS_SEED, it=TAILS_IT, ny=TAILS_NY, ns=TAILS_NS):
    """The 32-bit words and uniforms updateZ gives the cells (oracle.hmsc_oracle.update_z)."""
    from oracle import rng as R
    j = np.arange(ns)
    idx = (np.arange(ny)[:, None] + ny * (j[None, :] >> 2)).astype(np.uint64)
    w4 = R.Rng(seed).words(idx, 0, R.S_Z, it)
    w = np.choose(np.broadcast_to((j & 3)[None, :], idx.shape), w4)
    return w, R.u32o(w)
