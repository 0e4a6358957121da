"""The shared randomness contract (oracle/rng.py == hmsc_amd/csrc/rng.h) on CPU."""
import numpy as np
import pytest
from scipy import stats
from scipy.special import ndtri

from oracle.rng import Rng, philox4x32_10, qnorm_as241, trunc_normal_lower


@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, expect):
    """Random123 philox4x32_10 KAT vectors."""
    out = philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in out) == expect


def test_qnorm_as241_accuracy():
    p = np.concatenate([np.logspace(-300, -1, 3000), np.linspace(1e-3, 1 - 1e-3, 5000), 1 - np.logspace(-15, -1, 500)])
    a, b = qnorm_as241(p), ndtri(p)
    assert np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)) < 5e-15


def test_uniforms_open_interval_and_independence():
    r = Rng(42)
    a, b = r.uniforms(np.arange(200000), 0, 12, 3)
    assert a.min() > 0 and a.max() < 1 and b.min() > 0 and b.max() < 1
    assert stats.kstest(a, "uniform").pvalue > 1e-3
    assert abs(np.corrcoef(a, b)[0, 1]) < 0.01
    c, _ = r.uniforms(np.arange(200000), 0, 12, 4)   # next sweep: a different stream
    assert abs(np.corrcoef(a, c)[0, 1]) < 0.01


def test_normal_distribution():
    x = Rng(7).normal(np.arange(200000), 0, 22, 5)
    assert stats.kstest(x, "norm").pvalue > 1e-3


@pytest.mark.parametrize("shape", [0.3, 1.0, 2.5, 50.0, 5000.0])
def test_gamma_distribution(shape):
    g = Rng(9).gamma_std(np.arange(100000), 20, 1, shape)
    assert stats.kstest(g, "gamma", args=(shape,)).pvalue > 1e-3


@pytest.mark.parametrize("alpha", [-6.0, -1.0, 0.0, 0.7, 3.0, 9.0, 30.0])
def test_truncated_normal(alpha):
    u = Rng(11).uniforms(np.arange(100000), 0, 12, 2)[0]
    x = trunc_normal_lower(np.full(u.shape, alpha), u)
    assert np.all(x >= alpha)
    if alpha <= 9:
        d = stats.truncnorm(alpha, np.inf)
        assert stats.kstest(x, d.cdf).pvalue > 1e-3
    else:
        # deep tail: (x - alpha) * alpha ~ Exp(1) to O(1/alpha^2)
        assert abs(np.mean((x - alpha) * alpha) - 1.0) < 0.02


# ---------------------------------------------------------------------------------------------
# The oracle's draw is the reference of the GPU draw tests: hold it to mpmath at 50 digits first.
# ---------------------------------------------------------------------------------------------
def _tn_err(alpha, u):
    import draw_reference as D
    x = trunc_normal_lower(alpha, u)
    ref = D.tn_reference(alpha, u, x)
    refd = D.as_double(ref)
    return D.err_vs(x, ref), D.err_vs(x - alpha, np.array([r - float(a) for r, a in zip(ref, alpha)], dtype=object),
                                      floor=1e-300), x, refd


def test_trunc_normal_lower_against_mpmath():
    """x = trunc_normal_lower(alpha, u) against the exact root of Phic(x) = u Phic(alpha) (Newton
    at 50 digits from the oracle's value) on 600 cells of the tails model (test_gpu_z_tails.py:
    alpha = -+E over +-30, alpha <= 25, NA cells as alpha = -inf, u = (w + 1/2) 2^-32 from the
    model's own Philox words), with w = 0 and w = 2^32 - 1 forced into every tenth cell.

    Asserted: |dx| / max(1, |x|) <= 1e-13.  Measured 5.6e-16, and 1.3e-3 relative to the
    excess x - alpha: that is reached at a forced w = 2^32 - 1 cell in the deep tail, where the
    excess, 2^-33 / alpha, is below 1e-11 and a rounding of x is 1e-3 of it (4.6e-12
    over the cells that keep the model's own words); the draw is only as good as x itself there.  Before the complement 1 - p was formed on its own (oracle/rng.py)
    the cells with u within 3 2^-33 of 1 and alpha in (-9, -4) were off by up to 1.1e-8
    (test_draw_grid_record_and_oracle_on_it holds all of them)."""
    import draw_reference as D
    E, _ = D.tails_linear_predictor()
    _, _, _, Y = D.tails_design()
    w, _ = D.tails_uniforms()
    alpha = np.where(Y == 1, -E, E).ravel()
    w = w.ravel().astype(np.float64)
    keep = np.nonzero(alpha <= 25.0)[0]
    pick = keep[np.linspace(0, len(keep) - 1, 600).astype(int)]
    a, ww = alpha[pick].copy(), w[pick].copy()
    ww[0::20] = 0.0
    ww[10::20] = 2.0 ** 32 - 1.0
    a[5::20] = -np.inf
    e1, e2, x, _ = _tn_err(a, D.u_of_word(ww))
    k = int(np.argmax(e1))
    print("trunc_normal_lower vs mpmath: max |dx|/max(1,|x|)", e1.max(), "at alpha, u =", a[k], D.u_of_word(ww)[k],
          "; relative to the excess", e2[np.isfinite(a)].max())
    assert a.min() < -25 and a[np.isfinite(a)].max() > 24 and np.sum(ww == 2.0 ** 32 - 1.0) == 30
    assert e1.max() <= 1e-13


def test_draw_grid_record_and_oracle_on_it():
    """tests/golden/draw_grid_ref.npy (the reference of test_gpu_draw_functions.py's draws) is
    what mpmath gives: every 173rd cell and every cell of the ill-conditioned corner (alpha in
    [-9, -5], u >= 1 - 3 2^-33, sampled) is solved again here and must equal the record to
    double rounding.  The oracle is then held to the whole record at 1e-13 (measured 7.3e-16)."""
    import draw_reference as D
    a, u = D.draw_grid_cells()
    ref = D.draw_grid_reference()
    corner = np.nonzero((a >= -9) & (a <= -5) & (u > 1 - 2.0 ** -31))[0][::7]
    pick = np.unique(np.concatenate([np.arange(0, len(a), 173), corner]))
    again = D.as_double(D.tn_reference(a[pick], u[pick], ref[pick]))
    np.testing.assert_allclose(ref[pick], again, rtol=2.3e-16, atol=0)
    x = trunc_normal_lower(a, u)
    err = np.abs(x - ref) / np.maximum(1.0, np.abs(ref))
    k = int(np.argmax(err))
    print("oracle on the draw grid: max", err[k], "at alpha, u =", a[k], u[k], D.branch_name(a[k], u[k]))
    assert err[k] <= 1e-13


def test_trunc_normal_deep_tail_expansion():
    """alpha > 25: the oracle and the device define the draw as alpha - ln(u) / alpha.  The
    oracle equals that formula in mpmath to 1e-15 relative (measured 7.0e-17).

    The formula is the first term of the exact inverse.  With L = -ln u and x = alpha + d,
    log Phic(x) = -x^2 / 2 - log x - log sqrt(2 pi) - 1 / x^2 + ..., so Phic(x) = u Phic(alpha)
    reads  alpha d + d^2 / 2 + log(1 + d / alpha) + O(d / alpha^3) = L,  whence
        d = L / alpha - (L^2 / 2 + L) / alpha^3 + O(L^3 / alpha^5):
    the expansion overshoots the exact draw by the next term T = (L^2 / 2 + L) / alpha^3.  At
    alpha = 25+: u = 1/2 gives a gap of 5.94e-5 (T = 5.97e-5), u = 2^-33 a gap of 1.75e-2
    (T = 1.82e-2): small against the conditional sd 1 / alpha = 0.04 only for moderate L, which is
    why this is an approximation of the distribution.  Asserted: 0 < gap < T."""
    import mpmath as mp
    import draw_reference as D
    a = np.concatenate([np.full(21, np.nextafter(25.0, np.inf)), np.linspace(25.5, 30.0, 10).repeat(21)])
    u = np.tile(D.u_grid(), 11)
    x = trunc_normal_lower(a, u)
    formula = [D.tn_tail_one(aa, uu) for aa, uu in zip(a, u)]
    rel = D.err_vs(x, formula, floor=1e-300)
    print("deep tail: oracle vs formula", rel.max())
    assert rel.max() <= 1e-15
    with mp.workdps(D.DPS):
        for aa, uu, f in zip(a[:21], u[:21], formula[:21]):
            exact = D.tn_exact_one(aa, uu, float(f))
            L = -mp.log(mp.mpf(float(uu)))
            T = (L * L / 2 + L) / mp.mpf(float(aa)) ** 3
            gap = f - exact
            print("alpha = 25+: u", uu, "gap", float(gap), "next term", float(T))
            assert 0 < gap < T


def test_pg_moments_against_closed_forms():
    """oracle pg_moments against the closed forms at 120 digits, at the |c| of the device test
    (both sides of x = 1e-4 and x = 1, up to 1500 where cosh^2 overflows a double), relative
    error of mean and variance.  Bound 1e-14: the series below x = 1 is truncated at x^16 / 19!
    (< 1e-17), the mean's at x^4 / 480 (2e-19 at 1e-4); what is left is the rounding of about ten
    operations and, at x = 1+, the 7-fold cancellation of 2 tanh(x/2) - x sech^2(x/2).
    Measured: mean 1.7e-16, variance 2.5e-15 (at |c| = 1 + ulp)."""
    import draw_reference as D
    from oracle.hmsc_oracle import pg_moments
    c = np.concatenate([D.PG_ABS_C, -D.PG_ABS_C])
    b, c = [v.ravel() for v in np.meshgrid([1000.0, 1003.0, 5000.0], c, indexing="ij")]
    m, v = pg_moments(b, c)
    rm, rv = D.pg_reference(b, c)
    em, ev = D.err_vs(m, rm, floor=1e-300), D.err_vs(v, rv, floor=1e-300)
    print("pg_moments oracle: mean", em.max(), "var", ev.max(), "at c =", c[int(np.argmax(ev))])
    assert em.max() <= 1e-14 and ev.max() <= 1e-14
