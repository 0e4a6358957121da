"""hmsc_predict_community (hmsc_amd/csrc/community.hip) against the numpy restatement
(tests/community_reference.py) applied to hmsc_predict's own output for the same block and seed.

Values.  With u = 2^-53, t_j the terms of a column's numerator and g_j those of the denominator, in
longdouble from hmsc_predict's output: a plain column within (ns + 4) u sum |t_j|, a normalised one
within 1.01 [(ns + 4) u (sum |t_j| + |C| sum |g_j|) / |den| + u |C|]: ns roundings for the products
and the adds of a sum taken in any order, and 4 for the device's exp at the 1.54-spacing budget
tests/test_gpu_predict_cells.py holds it to; the quotient's bound is the first-order propagation of
both sums' errors plus its own rounding, 1 % for the second-order terms.  A reference value that is
NaN or infinite (exp of a large count overflows fp64 to inf, inf / inf is NaN) must be met exactly,
and so must a finite numerator over an infinite denominator (0, where the bound's own formula is
inf / inf).
Each case prints its worst ratio to the bound and how many values are bit-equal to the restatement
in the device's documented order; the count is not asserted.

Statistics.  n, every quantile and Pr equal numpy's on the device's own comm exactly; the mean stays
within summary_reference.mean_bound, the bound of a sequential fp64 sum.

Measured on an MI355X: the worst error / bound over all cases here was 0.491; every value of every
identity-transform case was bit-equal to the ordered restatement (112 cases), at least 0.87 of the
values of an exp case (the device's exp and numpy's round differently); every mean was bit-equal to
the sequential restatement.
"""
import functools

import numpy as np
import pytest

import community_reference as CR
import predict_reference as PR
import summary_reference as SR
from helpers import H, synthetic_model
from test_gpu_predict_summary import LEVELS, _inputs

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)
NY = 70


def _weights(ns, nw, seed=0):
    """nw = 1: the ones column (S).  Otherwise: the ones column plain; random columns with zero and
    negative weights and alternating normalise flags; a ones column normalised (identically 1
    where the denominator is finite and not 0); the last column a unit vector on species 1 mod ns."""
    rng = np.random.default_rng([seed, ns, nw])
    W = np.zeros((ns, nw))
    norm = np.zeros(nw, dtype=np.int32)
    W[:, 0] = 1.0
    for m in range(1, nw):
        w = rng.standard_normal(ns)
        w[rng.random(ns) < 0.3] = 0.0
        W[:, m] = w
        norm[m] = m % 2
    if nw >= 3:
        W[:, nw - 1] = 0.0
        W[1 % ns, nw - 1] = 1.0
        norm[nw - 1] = 0
    if nw >= 16:
        W[:, 2] = 1.0
        norm[2] = 1
    return W, norm


def _stack(inp, expected, seed):
    out, rc = PR.predict_inputs(inp, expected, seed)
    assert rc == 0, PR.last_error()
    return out                                                  # S x ny x ns


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _assert_values(comm, A, W, norm, transform, what):
    """The value test on comm (S x ny x nw) against the stack A (S x ny x ns)."""
    ns = A.shape[2]
    ref = CR.community_wide(A, W, norm, transform)
    bound = CR.value_bound(ref, norm, ns)
    Cw = ref["C"]
    fin = np.isfinite(Cw)
    assert np.array_equal(np.isnan(comm), np.isnan(Cw)), f"{what}: NaN pattern differs"
    inf = np.isinf(Cw)
    assert np.array_equal(comm[inf], Cw[inf].astype(np.float64)), f"{what}: infinite values differ"
    limit = fin & ~np.isfinite(bound)        # a finite sum over an infinite denominator: exactly 0
    assert np.array_equal(comm[limit], Cw[limit].astype(np.float64)), f"{what}: values at an infinite denominator differ"
    fin = fin & ~limit
    err = np.abs(comm[fin].astype(np.longdouble) - Cw[fin])
    b = bound[fin]
    ratio = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1)).astype(np.float64)
    ratio = np.where((b == 0) & (err > 0), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    ordered = CR.community_ordered(A, W, norm, transform)
    equal = int(np.sum((comm == ordered) | (np.isnan(comm) & np.isnan(ordered))))
    print(f"{what}: worst error / bound = {worst:.3f}; {equal} of {comm.size} values bit-equal to the ordered restatement")
    if worst > 1.0:
        k = tuple(int(v[int(np.argmax(ratio))]) for v in np.nonzero(fin))
        raise AssertionError(f"{what}: error / bound = {worst} at (s, i, m) = {k}: device {comm[k]!r}, reference "
                             f"{Cw[k]!r}, bound {bound[k]!r}, num {ref['num'][k]!r}, den {ref['den'][k[:2]]!r}, "
                             f"row {A[k[0], k[1]]!r}, weights {W[:, k[2]]!r}, normalise {norm[k[2]]}")
    return worst, equal


def _assert_statistics(got, probs, pairs, what):
    """n, quantiles and Pr of the device's own comm exactly; the mean within the sequential bound."""
    comm = got["comm"]
    ref = CR.statistics(comm, probs, pairs)
    assert np.array_equal(got["n"], ref["n"]), what
    if len(probs):
        bad = ~((got["quantiles"] == ref["quantiles"]) | (np.isnan(got["quantiles"]) & np.isnan(ref["quantiles"])))
        k = np.unravel_index(int(np.argmax(bad)), bad.shape)
        assert not bad.any(), (f"{what}: {int(bad.sum())} quantiles differ, first at (q, i, m) = {k}: device "
                               f"{got['quantiles'][k]!r}, reference {ref['quantiles'][k]!r}")
    assert _same(got["Pr"], ref["Pr"]), (what, got["Pr"], ref["Pr"])
    A = np.ascontiguousarray(comm.transpose(1, 2, 0))           # ny x nw x S
    wide = SR.longdouble_mean(A)
    fin = np.isfinite(wide) & (ref["n"] > 0)
    assert np.all(np.isnan(got["mean"][ref["n"] == 0]))
    assert _same(got["mean"][~fin], wide[~fin].astype(np.float64)), what
    with np.errstate(invalid="ignore"):
        err = np.abs(got["mean"].astype(np.longdouble) - wide)[fin].astype(np.float64)
        bound = SR.mean_bound(A)[fin]
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    equal = int(np.sum(got["mean"][fin] == ref["mean"][fin]))
    print(f"{what}: {equal} of {int(fin.sum())} means bit-equal to the sequential restatement")


@functools.lru_cache(maxsize=None)
def _case(levels, ns, nw, transform, expected, S):
    """One device call per case, shared by the value and the statistics test; never modified."""
    inp = _inputs(NY, ns, 3, LEVELS[levels], S, seed=21)
    seed = 4000 + 7 * S + ns
    A = _stack(inp, expected, seed)
    W, norm = _weights(ns, nw)
    pairs = ((0, NY - 1), (NY - 1, 3), (65, 2))
    got, rc = CR.call_community(inp, expected, seed, W, norm, transform, PROBS, pairs)
    assert rc == 0, PR.last_error()
    return A, W, norm, pairs, got


CASES = dict(argnames="levels,ns,nw,transform,expected,S",
             argvalues=[(lv, ns, nw, tr, ex, S) for lv in LEVELS for ns in (3, 37) for nw in (1, 3, 16) for tr in (0, 1)
                        for ex in (1, 0) for S in (1, 2, 65)])


@pytest.mark.parametrize(**CASES)
def test_values(levels, ns, nw, transform, expected, S):
    """70 sites (two ragged site tiles); ns = 3 leaves one of a site's four species lanes empty,
    ns = 37 gives two ragged species tiles; nc = 3, zero to two levels, the four families with
    YScalePar; nw 1, 3, 16 with mixed normalise flags, zero and negative weights."""
    A, W, norm, pairs, got = _case(levels, ns, nw, transform, expected, S)
    _assert_values(got["comm"], A, W, norm, transform, f"{levels} ns={ns} nw={nw} g={transform} expected={expected} S={S}")
    if nw >= 3 and not transform:      # the unit-vector column is that species' prediction itself
        assert _same(got["comm"][:, :, nw - 1], A[:, :, 1 % ns] + 0.0)


@pytest.mark.parametrize(**CASES)
def test_statistics(levels, ns, nw, transform, expected, S):
    A, W, norm, pairs, got = _case(levels, ns, nw, transform, expected, S)
    _assert_statistics(got, PROBS, pairs, f"{levels} ns={ns} nw={nw} g={transform} expected={expected} S={S}")


def test_large_k():
    """K = 128 (nc = 8, four levels of nf 30) at 65 x 33 with nw = 16, S = 3: the launch at the LDS
    limit (the two tiles' 98,816 B and the 4 KB of W rows)."""
    inp = _inputs(65, 33, 8, ((30, 65), (30, 22), (30, 65), (30, 9)), 3, seed=12, scale=0.25)
    assert inp["K"] == 128
    W, norm = _weights(33, 16)
    pairs = ((0, 64),)
    for expected in (1, 0):
        for transform in (0, 1):
            A = _stack(inp, expected, 5)
            got, rc = CR.call_community(inp, expected, 5, W, norm, transform, PROBS, pairs)
            assert rc == 0, PR.last_error()
            _assert_values(got["comm"], A, W, norm, transform, f"K128 expected={expected} g={transform}")
            _assert_statistics(got, PROBS, pairs, f"K128 expected={expected} g={transform}")


def _bits(x):
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


def test_slabs_and_repeats():
    """One site tile per slab (scratch_bytes = one tile's need: three slabs at ny = 150) with pairs
    that straddle the slabs, against the default single slab, and a repeated call: every output
    bit-equal.  One byte less than a tile's need is refused, naming the bytes.  Then the same without
    a random level (nr = 0: the slabs walk a Pi of no columns)."""
    for what, levels in (("slabs nr2", ((2, 150), (3, 12))), ("slabs nr0", ())):
        print(f"{what}: begins")            # a failure's captured output names the case
        _slabs_and_repeats(levels, what)


def _slabs_and_repeats(levels, what):
    S, ny, ns, nw = 9, 150, 37, 3
    inp = _inputs(ny, ns, 3, levels, S, seed=14)
    W, norm = _weights(ns, nw)
    pairs = ((10, 140), (70, 3), (64, 63))
    need = S * 64 * nw * 8
    base, rc = CR.call_community(inp, 0, 31, W, norm, 0, PROBS, pairs)
    assert rc == 0, PR.last_error()
    _assert_values(base["comm"], _stack(inp, 0, 31), W, norm, 0, what)
    _assert_statistics(base, PROBS, pairs, what)
    for scratch in (need, 2 * need + 8, 0):
        again, rc = CR.call_community(inp, 0, 31, W, norm, 0, PROBS, pairs, scratch_bytes=scratch)
        assert rc == 0, PR.last_error()
        for key in ("n", "mean", "quantiles", "Pr", "comm"):
            assert np.array_equal(_bits(np.ascontiguousarray(base[key])), _bits(np.ascontiguousarray(again[key]))), \
                (what, key, scratch)
    nocomm, rc = CR.call_community(inp, 0, 31, W, norm, 0, PROBS, pairs, scratch_bytes=need, want_comm=False)
    assert rc == 0 and nocomm["comm"] is None, PR.last_error()
    for key in ("n", "mean", "quantiles", "Pr"):
        assert np.array_equal(_bits(np.ascontiguousarray(base[key])), _bits(np.ascontiguousarray(nocomm[key]))), key
    before = PR.live_resources()
    none, rc = CR.call_community(inp, 0, 31, W, norm, 0, PROBS, pairs, scratch_bytes=need - 1)
    assert rc != 0 and none is None and str(need) in PR.last_error() and "scratch" in PR.last_error(), PR.last_error()
    assert PR.live_resources() == before


def test_nan_draw():
    """A NaN Poisson draw in one sample (a rate past exp(709.78), expected = 0) on species 0 of row 0:
    that sample's summed columns are NaN there (n = S - 1, as rowSums gives NA in R); a unit-vector
    column on species 2 is untouched, because a zero weight is a select."""
    S, ny, ns = 6, 66, 4
    inp = _inputs(ny, ns, 1, (), S, seed=13)
    inp["family"][:] = 3
    inp["sigma"][:] = 0.0
    inp["YScalePar"][0], inp["YScalePar"][1] = 0.0, 1.0
    inp["X"][:, 0] = np.linspace(0.5, 3.0, ny)
    inp["X"][0, 0] = 1.0
    inp["Beta"][:, 0, :] = 1.0
    inp["Beta"][4, 0, 0] = 800.0
    A = _stack(inp, 0, 21)
    assert np.isnan(A[4, 0, 0]) and np.isnan(A).sum() == np.isnan(A[4, :, 0]).sum() and not np.isnan(A[:, :, 1:]).any()
    nanrows = np.isnan(A[4, :, 0])
    W = np.column_stack([np.ones(ns), np.arange(1.0, ns + 1), np.eye(ns)[2]])
    norm = np.array([0, 1, 0], dtype=np.int32)
    got, rc = CR.call_community(inp, 0, 21, W, norm, 0, PROBS, ((0, ny - 1),))
    assert rc == 0, PR.last_error()
    _assert_values(got["comm"], A, W, norm, 0, "NaN draw")
    _assert_statistics(got, PROBS, ((0, ny - 1),), "NaN draw")
    assert np.all(got["n"][nanrows, :2] == S - 1) and np.all(got["n"][~nanrows, :2] == S) and np.all(got["n"][:, 2] == S)
    assert _same(got["comm"][:, :, 2], A[:, :, 2] + 0.0)
    assert np.all(np.isnan(got["Pr"][0, :2])) and np.isfinite(got["Pr"][0, 2])


def test_refusals_and_resources():
    """Every refusal by its message; no device resource is held after a good or a refused call."""
    inp = _inputs(5, 3, 2, (), 2, seed=15)
    W, norm = _weights(3, 3)
    before = PR.live_resources()
    good, rc = CR.call_community(inp, 1, 1, W, norm, 0, PROBS, ((0, 4),))
    assert rc == 0, PR.last_error()
    assert PR.live_resources() == before
    t = CR.community_timing()
    assert len(t) == 3 and all(x >= 0.0 for x in t) and t[1] > 0.0
    cases = ((dict(nw=0), "nw must lie in 1 .. 16"), (dict(nw=17), "nw must lie in 1 .. 16"),
             (dict(probs=np.linspace(0, 1, 9)), "at most 8 probabilities"), (dict(probs=(0.5, 1.25)), "[0, 1]"),
             (dict(probs=(-0.5,)), "[0, 1]"), (dict(pairs=((0, 5),)), "pair index 5"),
             (dict(pairs=((-1, 2),)), "pair index -1"), (dict(raw_pairs=np.zeros(18, np.int32)), "at most 8 site pairs"),
             (dict(scratch_bytes=2 * 64 * 3 * 8 - 1), "scratch"), (dict(null=("p",)), "NULL"), (dict(null=("c",)), "NULL"),
             (dict(null=("n",)), "NULL"), (dict(null=("mean",)), "NULL"), (dict(null=("W",)), "NULL"))
    for kw, match in cases:
        args = dict(probs=PROBS, pairs=())
        args.update(kw)
        got, rc = CR.call_community(inp, 1, 1, W, norm, 0, **args)
        assert rc != 0 and got is None and match in PR.last_error(), (kw, PR.last_error())
    got, rc = CR.call_community(dict(inp, nsamples=0), 1, 1, W, norm)
    assert rc != 0 and "nsamples" in PR.last_error(), PR.last_error()
    big = _inputs(5, 3, 129, (), 1, seed=15)
    got, rc = CR.call_community(big, 1, 1, W, norm)
    assert rc != 0 and "<= 128" in PR.last_error(), PR.last_error()
    assert PR.live_resources() == before


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def _with_xdata(hM0):
    """helpers.synthetic_model's data as a model defined with XData (constructGradient needs one)."""
    import pandas as pd
    X = np.asarray(hM0.X)
    XData = pd.DataFrame({f"x{k}": X[:, k] for k in range(1, X.shape[1])})
    rl = {name: hM0.ranLevels[name] for name in hM0.rLNames}
    return H.Hmsc(Y=hM0.Y, XData=XData, XFormula="~" + "+".join(XData.columns), Tr=hM0.Tr, distr=hM0.distr,
                  studyDesign=hM0.studyDesign, ranLevels=rl, YScale=True)


def _fit(hM):
    return H.sampleMcmc(hM, samples=5, transient=10, thin=1, nChains=2, updater={"GammaEta": False}, seed=5, verbose=0)


@pytest.fixture(scope="module")
def fitted():
    return _fit(_with_xdata(synthetic_model(ny=60, ns=9, nc=3, nf=2, nr=2, units=[60, 12], n_normal=2, n_poisson=3,
                                            seed=71, nt=3)))


@pytest.fixture(scope="module")
def fitted_normal():
    return _fit(_with_xdata(synthetic_model(ny=60, ns=6, nc=3, nf=2, nr=1, units=[15], n_normal=6, seed=72, nt=3)))


@pytest.fixture(scope="module")
def fitted_spatial():
    return _fit(_with_xdata(synthetic_model(ny=40, ns=7, nc=3, nf=2, nr=1, n_normal=2, n_poisson=2, seed=73, nt=2,
                                            spatial={0}, alpha_n=8)))


def _assert_gradient(hM, G, seed, what, **kw):
    """gradientSummary on the device against its host restatement on predict's list for the same
    seed: "Y" exactly (a unit-vector column is the cell itself); "S" and "T" within the sum of the
    two paths' value bounds at the worst sample of a grid point (an order statistic, and the
    interpolation between two, moves by no more than the values do); Pr within the share of
    samples whose two values are closer than their bounds."""
    predY = H.predict(hM, Gradient=G, seed=seed, expected=False, **kw)
    A = np.stack(predY, axis=0)                                  # S x ngrid x ns
    ngrid = A.shape[1]
    all_normal = bool(np.all(hM.distr[:, 0] == 1))
    Tr = np.asarray(hM.Tr, dtype=np.float64)
    for measure, index in (("S", 0), ("Y", 2), ("T", 1), ("T", hM.nt - 1)):
        host = H.gradientSummary(hM, G, measure, index=index, predY=predY)
        dev = H.gradientSummary(hM, G, measure, index=index, seed=seed, expected=False, **kw)
        Pr_ref, q_ref = CR.plot_gradient(predY, measure, index, PROBS, Tr, all_normal)
        assert host["ylabel"] == dev["ylabel"] and np.array_equal(host["xx"], dev["xx"])
        assert _same(host["Pr"], Pr_ref) and _same(np.stack([host["lo"], host["me"], host["hi"]]), q_ref), (what, measure)
        if measure == "Y":
            tol, amb = np.zeros(ngrid), 0
        else:
            W = np.ones((hM.ns, 1)) if measure == "S" else Tr[:, [index]]
            norm, tr = [int(measure == "T")], int(measure == "T" and all_normal)
            ref = CR.community_wide(A, W, norm, tr)
            b = CR.value_bound(ref, norm, hM.ns)[:, :, 0].astype(np.float64)
            tol = 2.0 * b.max(axis=0)
            c = ref["C"][:, :, 0].astype(np.float64)
            amb = int(np.sum(np.abs(c[:, ngrid - 1] - c[:, 0]) <= 2.0 * (b[:, ngrid - 1] + b[:, 0])))
        for key in ("lo", "me", "hi"):
            err = np.abs(dev[key] - host[key])
            print(f"{what} {measure}[{index}] {key}: worst error {float(err.max()):.3e}, tolerance {float(tol.min()):.3e}")
            assert np.all(err <= tol), (what, measure, key, float(np.max(err - tol)))
        assert abs(dev["Pr"] - host["Pr"]) <= amb / A.shape[0] + 1e-15, (what, measure, dev["Pr"], host["Pr"])


def test_end_to_end_gradient(fitted):
    """constructGradient -> predict(Gradient=) -> plotGradient's numbers, device against host, on a
    mixed-family model with traits and two levels."""
    G = H.constructGradient(fitted, "x1", ngrid=7)
    _assert_gradient(fitted, G, 3, "gradient")
    G = H.constructGradient(fitted, "x2", {"x1": (1,)}, ngrid=5)
    _assert_gradient(fitted, G, 4, "gradient x2")


def test_end_to_end_gradient_all_normal(fitted_normal):
    """An all-normal model: "T" takes exp of the predictions (plotGradient's rule), "S" does not."""
    G = H.constructGradient(fitted_normal, "x1", ngrid=6)
    _assert_gradient(fitted_normal, G, 8, "all normal")
    res = H.predictCommunity(fitted_normal, Gradient=G, seed=8, returnSamples=True)
    assert res["columns"] == ["S"] + list(fitted_normal.trNames) and res["samples"].shape == (10, 6, 1 + fitted_normal.nt)
    A = np.stack(H.predict(fitted_normal, Gradient=G, seed=8), axis=0)
    W = np.column_stack([np.ones(fitted_normal.ns), fitted_normal.Tr])
    _assert_values(res["samples"][:, :, :1], A, W[:, :1], [0], 0, "predictCommunity S")
    _assert_values(res["samples"][:, :, 1:], A, W[:, 1:], [1] * fitted_normal.nt, 1, "predictCommunity T")


def test_end_to_end_prepare_gradient_spatial(fitted_spatial):
    """A prepareGradient grid on a spatial level, its new units kriged on the device."""
    import pandas as pd
    hM = fitted_spatial
    rng = np.random.default_rng(5)
    n = 9
    XDataNew = pd.DataFrame({"x1": np.linspace(-1, 1, n), "x2": rng.standard_normal(n)})
    G = H.prepareGradient(hM, XDataNew, {hM.rLNames[0]: rng.random((n, 2))})
    _assert_gradient(hM, G, 6, "prepareGradient", krigeDevice=True)


def test_too_many_columns(fitted):
    with pytest.raises(ValueError, match="17"):
        H.predictCommunity(fitted, measures=("S",), weights=np.ones((fitted.ns, 16)))
