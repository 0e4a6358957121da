"""hmsc_predict_summary (hmsc_amd/csrc/summary.hip) against the numpy restatement
(tests/summary_reference.py) applied to hmsc_predict's own output for the same arguments and seed.

The summary kernel forms every value as predict_kernel does (predict_cell.h), so n, the positive
counts and every quantile must equal the reference's exactly: that both kernels compute the same
cell, and that the selection is exact under the heavy ties of 0 / 1 probit draws and at S = 1.  The
mean is a sequential fp64 sum in sample order: it is held to the bound of such a sum,
n 2^-53 (sum |x| / n), against the longdouble mean, and the number of means bit-equal to the
restatement's is printed.

Measured on an MI355X: every mean of every case here was bit-equal to the restatement's (test_cells:
2590 of 2590 in each of its 30 cases; K = 128: 2145 of 2145; the fitted model: 810 of 810); each
case prints its count.
"""
import numpy as np
import pytest

import predict_reference as PR
import summary_reference as SR
from helpers import H, synthetic_model

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)
YSCALE_CYCLE = [(2.5, 1.0), (0.0, 0.3), (-1.2, 3.0)]


def _inputs(ny, ns, nc, levels, S, seed, scale=1.0):
    """Random stacks in predict_reference.build_inputs' layout; levels: (nf, np) pairs.  Families
    cycle normal / probit / Poisson (sigma = 0) / lognormal Poisson, YScalePar on the normal columns."""
    rng = np.random.default_rng([seed, ny, ns, nc, S, len(levels)])
    fam = np.array([1, 2, 3, 3])[np.arange(ns) % 4].astype(np.int32)
    sigma = rng.uniform(0.2, 2.0, (S, ns))
    sigma[:, np.arange(ns) % 4 == 1] = 1.0
    sigma[:, np.arange(ns) % 4 == 2] = 0.0
    ysp = np.vstack([np.zeros(ns), np.ones(ns)])
    for k, j in enumerate(np.nonzero(fam == 1)[0]):
        ysp[:, j] = YSCALE_CYCLE[k % 3]
    nfs, nps = [f for f, _ in levels], [u for _, u in levels]
    inp = dict(X=rng.standard_normal((ny, nc)), Beta=scale * rng.standard_normal((S, nc, ns)), sigma=sigma, family=fam,
               YScalePar=ysp, np=nps, nf=nfs,
               Pi=np.column_stack([PR.random_pi(rng, ny, u) if u < ny else rng.permutation(ny).astype(np.int32) + 1
                                   for u in nps]) if levels else np.zeros((ny, 0), np.int32),
               Eta=[rng.standard_normal((S, u, f)) for f, u in levels],
               Lambda=[scale * rng.standard_normal((S, f, ns)) for f, _ in levels])
    inp["K"] = nc + sum(nfs)
    return inp


def _stack(inp, expected, seed):
    out, rc = PR.predict_inputs(inp, expected, seed)
    assert rc == 0, PR.last_error()
    return np.ascontiguousarray(out.transpose(1, 2, 0))      # ny x ns x S


def _same(a, b):
    """Equal values with the same NaN pattern."""
    return np.array_equal(a, b, equal_nan=True)


def _assert_summary(got, A, probs, qcols=None, what=""):
    """The assertions of every case: n, the positive counts and the quantiles exactly; the mean
    within the sequential sum's bound of the longdouble mean.  Returns the bit-equal mean count."""
    ref = SR.summarise(A, probs, qcols)
    assert np.array_equal(got["n"], ref["n"]), what
    with np.errstate(invalid="ignore"):
        assert _same(got["occ"], ref["occ"]), what
        assert np.array_equal(np.rint(np.nan_to_num(got["occ"] * got["n"])).astype(np.int64), ref["pos"]), what
    if len(probs):
        bad = ~((got["quantiles"] == ref["quantiles"]) | (np.isnan(got["quantiles"]) & np.isnan(ref["quantiles"])))
        k = np.unravel_index(int(np.argmax(bad)), bad.shape)
        assert not bad.any(), (f"{what}: {int(bad.sum())} quantiles differ, first at (q, i, j) = {k}: device "
                               f"{got['quantiles'][k]!r}, reference {ref['quantiles'][k]!r} (lo {ref['lo'][k]!r}, hi "
                               f"{ref['hi'][k]!r}, n {ref['n'][k[1:]]})")
    ok = ref["n"] > 0
    assert np.all(np.isnan(got["mean"][~ok])) and np.all(np.isnan(got["occ"][~ok]))
    err = np.abs(got["mean"].astype(np.longdouble) - SR.longdouble_mean(A))[ok].astype(np.float64)
    bound = SR.mean_bound(A)[ok]
    assert np.all(err <= bound), (what, float(np.max(err - bound)))
    equal = int(np.sum(got["mean"][ok] == ref["mean"][ok]))
    print(f"{what}: {equal} of {int(ok.sum())} means bit-equal to the sequential restatement")
    return equal


LEVELS = {"nr0": (), "nr1": ((2, 70),), "nr2": ((2, 70), (3, 12))}


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65])
@pytest.mark.parametrize("expected", [1, 0], ids=["expected", "draws"])
@pytest.mark.parametrize("levels", list(LEVELS))
def test_cells(levels, expected, S):
    """70 x 37 (two ragged tiles per axis), nc = 3, zero to two levels (np = ny and np = 12), the four
    families with YScalePar on the normal columns, quantiles 0.025 / 0.5 / 0.975 on all columns."""
    inp = _inputs(70, 37, 3, LEVELS[levels], S, seed=11)
    seed = 977 + S
    A = _stack(inp, expected, seed)
    got, rc = SR.call_summary(inp, expected, seed, PROBS)
    assert rc == 0, PR.last_error()
    _assert_summary(got, A, PROBS, what=f"{levels} expected={expected} S={S}")


def test_large_k():
    """K = 128 (nc = 8, four levels of nf 30) at 65 x 33, S = 3: the launch with the two tiles' 98,816 B
    of LDS (and 1 KB for the tile's units)."""
    inp = _inputs(65, 33, 8, ((30, 65), (30, 22), (30, 65), (30, 9)), 3, seed=12, scale=0.25)
    assert inp["K"] == 128
    for expected in (1, 0):
        A = _stack(inp, expected, 5)
        got, rc = SR.call_summary(inp, expected, 5, PROBS)
        assert rc == 0, PR.last_error()
        _assert_summary(got, A, PROBS, what=f"K128 expected={expected}")


def test_nan_cells():
    """A Poisson column (sigma = 0, so z = L) whose rate overflows past L = 709.78 in some samples
    (row 0), in every sample (row 1) and in none: n < S with the statistics of the rest; n = 0 with
    NaN mean, occ and quantiles."""
    S, ny = 7, 66
    inp = _inputs(ny, 2, 1, (), S, seed=13)
    inp["family"][:] = 3
    inp["sigma"][:] = 0.0
    inp["X"][:, 0] = np.linspace(0.5, 3.0, ny)
    inp["X"][0, 0], inp["X"][1, 0] = 1.0, 1000.0
    inp["Beta"][:, 0, :] = 1.0
    inp["Beta"][[1, 4, 5], 0, 0] = 800.0
    A = _stack(inp, 0, 21)
    assert np.isnan(A[0, 0]).sum() == 3 and np.isnan(A[0, 1]).sum() == 0 and np.all(np.isnan(A[1]))
    got, rc = SR.call_summary(inp, 0, 21, PROBS)
    assert rc == 0, PR.last_error()
    _assert_summary(got, A, PROBS, what="NaN cells")
    assert got["n"][0, 0] == S - 3 and got["n"][0, 1] == S and np.all(got["n"][1] == 0)
    assert np.all(np.isnan(got["mean"][1])) and np.all(np.isnan(got["occ"][1])) and np.all(np.isnan(got["quantiles"][:, 1]))
    assert np.all(np.isfinite(got["mean"][0])) and np.all(np.isfinite(got["quantiles"][:, 0]))


def test_slabs_and_repeats():
    """One site tile per slab (scratch_bytes = one tile's need: three slabs at ny = 150) against the
    default single slab, and a repeated call: every output bit-equal.  Quantiles on the flagged
    columns only (NaN elsewhere).  One byte less than a tile's need is refused, naming the bytes.
    Then the same without a random level (nr = 0: the slabs walk a Pi of no columns)."""
    for what, levels in (("slabs nr2", ((2, 150), (3, 12))), ("slabs nr0", ())):
        print(f"{what}: begins")            # a failure's captured output names the case
        _slabs_and_repeats(levels, what)


def _slabs_and_repeats(levels, what):
    S, ny, ns = 9, 150, 37
    inp = _inputs(ny, ns, 3, levels, S, seed=14)
    qcols = inp["family"] == 3
    need = S * 64 * int(qcols.sum()) * 8
    base, rc = SR.call_summary(inp, 0, 31, PROBS, qcols)
    assert rc == 0, PR.last_error()
    _assert_summary(base, _stack(inp, 0, 31), PROBS, qcols, what=what)
    assert np.all(np.isnan(base["quantiles"][:, :, ~qcols])) and not np.any(np.isnan(base["quantiles"][:, :, qcols]))
    for scratch in (need, 2 * need + 8, 0):
        again, rc = SR.call_summary(inp, 0, 31, PROBS, qcols, scratch_bytes=scratch)
        assert rc == 0, PR.last_error()
        for key in ("mean", "occ", "n", "quantiles"):
            assert np.array_equal(base[key].view(np.int64 if base[key].dtype == np.float64 else np.int32),
                                  again[key].view(np.int64 if again[key].dtype == np.float64 else np.int32)), (what, key, scratch)
    before = PR.live_resources()
    none, rc = SR.call_summary(inp, 0, 31, PROBS, qcols, scratch_bytes=need - 1)
    assert rc != 0 and none is None and str(need) in PR.last_error() and "scratch" in PR.last_error(), PR.last_error()
    assert PR.live_resources() == before


def test_refusals():
    """More than 8 probabilities, a probability outside [0, 1] and nsamples = 0: named errors that
    hold no device resource afterwards; predict's own limits are kept (K <= 128)."""
    inp = _inputs(5, 3, 2, (), 2, seed=15)
    before = PR.live_resources()
    for kw, match in ((dict(probs=np.linspace(0, 1, 9)), "at most 8"), (dict(probs=(0.5, 1.25)), "[0, 1]"),
                      (dict(probs=(-0.5,)), "[0, 1]")):
        got, rc = SR.call_summary(inp, 1, 1, **kw)
        assert rc != 0 and match in PR.last_error(), PR.last_error()
    got, rc = SR.call_summary(dict(inp, nsamples=0), 1, 1)
    assert rc != 0 and "nsamples" in PR.last_error(), PR.last_error()
    big = _inputs(5, 3, 129, (), 1, seed=15)
    got, rc = SR.call_summary(big, 1, 1)
    assert rc != 0 and "<= 128" in PR.last_error(), PR.last_error()
    assert PR.live_resources() == before


def test_no_quantiles():
    """nq = 0 (and a NULL hmsc_summary_args' worth of work): mean, occ and n alone."""
    inp = _inputs(70, 37, 3, ((2, 70),), 5, seed=16)
    got, rc = SR.call_summary(inp, 0, 3)
    assert rc == 0, PR.last_error()
    _assert_summary(got, _stack(inp, 0, 3), ())


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    hM = synthetic_model(ny=90, ns=9, nc=3, nf=2, nr=2, units=[90, 15], n_normal=2, n_poisson=3, seed=61, yscale=True)
    return H.sampleMcmc(hM, samples=12, transient=20, thin=2, nChains=2, updater={"GammaEta": False}, seed=5, verbose=0)


def _end_to_end(hM, **kw):
    predY = H.computePredictedValues(hM, expected=False, seed=3, **kw)
    sm = H.computePredictedValues(hM, expected=False, seed=3, summary=True, **kw)
    assert predY.shape[:2] == (hM.ny, hM.ns) and not np.any(np.isnan(predY))
    fam = hM.distr[:, 0]
    ref = SR.as_summary(predY, fam)
    assert np.array_equal(sm["probs"], [0.5]) and np.array_equal(sm["probs"], ref["probs"])
    got = dict(mean=sm["mean"], occ=sm["occ"], n=sm["n"], quantiles=sm["quantiles"])
    _assert_summary(got, predY, (0.5,), fam == 3, what=f"end to end {sorted(kw)}")
    assert _same(sm["median"], ref["median"]) and np.all(np.isnan(sm["median"][:, fam != 3]))
    with np.errstate(all="ignore"):
        a, b = H.evaluateModelFit(hM, predY), H.evaluateModelFit(hM, summary=sm)
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])), key
        assert np.all(np.abs(a[key] - b[key])[~np.isnan(a[key])] <= 1e-10), (key, a[key], b[key])


def test_end_to_end(fitted):
    """computePredictedValues(summary=True) against the reference summary of the array the same call
    returns, and evaluateModelFit from either: every key to 1e-10."""
    _end_to_end(fitted)


def test_end_to_end_probs(fitted):
    """probs on every column, 0.5 added for the Poisson columns."""
    hM = fitted
    predY = H.computePredictedValues(hM, expected=True, seed=3)
    sm = H.computePredictedValues(hM, expected=True, seed=3, summary=True, probs=(0.025, 0.975))
    assert np.array_equal(sm["probs"], [0.025, 0.975, 0.5]) and sm["quantiles"].shape == (3, hM.ny, hM.ns)
    _assert_summary(dict(mean=sm["mean"], occ=sm["occ"], n=sm["n"], quantiles=sm["quantiles"]), predY, sm["probs"],
                    what="end to end probs")
    assert _same(sm["median"], sm["quantiles"][2])


def test_end_to_end_partition(fitted):
    """2-fold cross-validation: each fold fills its held-out rows."""
    _end_to_end(fitted, partition=np.arange(fitted.ny) % 2 + 1)


def test_end_to_end_partition_sp(fitted):
    """2 x 2 partition / partition_sp: each species fold fills its columns, under the array path's
    seeds."""
    hM = fitted
    _end_to_end(hM, partition=np.arange(hM.ny) % 2 + 1, partition_sp=np.arange(hM.ns) % 2 + 1)
