"""The numpy restatement of hmsc_predict_summary (hmsc_amd/csrc/summary.hip), and the C ABI call
from arrays (tests/test_host_predict_summary.py, tests/test_gpu_predict_summary.py).  Test
infrastructure only.

From a stacked ny x ns x S array of predictions, per cell over the samples in order:

    n      the number of values that are not NaN
    sum    sequential fp64 adds in sample order, NaN skipped, from 0.0; mean = sum / n
    occ    (number of values > 0) / n
    q(p)   R's type 7: h = (n - 1) p, lo = x_(floor h), hi = x_(ceil h) of the sorted non-NaN
           values, lo + (h - floor h) (hi - lo), and lo itself where hi = lo

n = 0 gives NaN everywhere.  Every operation is one IEEE double operation in a fixed order, so a
device that forms the same values in the same order returns the same bits.
"""
import ctypes as C

import numpy as np


def summarise(A, probs=(), qcols=None):
    """A: ny x ns x S.  Returns dict(mean, occ, n, pos, sum, abs_sum, quantiles (len(probs) x ny x ns),
    lo, hi (the order statistics used, same shape)).  qcols (ns, bool): columns that get quantiles
    (None: all); the others are NaN."""
    A = np.asarray(A, dtype=np.float64)
    ny, ns, S = A.shape
    ok = ~np.isnan(A)
    n = ok.sum(axis=2).astype(np.int32)
    total = np.zeros((ny, ns))
    for s in range(S):                               # the sequential sum, sample by sample
        total = np.where(ok[:, :, s], total + np.where(ok[:, :, s], A[:, :, s], 0.0), total)
    with np.errstate(invalid="ignore"):
        pos = (ok & (A > 0)).sum(axis=2).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / n
        occ = pos / n.astype(np.float64)
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    nq = len(probs)
    quant = np.full((nq, ny, ns), np.nan)
    lo, hi = quant.copy(), quant.copy()
    if nq:
        srt = np.sort(A, axis=2)                     # NaN last
        cols = np.ones(ns, dtype=bool) if qcols is None else np.asarray(qcols).astype(bool)
        has = (n > 0) & cols[None, :]
        nn = np.maximum(n, 1)
        for q, p in enumerate(probs):
            h = (nn - 1).astype(np.float64) * p
            fl = np.floor(h)
            g = h - fl
            k0 = fl.astype(np.int64)
            k1 = np.minimum(k0 + (g > 0), nn - 1)
            x0 = np.take_along_axis(srt, k0[:, :, None], axis=2)[:, :, 0]
            x1 = np.take_along_axis(srt, k1[:, :, None], axis=2)[:, :, 0]
            with np.errstate(invalid="ignore", over="ignore"):
                d = x1 - x0
                r = np.where(x1 != x0, x0 + g * d, x0)
            quant[q] = np.where(has, r, np.nan)
            lo[q] = np.where(has, x0, np.nan)
            hi[q] = np.where(has, x1, np.nan)
    return dict(mean=mean, occ=occ, n=n, pos=pos, sum=total, abs_sum=np.nansum(np.abs(A), axis=2), quantiles=quant,
                lo=lo, hi=hi, probs=probs)


def as_summary(A, fam, probs=()):
    """The dict predictSummary returns, from the stack: the caller's probs on every column, 0.5 added
    for Poisson columns; without probs the median of the Poisson columns only."""
    fam = np.asarray(fam)
    pois = fam == 3
    probs = [float(p) for p in probs]
    qcols = np.ones(len(fam), dtype=bool) if probs else pois
    if pois.any() and 0.5 not in probs:
        probs = probs + [0.5]
    r = summarise(A, probs, qcols)
    median = r["quantiles"][probs.index(0.5)].copy() if 0.5 in probs else np.full(r["mean"].shape, np.nan)
    return dict(mean=r["mean"], occ=r["occ"], n=r["n"], probs=np.array(probs), quantiles=r["quantiles"], median=median)


def mean_bound(A):
    """The forward error bound of a sequential fp64 sum of n terms, divided by n: n 2^-53 (sum |x| / n)
    (gamma_(n-1) sum |x| for the sum, one rounding for the division)."""
    A = np.asarray(A, dtype=np.float64)
    n = (~np.isnan(A)).sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return n * 2.0 ** -53 * (np.nansum(np.abs(A), axis=2) / n)


def longdouble_mean(A):
    A = np.asarray(A, dtype=np.float64)
    n = (~np.isnan(A)).sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nansum(A.astype(np.longdouble), axis=2) / n


def call_summary(inp, expected, seed, probs=(), qcols=None, scratch_bytes=0, device=0):
    """hmsc_predict_summary on a dict of inputs in predict_reference.build_inputs' layout (X ny x nc;
    Beta S x nc x ns; sigma S x ns; family ns; YScalePar 2 x ns; Pi ny x nr 1-based; np, nf; Eta[r]
    S x np_r x nf_r; Lambda[r] S x nf_r x ns).  Returns (dict or None, return code)."""
    from hmsc_amd import _lib as L
    X = np.asarray(inp["X"], dtype=np.float64)
    Beta = np.asarray(inp["Beta"], dtype=np.float64)
    S, nc, ns = Beta.shape
    ny, nr = X.shape[0], len(inp["nf"])
    cm = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).transpose(0, 2, 1)).ravel()  # noqa: E731
    keep = [np.ascontiguousarray(X.ravel(order="F")), cm(Beta), L.f64(np.asarray(inp["sigma"]).ravel()),
            L.i32(inp["family"]), L.f64(np.asarray(inp["YScalePar"], dtype=np.float64).ravel(order="F")),
            L.i32(np.asarray(inp["Pi"]).reshape(ny, nr).ravel(order="F") if nr else [0]),
            L.i32(inp["np"] if nr else [0]), L.i32(inp["nf"] if nr else [0])]
    a = L.hmsc_predict_args()
    a.ny, a.ns, a.nc, a.nr, a.nsamples = ny, ns, nc, nr, int(inp.get("nsamples", S))
    a.expected, a.seed, a.device = int(expected), int(seed), int(device)
    a.X, a.Beta, a.sigma = L.fptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2])
    a.family, a.YScalePar = L.iptr(keep[3]), L.fptr(keep[4])
    a.Pi, a.np, a.nf = L.iptr(keep[5]), L.iptr(keep[6]), L.iptr(keep[7])
    for r in range(nr):
        e, lm = cm(inp["Eta"][r]), cm(inp["Lambda"][r])
        keep += [e, lm]
        a.Eta[r], a.Lambda[r] = L.fptr(e), L.fptr(lm)
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    nq = len(probs)
    qc = L.i32(np.ones(ns) if qcols is None else np.asarray(qcols).astype(np.int32))
    q = L.hmsc_summary_args()
    q.nq, q.scratch_bytes = nq, int(scratch_bytes)
    q.probs, q.qcols = (L.fptr(probs), L.iptr(qc)) if nq else (None, None)
    mean, occ = np.full(ny * ns, 7.25), np.full(ny * ns, 7.25)
    n = np.full(ny * ns, -7, dtype=np.int32)
    quant = np.full(max(nq, 1) * ny * ns, 7.25)
    rc = L.lib().hmsc_predict_summary(C.byref(a), C.byref(q), L.fptr(mean), L.fptr(occ), L.iptr(n),
                                      L.fptr(quant) if nq else None)
    if rc != 0:
        return None, rc
    return dict(mean=mean.reshape(ns, ny).T, occ=occ.reshape(ns, ny).T, n=n.reshape(ns, ny).T,
                quantiles=quant.reshape(max(nq, 1), ns, ny).transpose(0, 2, 1)[:nq], probs=probs), rc
