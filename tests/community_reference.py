"""The numpy restatement of hmsc_predict_community (hmsc_amd/csrc/community.hip), the C ABI call from
arrays, and plotGradient's formulas (R/plotGradient.R:93-138) written out literally
(tests/test_host_gradient.py, tests/test_gpu_community.py).  Test infrastructure only.

From a stack A (S x ny x ns) of predictions, weights W (ns x nw), normalise flags and a transform g
(identity or exp), per sample s, site i and column m

    num = sum over j with W[j, m] != 0 of g(A[s, i, j]) W[j, m]
    den = sum over j of g(A[s, i, j])
    C[s, i, m] = num / den if normalise[m] else num

A zero weight is a select: the species does not enter num at all, whatever it holds.
"""
import ctypes as C

import numpy as np

import summary_reference as SR

U = 2.0 ** -53


def _fp64_range(x):
    """A longdouble value beyond fp64's range is +-inf on the device: IEEE's result of the exp, the
    product or the sum that formed it."""
    big = np.longdouble(np.finfo(np.float64).max)
    return np.where(np.abs(x) > big, np.sign(x) * np.longdouble(np.inf), x)


def community_wide(A, W, normalise, transform):
    """C in longdouble, with what the error bounds need; an exp, a product or a sum beyond fp64's
    range is infinite, as it is in IEEE fp64 arithmetic.  Returns dict(C, num, den (S x ny [x nw]),
    abs_t = sum |t_j| (S x ny x nw), abs_g = sum |g_j| (S x ny))."""
    A = np.asarray(A, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    S, ny, ns = A.shape
    nw = W.shape[1]
    wide = A.astype(np.longdouble)
    with np.errstate(over="ignore", invalid="ignore"):
        G = np.exp(wide) if transform else wide
        G = _fp64_range(G)
    with np.errstate(invalid="ignore"):
        den = _fp64_range(G.sum(axis=2))
        abs_g = np.abs(G).sum(axis=2)
    num = np.zeros((S, ny, nw), dtype=np.longdouble)
    abs_t = np.zeros((S, ny, nw), dtype=np.longdouble)
    for m in range(nw):
        use = W[:, m] != 0.0                       # the select
        with np.errstate(invalid="ignore", over="ignore"):
            t = _fp64_range(G[:, :, use] * W[use, m].astype(np.longdouble))
            num[:, :, m] = _fp64_range(t.sum(axis=2))
            abs_t[:, :, m] = np.abs(t).sum(axis=2)
    Cw = num.copy()
    for m in range(nw):
        if normalise[m]:
            with np.errstate(invalid="ignore", divide="ignore"):
                Cw[:, :, m] = num[:, :, m] / den
    return dict(C=Cw, num=num, den=den, abs_t=abs_t, abs_g=abs_g)


def community_ordered(A, W, normalise, transform):
    """C in fp64 in the device's documented order: four partial sums per site, partial l over the
    species j = l mod 4 in ascending j from 0.0 (for num the rounded product g W, skipped at a zero
    weight), then ((s_0 + s_1) + s_2) + s_3.  g = np.exp on the host, which need not round as the
    device's exp does."""
    A = np.asarray(A, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    S, ny, ns = A.shape
    nw = W.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        G = np.exp(A) if transform else A
        den_l = np.zeros((4, S, ny))
        num_l = np.zeros((4, S, ny, nw))
        for j in range(ns):
            den_l[j % 4] = den_l[j % 4] + G[:, :, j]
            for m in range(nw):
                if W[j, m] != 0.0:
                    num_l[j % 4, :, :, m] = num_l[j % 4, :, :, m] + G[:, :, j] * W[j, m]
        den = ((den_l[0] + den_l[1]) + den_l[2]) + den_l[3]
        num = ((num_l[0] + num_l[1]) + num_l[2]) + num_l[3]
        out = num.copy()
        for m in range(nw):
            if normalise[m]:
                with np.errstate(divide="ignore"):
                    out[:, :, m] = num[:, :, m] / den
    return out


def value_bound(ref, normalise, ns):
    """The bound of the value test, per (s, i, m): a plain column (ns + 4) u sum |t_j|; a normalised
    one 1.01 [(ns + 4) u (sum |t_j| + |C| sum |g_j|) / |den| + u |C|]."""
    nw = ref["C"].shape[2]
    out = np.empty(ref["C"].shape, dtype=np.longdouble)
    for m in range(nw):
        if normalise[m]:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                c = np.abs(ref["C"][:, :, m])
                out[:, :, m] = 1.01 * ((ns + 4) * U * (ref["abs_t"][:, :, m] + c * ref["abs_g"]) / np.abs(ref["den"]) + U * c)
        else:
            out[:, :, m] = (ns + 4) * U * ref["abs_t"][:, :, m]
    return out


def statistics(comm, probs=(), pairs=()):
    """The per-site statistics of a stack comm (S x ny x nw): summary_reference.summarise on the
    ny x nw x S stack, and Pr per pair (a, b) and column: the share of samples with
    comm[s, b, m] > comm[s, a, m], NaN if either holds a NaN in any sample."""
    comm = np.asarray(comm, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = SR.summarise(np.ascontiguousarray(comm.transpose(1, 2, 0)), probs)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pr = np.full((len(pairs), comm.shape[2]), np.nan)
    for k, (a, b) in enumerate(pairs):
        for m in range(comm.shape[2]):
            xa, xb = comm[:, a, m], comm[:, b, m]
            if not (np.isnan(xa).any() or np.isnan(xb).any()):
                pr[k, m] = np.mean(xb > xa)
    r["Pr"] = pr
    return r


def plot_gradient(predY, measure, index, q, Tr, all_normal):
    """R/plotGradient.R:93-138 literally, from the list predY of ngrid x ns arrays: (Pr, qpred
    (len(q) x ngrid)).  Quantiles are summary_reference's type 7."""
    ngrid = predY[0].shape[0]
    if measure == "S":
        pred = np.stack([a.sum(axis=1) for a in predY], axis=1)                 # abind(lapply(predY, rowSums), along=2)
    elif measure == "Y":
        pred = np.stack(predY, axis=2)[:, index, :]
    else:
        def one(a):
            g = np.exp(a) if all_normal else a
            with np.errstate(invalid="ignore", divide="ignore"):
                return (g @ Tr) / np.repeat(g.sum(axis=1)[:, None], Tr.shape[1], axis=1)
        pred = np.stack([one(a) for a in predY], axis=2)[:, index, :]
    last, first = pred[ngrid - 1], pred[0]
    Pr = np.nan if (np.isnan(last).any() or np.isnan(first).any()) else float(np.mean(last > first))
    qpred = SR.summarise(pred[:, None, :], q)["quantiles"][:, :, 0]
    return Pr, qpred


def predict_args(inp, expected, seed, keep, device=0):
    """hmsc_predict_args from a dict in predict_reference.build_inputs' layout (as
    summary_reference.call_summary fills it)."""
    from hmsc_amd import _lib as L
    X = np.asarray(inp["X"], dtype=np.float64)
    Beta = np.asarray(inp["Beta"], dtype=np.float64)
    S, nc, ns = Beta.shape
    ny, nr = X.shape[0], len(inp["nf"])
    cm = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).transpose(0, 2, 1)).ravel()  # noqa: E731
    k0 = [np.ascontiguousarray(X.ravel(order="F")), cm(Beta), L.f64(np.asarray(inp["sigma"]).ravel()),
          L.i32(inp["family"]), L.f64(np.asarray(inp["YScalePar"], dtype=np.float64).ravel(order="F")),
          L.i32(np.asarray(inp["Pi"]).reshape(ny, nr).ravel(order="F") if nr else [0]),
          L.i32(inp["np"] if nr else [0]), L.i32(inp["nf"] if nr else [0])]
    a = L.hmsc_predict_args()
    a.ny, a.ns, a.nc, a.nr, a.nsamples = ny, ns, nc, nr, int(inp.get("nsamples", S))
    a.expected, a.seed, a.device = int(expected), int(seed), int(device)
    a.X, a.Beta, a.sigma = L.fptr(k0[0]), L.fptr(k0[1]), L.fptr(k0[2])
    a.family, a.YScalePar = L.iptr(k0[3]), L.fptr(k0[4])
    a.Pi, a.np, a.nf = L.iptr(k0[5]), L.iptr(k0[6]), L.iptr(k0[7])
    keep += k0
    for r in range(nr):
        e, lm = cm(inp["Eta"][r]), cm(inp["Lambda"][r])
        keep += [e, lm]
        a.Eta[r], a.Lambda[r] = L.fptr(e), L.fptr(lm)
    return a, S, ny, ns


def call_community(inp, expected, seed, W, normalise, transform=0, probs=(), pairs=(), scratch_bytes=0, want_comm=True,
                   nw=None, raw_pairs=None, null=()):
    """hmsc_predict_community on a dict of inputs.  W: ns x nw.  nw overrides the column count
    passed (for refusals); null names arguments passed as NULL ("p", "c", "n", "mean", "W").
    Returns (dict(n, mean (ny x nw), quantiles (nq x ny x nw), Pr (npairs x nw), comm (S x ny x nw
    or None)) or None, return code)."""
    from hmsc_amd import _lib as L
    keep = []
    a, S, ny, ns = predict_args(inp, expected, seed, keep)
    W = np.asarray(W, dtype=np.float64).reshape(ns, -1)
    k = W.shape[1]
    Wf = np.ascontiguousarray(W.ravel(order="F"))
    norm = L.i32(np.asarray(normalise).astype(np.int32))
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    pr_in = np.ascontiguousarray(np.asarray(pairs if raw_pairs is None else raw_pairs, dtype=np.int32).reshape(-1))
    nq, npairs = len(probs), len(pr_in) // 2
    c = L.hmsc_community_args()
    c.nw = k if nw is None else int(nw)
    c.W = None if "W" in null else L.fptr(Wf)
    c.normalise = L.iptr(norm)
    c.transform, c.nq, c.npairs, c.scratch_bytes = int(transform), nq, npairs, int(scratch_bytes)
    c.probs = L.fptr(probs) if nq else None
    c.pairs = L.iptr(pr_in) if npairs else None
    kk = max(k, c.nw, 1)
    n = np.full(ny * kk, -7, dtype=np.int32)
    mean = np.full(ny * kk, 7.25)
    quant = np.full(max(nq, 1) * ny * kk, 7.25)
    pr = np.full(max(npairs, 1) * kk, 7.25)
    comm = np.full(S * ny * kk, 7.25) if want_comm else None
    rc = L.lib().hmsc_predict_community(None if "p" in null else C.byref(a), None if "c" in null else C.byref(c),
                                        None if "n" in null else L.iptr(n), None if "mean" in null else L.fptr(mean),
                                        L.fptr(quant) if nq else None, L.fptr(pr) if npairs else None,
                                        L.fptr(comm) if want_comm else None)
    if rc != 0:
        return None, rc
    return dict(n=n.reshape(k, ny).T, mean=mean.reshape(k, ny).T,
                quantiles=quant.reshape(max(nq, 1), k, ny).transpose(0, 2, 1)[:nq],
                Pr=pr[:npairs * k].reshape(k, npairs).T,
                comm=comm.reshape(S, k, ny).transpose(0, 2, 1) if want_comm else None), rc


def community_timing():
    from hmsc_amd import _lib as L
    out = (C.c_double * 3)()
    L.check(L.lib().hmsc_debug_community_timing(out))
    return list(out)
