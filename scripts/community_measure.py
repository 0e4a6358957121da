"""Community-level posterior summaries (hmsc_predict_community, community.hip) against the route through
the prediction array (predict + numpy reductions) at the config-4 shape, on one MI355X.

    python scripts/community_measure.py [--out profiles/community_measure.txt] [--samples 20,200,1000]

ny = 10 000, ns = 1 000, nc = 20, one level with np = ny and nf = 10, probit; Tr = [1, three N(0, 1)
traits] (nt = 4), so measures ("S", "T") are nw = 5 columns; the posterior stacks are generated from
a seed as scripts/summary_measure.py makes them (no fit: the cost does not depend on the values).
(a) the array route at S = 20, which is what fits: predict, then per sample rowSums and
(a %*% Tr) / rowSums(a), then type-7 quantiles and Pr per site; (b) predictCommunity at every S, split
by hmsc_debug_community_timing (host clock around the synchronised launches); one warm-up call per
shape, then three timed calls, medians.  Kernel A's rate in cells (ny ns S) per second stands beside
predict_summary_kernel's on the same cells, from summary_measure's own path (b) in the same process.
The S = 20 result of (b) is compared with (a)'s under the bounds of tests/test_gpu_community.py."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import hmsc_amd as H  # noqa: E402
from hmsc_amd import _lib as L  # noqa: E402
from hmsc_amd.gradient import quantile7  # noqa: E402
from hmsc_amd.workloads import synthetic_probit  # noqa: E402
import summary_measure as SM  # noqa: E402

PROBS = (0.025, 0.5, 0.975)
NT = 4


def community_ms():
    ms = np.zeros(3)
    L.check(L.lib().hmsc_debug_community_timing(L.fptr(ms)))
    return ms


def path_a(hM, expected):
    """The route that needs the array: predict, then the reductions on the host."""
    t0 = time.perf_counter()
    predY = H.predict(hM, expected=expected, seed=3)
    t1 = time.perf_counter()
    Tr = np.asarray(hM.Tr)
    A = np.stack(predY, axis=0)                                             # S x ny x ns
    rs = A.sum(axis=2)
    with np.errstate(all="ignore"):
        C = np.concatenate([rs[:, :, None], (A @ Tr) / rs[:, :, None]], axis=2)   # S x ny x (1 + nt)
        q = quantile7(C.transpose(1, 2, 0), PROBS)
        mean = np.nanmean(C, axis=0)
        pr = np.mean(C[:, -1] > C[:, 0], axis=0)
    return t1 - t0, time.perf_counter() - t1, A, C, q, mean, pr


def path_b(hM, expected, samples=False):
    t0 = time.perf_counter()
    res = H.predictCommunity(hM, expected=expected, seed=3, measures=("S", "T"), probs=PROBS,
                             contrast=(0, hM.ny - 1), returnSamples=samples)
    return time.perf_counter() - t0, res, community_ms()


def check(res, A, hM):
    """The value bounds of tests/test_gpu_community.py at the timed size, on the first 256 sites of
    every sample (the longdouble reference of all 1e4 sites would take minutes), and the statistics
    of the device's own samples on every site."""
    import community_reference as CR
    W = np.column_stack([np.ones(hM.ns), hM.Tr])
    norm = [0] + [1] * hM.nt
    ref = CR.community_wide(A[:, :256], W, norm, 0)
    bound = CR.value_bound(ref, norm, hM.ns)
    got = res["samples"][:, :256]
    fin = np.isfinite(ref["C"])
    assert np.array_equal(np.isnan(got), np.isnan(ref["C"]))
    ratio = (np.abs(got[fin].astype(np.longdouble) - ref["C"][fin]) / bound[fin]).astype(np.float64)
    assert np.all(ratio <= 1.0)
    st = CR.statistics(res["samples"], PROBS, ((0, hM.ny - 1),))
    assert np.array_equal(res["n"], st["n"]) and np.array_equal(res["quantiles"], st["quantiles"], equal_nan=True)
    assert np.array_equal(res["Pr"], st["Pr"], equal_nan=True)
    return (f"values of the first 256 sites within the bound (worst error / bound {float(ratio.max()):.3f}); n, quantiles "
            f"and Pr of all sites equal numpy's on the returned samples exactly")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "community_measure.txt"))
    ap.add_argument("--samples", default="20,200,1000")
    args = ap.parse_args()
    sizes = [int(s) for s in args.samples.split(",")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hM = synthetic_probit(ny=SM.NY, ns=SM.NS, nc=SM.NC, nf=SM.NF)
    rng = np.random.default_rng(7)
    hM.Tr = np.column_stack([np.ones(SM.NS)] + [rng.standard_normal(SM.NS) for _ in range(NT - 1)])
    hM.nt, hM.trNames = NT, ["(Intercept)"] + [f"T{k}" for k in range(1, NT)]
    post = SM.make_post(max(sizes))
    cells = float(SM.NY) * SM.NS
    med = lambda v: float(np.median(v))  # noqa: E731
    say(f"community_measure: ny = {SM.NY}, ns = {SM.NS}, nc = {SM.NC}, nf = {SM.NF} (K = {SM.NC + SM.NF}), probit, "
        f"nt = {NT}: nw = {1 + NT} columns (S and the traits' community-weighted means); stacks from a seed")
    for expected in (True, False):
        say()
        say(f"expected = {expected}")
        hM.postList = [post[:2]]
        path_a(hM, expected), path_b(hM, expected), SM.path_b(hM, expected)        # warm-up: module load, allocator
        hM.postList = [post[:20]]
        ta, a = [], None
        for _ in range(3):
            del a
            a = path_a(hM, expected)
            ta.append(a[:2])
        say(f"  (a) array route  S = 20: predict {med([t[0] for t in ta]):.3f} s, numpy reductions "
            f"{med([t[1] for t in ta]):.3f} s")
        b = path_b(hM, expected, samples=True)
        say("      S = 20, (b) against (a)'s array: " + check(b[1], a[2], hM))
        del a, b
        for S in sizes:
            hM.postList = [post[:S]]
            path_b(hM, expected)
            tb = [path_b(hM, expected) for _ in range(3)]
            ms = np.median([t[2] for t in tb], axis=0)
            sm = np.median([SM.path_b(hM, expected)[4] for _ in range(3)], axis=0)
            say(f"  (b) predictCommunity S = {S}: call {med([t[0] for t in tb]):.3f} s; uploads {ms[0]:.1f} ms, kernel A "
                f"{ms[1]:.2f} ms = {S * cells / ms[1] * 1e-6:.1f} G cells/s, statistics + copy back {ms[2]:.1f} ms; "
                f"predict_summary_kernel on the same cells {sm[1]:.2f} ms = {S * cells / sm[1] * 1e-6:.1f} G cells/s "
                f"(kernel A at {sm[1] / ms[1]:.2f} of its rate)")
            del tb
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
