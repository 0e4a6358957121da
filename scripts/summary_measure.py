"""Posterior predictive summaries (hmsc_predict_summary, summary.hip) against the array path
(computePredictedValues + evaluateModelFit) at the config-4 shape, on one MI355X.

    python scripts/summary_measure.py [--out profiles/summary_measure.txt] [--samples 20,200,1000]
                                      [--z-us 77.8] [--trace-only]

ny = 10 000, ns = 1 000, nc = 20, one level with np = ny and nf = 10, probit; the posterior stacks
are generated from a seed (no fit: the cost does not depend on the values).  (a) the array path at
S = 20, which is what fits; (b) computePredictedValues(summary=True) + evaluateModelFit(summary=)
at every S; both for expected = True and False; one warm-up call per shape, then three timed calls,
(a) and (b) alternating where both exist; medians.  Kernel times: hmsc_debug_summary_timing (host
clock around the synchronised launches).  hmsc_predict has no such split, so predict_kernel's time
comes from a kernel trace: --trace-only runs each path once at S = 20, for a separate run under
`rocprofv3 --kernel-trace --stats`.
The quantile kernel is measured on a variant with 100 Poisson columns at S = 200 and S = 1000.
The S = 20 summary is compared with the reference summary (tests/summary_reference.py) of path
(a)'s array with the assertions of tests/test_gpu_predict_summary.py.

--z-us: the z kernel's live time per launch at config 4 from the README (77.8 us for 1e7 cells)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hmsc_amd as H  # noqa: E402
from hmsc_amd import _lib as L  # noqa: E402
from hmsc_amd.workloads import synthetic_probit  # noqa: E402

NY, NS, NC, NF = 10000, 1000, 20, 10


def make_post(S, seed=20261020):
    rng = np.random.default_rng(seed)
    lam_scale = 1.0 / np.arange(1, NF + 1)[:, None]
    return [dict(Beta=rng.normal(0.0, 0.3, (NC, NS)), sigma=np.ones(NS), Eta=[rng.standard_normal((NY, NF))],
                 Lambda=[rng.standard_normal((NF, NS)) * lam_scale], Alpha=[np.zeros(NF, dtype=np.int64)])
            for _ in range(S)]


def summary_ms():
    ms = np.zeros(3)
    L.check(L.lib().hmsc_debug_summary_timing(L.fptr(ms)))
    return ms


def path_a(hM, expected):
    t0 = time.perf_counter()
    predY = H.computePredictedValues(hM, expected=expected, seed=3)
    t1 = time.perf_counter()
    with np.errstate(all="ignore"):
        mf = H.evaluateModelFit(hM, predY)
    return t1 - t0, time.perf_counter() - t1, predY, mf


def path_b(hM, expected, probs=()):
    t0 = time.perf_counter()
    sm = H.computePredictedValues(hM, expected=expected, seed=3, summary=True, probs=probs)
    t1 = time.perf_counter()
    with np.errstate(all="ignore"):
        mf = H.evaluateModelFit(hM, summary=sm)
    return t1 - t0, time.perf_counter() - t1, sm, mf, summary_ms()


def check_equal(sm, predY, fam, probs):
    """The tests' assertions at the timed size; returns a line for the profile."""
    import summary_reference as SR
    ref = SR.summarise(predY, sm["probs"], None if len(probs) else fam == 3)
    assert np.array_equal(sm["n"], ref["n"])
    assert np.array_equal(sm["occ"], ref["occ"], equal_nan=True)
    assert np.array_equal(sm["quantiles"], ref["quantiles"], equal_nan=True)
    ok = ref["n"] > 0
    err = np.abs(sm["mean"].astype(np.longdouble) - SR.longdouble_mean(predY))[ok].astype(np.float64)
    assert np.all(err <= SR.mean_bound(predY)[ok])
    eq = int(np.sum(sm["mean"][ok] == ref["mean"][ok]))
    return (f"n, occ and quantiles equal exactly; every mean within n 2^-53 mean|x| of the longdouble mean; "
            f"{eq} of {int(ok.sum())} means bit-equal to the sequential restatement")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_measure.txt"))
    ap.add_argument("--samples", default="20,200,1000")
    ap.add_argument("--z-us", type=float, default=77.8)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    sizes = [int(s) for s in args.samples.split(",")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hM = synthetic_probit(ny=NY, ns=NS, nc=NC, nf=NF)
    fam = hM.distr[:, 0]
    post = make_post(max(sizes))
    cells = float(NY) * NS
    if args.trace_only:
        hM.postList = [post[:20]]
        for expected in (True, False):
            path_a(hM, expected)
            path_b(hM, expected)
        return
    say(f"summary_measure: ny = {NY}, ns = {NS}, nc = {NC}, nf = {NF} (K = {NC + NF}), probit; stacks from a seed")
    say(f"z kernel, live, config 4 (README): {args.z_us:.1f} us per 1e7 cells = {cells / args.z_us * 1e-3:.1f} G cells/s")
    for expected in (True, False):
        say()
        say(f"expected = {expected}")
        hM.postList = [post[:2]]
        path_a(hM, expected), path_b(hM, expected)                 # warm-up: module load, allocator
        hM.postList = [post[:20]]
        ta, tb = [], []
        for _ in range(3):
            a = path_a(hM, expected)
            b = path_b(hM, expected)
            ta.append(a[:2]), tb.append(b[:2] + (b[4],))
        med = lambda v: float(np.median(v))  # noqa: E731
        say(f"  (a) array path   S = 20: computePredictedValues {med([t[0] for t in ta]):.3f} s, evaluateModelFit "
            f"{med([t[1] for t in ta]):.3f} s")
        ms = np.median([t[2] for t in tb], axis=0)
        say(f"  (b) summary path S = 20: computePredictedValues {med([t[0] for t in tb]):.3f} s, evaluateModelFit "
            f"{med([t[1] for t in tb]):.3f} s; uploads {ms[0]:.1f} ms, summary kernel {ms[1]:.2f} ms = "
            f"{20 * cells / ms[1] * 1e-6:.1f} G cells/s, quantiles + copy back {ms[2]:.1f} ms")
        say("      S = 20 summary against the reference summary of (a)'s array: " + check_equal(b[2], a[2], fam, ()))
        worst = max(float(np.nanmax(np.abs(a[3][k] - b[3][k]))) for k in a[3])
        say(f"      evaluateModelFit, (a) against (b): worst difference over all keys {worst:.2e}")
        del a, b
        for S in sizes:
            if S == 20:
                continue
            hM.postList = [post[:S]]
            path_b(hM, expected)
            tb = [path_b(hM, expected) for _ in range(3)]
            ms = np.median([t[4] for t in tb], axis=0)
            say(f"  (b) summary path S = {S}: computePredictedValues {med([t[0] for t in tb]):.3f} s, evaluateModelFit "
                f"{med([t[1] for t in tb]):.3f} s; uploads {ms[0]:.1f} ms, summary kernel {ms[1]:.2f} ms = "
                f"{S * cells / ms[1] * 1e-6:.1f} G cells/s, quantiles + copy back {ms[2]:.1f} ms")
            del tb
    say()
    say("quantile kernel: the first 100 columns Poisson, expected = False, median of those columns")
    hM.distr[:100, 0] = 3
    for S in [s for s in sizes if s >= 200]:
        hM.postList = [post[:S]]
        path_b(hM, False)
        tb = [path_b(hM, False) for _ in range(3)]
        ms = np.median([t[4] for t in tb], axis=0)
        # the copy back of mean, occ, n and one quantile plane is in ms[2]: time it apart by the nq = 0 call
        read = 65.0 * S * 8 * NY * 100
        say(f"  S = {S}: call {np.median([t[0] for t in tb]):.3f} s; uploads {ms[0]:.1f} ms, summary kernels {ms[1]:.1f} ms, "
            f"quantile kernels + copy back {ms[2]:.1f} ms; the quantile kernels read {read * 1e-9:.1f} GB "
            f"(65 passes x n x 8 B per cell): at most {read / ms[2] * 1e-9:.2f} TB/s over that time")
        del tb
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
