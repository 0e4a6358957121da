"""Conditional prediction of spatial models, predict(Yc, condBatch=True, condSpatial=True)
(hmsc_predict_conditional_spatial, cond.hip) against condBatch=False (the per-sample loop over
hmsc_set_state / hmsc_update / hmsc_get_state on a chain of the prediction design), on one MI355X.

    python scripts/cond_spatial_measure.py [--out profiles/cond_spatial_measure.txt] [--cases full,gpp]

Case full: spatial_vignette4 'Full' at a cross-validation fold's size, ny = np = 500, 200 samples,
mcmcStep = 10.  Case gpp: spatial_vignette4 'GPP' at ny = 5000, 200 samples, mcmcStep = 10.  The
posterior of a short chain; one of the five species is held out (its column of Yc is NA).  The
batched path: one warm-up call on two samples, then three timed calls, the median reported; the
conditioning step alone (_conditional_etas_batched) and predict as a whole separately, with the four
slots of hmsc_debug_cond_timing of the last call.  The per-sample loop is existing code and is
timed on --loop-samples samples (three runs, the median) and scaled to all of them: its cost per
sample does not depend on the number of samples beyond the chain it builds once, which is timed
with it."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hmsc_amd as H  # noqa: E402
from hmsc_amd import _lib as L  # noqa: E402
from hmsc_amd.workloads import spatial_vignette4  # noqa: E402

CASES = dict(full=dict(ny=500, method="Full", S=200, mcmcStep=10),
             gpp=dict(ny=5000, method="GPP", S=200, mcmcStep=10))


def wall(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def measure(name, loop_samples):
    c = CASES[name]
    S, m = c["S"], c["mcmcStep"]
    hM = spatial_vignette4(ny=c["ny"], method=c["method"])
    H.sampleMcmc(hM, samples=S, transient=20, nChains=1, seed=1, verbose=0,
                 updater=None if c["method"] == "Full" else {"GammaEta": False})   # (no GammaEta for 'GPP', as in R)
    post = H.poolMcmcChains(hM.postList)
    Yc = np.array(hM.Y, dtype=np.float64)
    Yc[:, -1] = np.nan
    Pm = importlib.import_module("hmsc_amd.predict")
    X = np.asarray(hM.X, dtype=np.float64)
    betas = [np.asarray(s["Beta"], dtype=np.float64) for s in post]
    used = len(np.unique(np.concatenate([np.asarray(s["Alpha"][0]).ravel() for s in post])))
    kw = dict(Yc=Yc, mcmcStep=m, expected=True, seed=7)

    H.predict(hM, post=post[:2], condBatch=True, condSpatial=True, **kw)                  # warm-up
    bat, bstep = [], []
    for _ in range(3):
        t, pb = wall(lambda: H.predict(hM, post=post, condBatch=True, condSpatial=True, **kw))
        bat.append(t)
        ms = np.zeros(4)
        L.check(L.lib().hmsc_debug_cond_timing(L.fptr(ms)))
    for _ in range(3):
        bstep.append(wall(lambda: Pm._conditional_etas_batched(hM, post, X, betas, hM.studyDesign, Yc, m,
                                                               np.random.default_rng(7), 0, spatial=True))[0])
    n = loop_samples
    H.predict(hM, post=post[:2], **kw)                                                    # warm-up
    loop, lstep = [], []
    for _ in range(3):
        t, pl = wall(lambda: H.predict(hM, post=post[:n], **kw))
        loop.append(t)
        lstep.append(wall(lambda: Pm._conditional_etas(hM, post[:n], X, hM.studyDesign, Yc, m,
                                                       np.random.default_rng(7), 0))[0])
    diff = max(float(np.max(np.abs(a - b))) for a, b in zip(pl, pb[:n]))
    mb, ml, sb, sl = (float(np.median(v)) for v in (bat, loop, bstep, lstep))
    fmt = lambda v: " / ".join(f"{t:.3f}" for t in v)  # noqa: E731
    return [f"case {name}: spatial_vignette4 '{c['method']}', ny = np = {c['ny']}, ns = {hM.ns}, nf = 1, S = {S}, mcmcStep = {m}, "
            f"one of {hM.ns} species held out; {used} grid values in use" +
            (f", {np.asarray(hM.rL[0]['sKnot']).shape[0]} knots" if c["method"] == "GPP" else ""),
            f"  predict(condBatch=True, condSpatial=True), all {S} samples, wall, 3 runs: {fmt(bat)} s (median {mb:.3f})",
            f"  predict(condBatch=False), {n} samples, wall, 3 runs: {fmt(loop)} s (median {ml:.3f}); scaled to {S} samples: "
            f"{ml * S / n:.2f} s",
            f"  predict as a whole, per-sample loop (scaled) / batched: {ml * S / n / mb:.1f}x",
            f"  the conditioning step alone: batched {fmt(bstep)} s (median {sb:.3f}); loop on {n} samples {fmt(lstep)} s "
            f"(median {sl:.3f}), scaled {sl * S / n:.2f} s; loop (scaled) / batched: {sl * S / n / sb:.1f}x",
            f"  batched call, last run (hmsc_debug_cond_timing): upload + allocation + grid + factors {ms[0]:.2f} ms, Z launches "
            f"{ms[1]:.3f} ms ({m + 1} launches), Eta steps {ms[2]:.3f} ms ({m} steps), copy back {ms[3]:.2f} ms",
            f"  max |expected value, batched - loop| over the first {n} samples: {diff:.2e}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_spatial_measure.txt"))
    ap.add_argument("--cases", default="full,gpp")
    ap.add_argument("--loop-samples", type=int, default=10)
    args = ap.parse_args()
    lines = ["Conditional prediction of spatial models, batched (cond.hip, condSpatial) against the per-sample loop, "
             "one MI355X: python scripts/cond_spatial_measure.py", ""]
    for name in args.cases.split(","):
        lines += measure(name, args.loop_samples) + [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
