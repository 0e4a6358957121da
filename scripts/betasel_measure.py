"""What variable selection (XSelect) costs at the config-4 shape.

    python scripts/betasel_measure.py [--steps 1000] [--reps 3] [--plain-only] [--out FILE]

Two chains on one GPU, Gamma2 and GammaEta off (R/sampleMcmc.R:207-216 clears both for an
XSelect model), every sweep recorded:
  sel    hmsc_amd.workloads.synthetic_probit (ny = 10 000, ns = 1 000, nc = 20, one
         sample-level random level with nf = 10, probit) with one selection on columns 16-20,
         spGroup = 1:ns (a group per species), q = 0.5
  plain  the same data without XSelect, the same updater switches: the same launches but for
         updateBetaSel and the BLx refresh, so the difference is the feature's cost
--plain-only runs the plain chain alone (a build of the parent commit, which has no XSelect).
Sweep rates are host wall clock around Chain.run (it ends in a device synchronise), the chains
alternating, after a warm-up that also captures the sweep graphs.  Kernel times come from a
separate eager pass with hmsc_profile (HIP events): id 11 = updateBetaSel (all its launches),
beside BetaLambda (id 2), updateZ (id 0) and the whole sweep (id 4).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hmsc_amd as H  # noqa: E402
from hmsc_amd.workloads import synthetic_probit  # noqa: E402


def models(ny, ns, plain_only):
    plain = synthetic_probit(ny=ny, ns=ns)
    out = dict(plain=plain)
    if not plain_only:
        sel = [dict(covGroup=[16, 17, 18, 19, 20], spGroup=np.arange(1, ns + 1), q=np.full(ns, 0.5))]
        out["sel"] = H.Hmsc(Y=plain.Y, X=plain.X, covNames=list(plain.covNames), XSelect=sel, distr="probit",
                            studyDesign=plain.studyDesign, ranLevels=plain.ranLevels)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ny", type=int, default=10000)
    ap.add_argument("--ns", type=int, default=1000)
    ap.add_argument("--prof-sweeps", type=int, default=50)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    up = {"Gamma2": False, "GammaEta": False}
    hms = models(a.ny, a.ns, a.plain_only)
    chains, it = {}, {}
    for name, hM in hms.items():
        ch = H.Chain(hM, 20261015, device=0, updater=up)
        ch.init()
        ch.run(transient=40, samples=0, adaptNf=[0], record=False)      # warm-up; graphs captured
        ch.run(transient=0, samples=32, adaptNf=[0], iter0=40)          # ... and the recorded ones
        chains[name], it[name] = ch, 72
    rates = {k: [] for k in chains}
    incl = None
    for _ in range(a.reps):
        for name, ch in chains.items():
            ch.sync()
            t0 = time.perf_counter()
            rec = ch.run(transient=0, samples=a.steps, adaptNf=[0], iter0=it[name])
            rates[name].append(a.steps / (time.perf_counter() - t0))
            it[name] += a.steps
            if name == "sel":
                incl = float(rec["BetaSel"].mean())
    res = dict(shape=dict(ny=a.ny, ns=a.ns, nc=20, nf=10, sel_cols=5, groups=a.ns), steps=a.steps,
               sweeps_per_s={k: [round(v, 1) for v in r] for k, r in rates.items()}, mean_inclusion=incl)
    prof = {}
    for name, ch in chains.items():
        ch.profile(True)
        for k in range(a.prof_sweeps):
            ch.sweep(it[name] + k)
        ch.sync()
        d = {}
        for pid in ("betasel", "betalambda", "eta_unit", "z", "sweep"):
            if pid not in ch.PROF_IDS:
                continue
            ms, n = ch.profile_get(pid)
            if n:
                d[pid] = dict(us_per_sweep=round(1e3 * ms / a.prof_sweeps, 2), launches_per_sweep=n / a.prof_sweeps)
        ch.profile(False)
        prof[name] = d
        ch.close()
    res["profile_eager"] = prof
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
