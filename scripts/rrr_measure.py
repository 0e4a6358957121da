"""What reduced-rank regression covariates cost at the config-4 shape.

    python scripts/rrr_measure.py [--steps 1000] [--reps 3] [--out FILE]

Two chains on one GPU, GammaEta off, every sweep recorded:
  rrr    ny = 10 000, ns = 1 000, 20 plain columns + ncRRR = 2 components of ncORRR = 10
         covariates (nc = 22), one sample-level random level with nf = 10, probit
  plain  the same data with 22 plain columns and no XRRR (the fused sweep)
Sweep rates are host wall clock around Chain.run (it ends in a device synchronise), the two
chains alternating, after a warm-up that also captures the sweep graphs.  Kernel times come from
a separate eager pass with hmsc_profile (HIP events): id 10 = updatewRRR's pass over Z, beside
the launch of updateEta that reads Z once (the fused Eta kernel, id 3, when the chain takes it;
the ZL pass, id 1, otherwise) and updateZ (id 0).  Bytes: the Z pass and Eta's read ny ns 8 B.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hmsc_amd as H  # noqa: E402
from hmsc_amd.workloads import SYNTHETIC_SEED  # noqa: E402


def models(ny, ns, ncN, ncRRR, ncORRR, nf):
    import pandas as pd
    rng = np.random.default_rng(SYNTHETIC_SEED)
    X = np.column_stack([np.ones(ny), rng.standard_normal((ny, ncN - 1))])
    XR = rng.standard_normal((ny, ncORRR))
    w = rng.normal(0.0, 0.5, (ncRRR, ncORRR))
    Xf = np.hstack([X, XR @ w.T])
    B = rng.normal(0.0, 0.5, (ncN + ncRRR, 1)) + rng.normal(0.0, 0.3, (ncN + ncRRR, ns))
    Lp = Xf @ B + rng.standard_normal((ny, nf)) @ (rng.standard_normal((nf, ns)) / np.arange(1, nf + 1)[:, None])
    Y = (Lp + rng.standard_normal((ny, ns)) > 0).astype(np.float64)
    units = np.arange(1, ny + 1)

    def level():
        rl = H.HmscRandomLevel(units=units)
        H.setPriors(rl, nfMin=nf, nfMax=nf)
        return {"sample": rl}
    sd = pd.DataFrame({"sample": units})
    names = ["(Intercept)"] + [f"x{k}" for k in range(1, ncN)]
    rrr = H.Hmsc(Y=Y, X=X, covNames=names, XRRR=XR, ncRRR=ncRRR, distr="probit", studyDesign=sd, ranLevels=level())
    plain = H.Hmsc(Y=Y, X=Xf, covNames=names + [f"r{k}" for k in range(ncRRR)], distr="probit", studyDesign=sd,
                   ranLevels=level())
    return rrr, plain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ny", type=int, default=10000)
    ap.add_argument("--ns", type=int, default=1000)
    ap.add_argument("--prof-sweeps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    up = {"GammaEta": False}
    hms = dict(zip(("rrr", "plain"), models(a.ny, a.ns, 20, 2, 10, 10)))
    chains, it = {}, {}
    for name, hM in hms.items():
        ch = H.Chain(hM, 20261015, device=0, updater=up)
        ch.init()
        ch.run(transient=40, samples=0, adaptNf=[0], record=False)      # warm-up; graphs captured
        ch.run(transient=0, samples=32, adaptNf=[0], iter0=40)          # ... and the recorded ones
        chains[name], it[name] = ch, 72
    rates = {k: [] for k in chains}
    for _ in range(a.reps):
        for name, ch in chains.items():
            ch.sync()
            t0 = time.perf_counter()
            ch.run(transient=0, samples=a.steps, adaptNf=[0], iter0=it[name])
            rates[name].append(a.steps / (time.perf_counter() - t0))
            it[name] += a.steps
    res = dict(shape=dict(ny=a.ny, ns=a.ns, nc=22, ncRRR=2, ncORRR=10, nf=10), steps=a.steps,
               sweeps_per_s={k: [round(v, 1) for v in r] for k, r in rates.items()})
    zbytes = a.ny * a.ns * 8
    prof = {}
    for name, ch in chains.items():
        ch.profile(True)
        for k in range(a.prof_sweeps):
            ch.sweep(it[name] + k)
        ch.sync()
        d = {}
        for pid in ("wrrr", "zl", "eta_unit", "z", "sweep"):
            ms, n = ch.profile_get(pid)
            if n:
                d[pid] = dict(us=round(1e3 * ms / n, 2), launches_per_sweep=n / a.prof_sweeps)
                if pid in ("wrrr", "zl", "eta_unit"):
                    d[pid]["TB_per_s"] = round(zbytes / (1e-3 * ms / n) / 1e12, 3)
        ch.profile(False)
        prof[name] = d
        ch.close()
    res["profile_eager"] = prof
    res["z_pass_bytes"] = zbytes
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
