"""Prediction maps of a GPP level (predictMap(gppDevice=True), mode 4 of hmsc_predict_map, gpp.hip) on
one MI355X.

    python scripts/gpp_measure.py [--out profiles/gpp_measure.txt] [--nn 20000,100000,1000000] [--samples 200]
                                  [--budget-s 900]

workloads.spatial_vignette4(method="GPP") at np = 5000 fitted units (ns = 5 probit species, nf = 1,
constructKnots(knotDist = 0.2, minKnotDist = 0.4)); the posterior is generated from a seed (no fit:
the cost does not depend on the values), its alpha indices uniform over the five alphapw grid points
around the generating scale 0.35; nn new sites uniform in the unit square, every row its own new
unit; predictMap(cells=False, measures=("S",), weights=one column), expected values, as
scripts/map_measure.py.

Per nn, each in a fresh process (one warm-up call, then three timed: the median):
the call's wall time, mapTiming()'s split, the slab kernel's fp64 rate 2 nn nK c / (its device time),
c = the (sample, factor) pairs = samples x nf, beside the 28-31 TFLOP/s README quotes for the map's
triangular solve; the same map with predictEtaMean=True (mode 0) for context.  Then the host path
(predictLatentFactor with device=None) at the first nn on 3 samples, scaled to all samples.
A step that would start after --budget-s seconds of this script is skipped and reported as such."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NP = 5000
README_TRSM = "28-31"


def setup(nn, S, seed=20261021):
    import pandas as pd
    import hmsc_amd as H
    from hmsc_amd.workloads import spatial_vignette4
    hM = spatial_vignette4(ny=NP, method="GPP")
    rng = np.random.default_rng(seed)
    alphas = np.asarray(hM.rL[0].alphapw, dtype=np.float64)[:, 0]
    mid = int(np.argmin(np.abs(alphas - 0.35)))
    grid = np.arange(mid - 2, mid + 3) + 1                         # 1-based grid indices
    post = [dict(Beta=rng.normal(0.0, 0.5, (hM.nc, hM.ns)), sigma=np.ones(hM.ns), Eta=[rng.standard_normal((NP, 1))],
                 Lambda=[rng.standard_normal((1, hM.ns))], Alpha=[rng.choice(grid, 1)]) for _ in range(S)]
    G = H.prepareGradient(hM, pd.DataFrame({"x1": np.zeros(nn)}), {"sample": rng.random((nn, 2))})
    X = np.column_stack([np.ones(nn), rng.standard_normal(nn)])
    w = np.sign(np.arange(hM.ns) - 2.0)
    kw = dict(post=post, X=X, studyDesign=G["studyDesignNew"], ranLevels=G["rLNew"], seed=7, expected=True)
    return H, hM, kw, w, G


def child(args):
    H, hM, kw, w, G = setup(args.nn, args.samples)
    nK = int(np.asarray(hM.rL[0]["sKnot"]).shape[0])
    if args.route == "host":
        from hmsc_amd.predict import predictLatentFactor, _levels
        post = kw["post"][:3]
        units, unitsPred = _levels(hM.dfPi["sample"]), _levels(kw["studyDesign"]["sample"])
        t0 = time.perf_counter()
        predictLatentFactor(unitsPred, units, [s["Eta"][0] for s in post], G["rLNew"]["sample"],
                            postAlpha=[s["Alpha"][0] for s in post], rng=np.random.default_rng(1))
        print("RESULT " + json.dumps(dict(wall=time.perf_counter() - t0, samples=3, nK=nK)), flush=True)
        return
    from hmsc_amd.gradient import mapTiming
    mode = dict(gppDevice=True) if args.route == "gpp" else dict(predictEtaMean=True)

    def fn():
        H.predictMap(hM, measures=("S",), weights={"w": w}, cells=False, **mode, **kw)
        return mapTiming()

    fn()
    reps = 3
    walls, phases = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        phases.append(fn())
        walls.append(time.perf_counter() - t0)
    k = int(np.argsort(walls)[len(walls) // 2])
    print("RESULT " + json.dumps(dict(wall=walls[k], reps=reps, phases=phases[k], nK=nK)), flush=True)


def spawn(route, nn, S, limit=600):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--route", route, "--nn", str(nn), "--samples", str(S)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd[2:])} ended with {p.returncode}: {p.stderr[-600:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpp_measure.txt"))
    ap.add_argument("--nn", default="20000,100000,1000000")
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--budget-s", type=float, default=900.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--route", default="gpp")
    args = ap.parse_args()
    if args.child:
        args.nn = int(args.nn)
        return child(args)
    t_start = time.perf_counter()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(args.out, "w") as f:                # kept current: a later step may be cut short
            f.write("\n".join(lines) + "\n")

    def in_budget(what):
        if time.perf_counter() - t_start < args.budget_s:
            return True
        say(f"  {what}: not measured (the script's time budget of {args.budget_s:.0f} s was used up)")
        return False

    S, nf = args.samples, 1
    sizes = [int(s) for s in args.nn.split(",")]
    say(f"gpp_measure: spatial_vignette4(method='GPP') at np = {NP} fitted units, ns = 5, nf = {nf}, {S} samples from a "
        f"seed, alpha on 5 grid points around 0.35; predictMap(cells=False), expected values, community columns S and "
        f"one weighted sum; one MI355X")
    say(f"README's rate of the map's triangular solve ('Full' predictEtaMean): {README_TRSM} TFLOP/s")
    say()
    for nn in sizes:
        for route, label in (("gpp", "gppDevice=True (mode 4)"), ("mean", "predictEtaMean=True (mode 0)")):
            what = f"nn = {nn} {label}"
            if not in_budget(what):
                continue
            r = spawn(route, nn, S)
            ph = r["phases"]
            say(f"  {what}: call {r['wall']:.3f} s (median of {r['reps']}), nK = {r['nK']}")
            say("      phases (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in ph.items()))
            if route == "gpp":
                c = S * nf
                flop = 2.0 * nn * r["nK"] * c
                say(f"      slab kernel (phase 'mean'): 2 nn nK c = {flop:.3e} flop in {ph['mean']:.2f} ms = "
                    f"{flop / ph['mean'] * 1e-9:.3f} TFLOP/s (c = {c} pairs; the knots fill {r['nK']} of the kernel's "
                    f"{-(-r['nK'] // 64) * 64} chunk columns); dDn pass (phase 'K12') {ph['K12']:.2f} ms")
    say()
    nn = sizes[0]
    if in_budget("host path"):
        h = spawn("host", nn, S, limit=900)
        say(f"host path (predictLatentFactor, device=None) at nn = {nn}: {h['wall']:.2f} s for {h['samples']} samples x "
            f"{nf} factor = {h['wall'] / h['samples']:.2f} s per sample, {h['wall'] / h['samples'] * S:.0f} s for {S} samples "
            f"(scaled; the factors alone, without predict's values and summaries)")


if __name__ == "__main__":
    main()
