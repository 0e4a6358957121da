"""Prediction maps (predictMap, hmsc_predict_map, map.hip) against the route through hmsc_krige and
the host (predictSummary + predictCommunity with krigeDevice=True), on one MI355X.

    python scripts/map_measure.py [--out profiles/map_measure.txt] [--nn-both 20000] [--nn-map 100000,1000000]
                                  [--samples 200] [--budget-s 480]

workloads.spatial_vignette4 at ny = 5000 fitted units (ns = 5 probit species, nf = 1, 'Full'); the
posterior is generated from a seed (no fit: the cost does not depend on the values), its alpha
indices uniform over the five alphapw grid points around the generating scale 0.35, which is what a
fitted chain's alpha visits; 200 samples; nn new sites uniform in the unit square, every row its own
new unit.  predictEtaMean and predictEtaMeanField, expected values, measure "S" and the weighted sum
of the species' slopes' signs as community columns.

(a) at --nn-both: wall time and peak host RSS of both routes, each in a fresh process (one warm-up
    call, then three timed: medians; the RSS is the process' high-water mark), and the outputs
    compared for equality.
(b) predictMap alone at --nn-map with cells=False, and at the first of them with cells: wall time,
    hmsc_debug_map_timing's phases, cells/s of the summary and community kernels.
(c) the triangular solve's share of (b).
A step that would start after --budget-s seconds of this script is skipped and reported as such;
sizes of 10^6 are timed once after the warm-up."""
import argparse
import json
import os
import resource
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NP = 5000
README_SUMMARY, README_COMMUNITY = "3.6-4.1e10", "4.0-4.8e10"   # cells/s, README's status bullets


def setup(nn, S, seed=20261020):
    import pandas as pd
    import hmsc_amd as H
    from hmsc_amd.workloads import spatial_vignette4
    hM = spatial_vignette4(ny=NP)
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
    return H, hM, kw, w, alphas[grid - 1]


def run_parent(H, hM, kw, w, mode):
    c = H.predictSummary(hM, krigeDevice=True, **mode, **kw)
    m = H.predictCommunity(hM, krigeDevice=True, measures=("S",), weights={"w": w}, **mode, **kw)
    return c, m


def run_map(H, hM, kw, w, mode, cells=True):
    from hmsc_amd.gradient import mapTiming
    r = H.predictMap(hM, measures=("S",), weights={"w": w}, cells=cells, **mode, **kw)
    return r["cells"], r["community"], mapTiming()


def child(args):
    H, hM, kw, w, _ = setup(args.nn, args.samples)
    mode = {args.mode: True}
    reps = 1 if args.nn >= 10 ** 6 else 3
    fn = (lambda: run_parent(H, hM, kw, w, mode)) if args.route == "parent" else \
        (lambda: run_map(H, hM, kw, w, mode, cells=not args.no_cells))
    fn()
    walls, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
    res = dict(wall=float(np.median(walls)), reps=reps, rss_mb=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0)
    if args.route == "map":
        res["phases"] = out[2]
    if args.dump:
        np.savez(args.dump, **{f"{p}_{k}": np.asarray(v) for p, d in (("cells", out[0]), ("community", out[1]))
                               if d is not None for k, v in d.items() if k != "columns"})
    print("RESULT " + json.dumps(res), flush=True)


def spawn(route, mode, nn, S, no_cells=False, dump=None, limit=900):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--route", route, "--mode", mode, "--nn", str(nn),
           "--samples", str(S)] + (["--no-cells"] if no_cells else []) + (["--dump", dump] if dump else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd[2:])} ended with {p.returncode}: {p.stderr[-600:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_measure.txt"))
    ap.add_argument("--nn-both", type=int, default=20000)
    ap.add_argument("--nn-map", default="100000,1000000")
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--budget-s", type=float, default=480.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--route", default="map")
    ap.add_argument("--mode", default="predictEtaMean")
    ap.add_argument("--nn", type=int, default=20000)
    ap.add_argument("--no-cells", action="store_true")
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    if args.child:
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

    S, ns = args.samples, 5
    say(f"map_measure: spatial_vignette4 at np = {NP} fitted units, ns = {ns}, nf = 1, {S} samples from a seed, alpha on 5 "
        f"grid points around 0.35; expected values; community columns S and one weighted sum")
    say(f"README's rates: summary kernel {README_SUMMARY} cells/s, community kernel A {README_COMMUNITY} cells/s")
    say()
    nn = args.nn_both
    say(f"(a) both routes at nn = {nn}: fresh process each, warm-up then medians of three")
    tmp = tempfile.mkdtemp(prefix="map_measure_")
    for mode in ("predictEtaMean", "predictEtaMeanField"):
        if not in_budget(f"{mode}"):
            continue
        da, db = os.path.join(tmp, f"map_a_{mode}.npz"), os.path.join(tmp, f"map_b_{mode}.npz")
        a = spawn("parent", mode, nn, S, dump=da)
        b = spawn("map", mode, nn, S, dump=db)
        za, zb = np.load(da), np.load(db)
        same = all(np.array_equal(za[k], zb[k], equal_nan=True) for k in zb.files)
        os.remove(da), os.remove(db)
        say(f"  {mode}: predictSummary + predictCommunity (krigeDevice) {a['wall']:.3f} s, peak RSS {a['rss_mb']:.0f} MB; "
            f"predictMap {b['wall']:.3f} s, peak RSS {b['rss_mb']:.0f} MB: {a['wall'] / b['wall']:.2f}x the time, "
            f"{a['rss_mb'] / b['rss_mb']:.2f}x the memory; all outputs equal: {same}")
        say("      predictMap phases (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in b["phases"].items()))
    say()
    say("(b) predictMap alone; (c) the triangular solve's share")
    sizes = [int(s) for s in args.nn_map.split(",")]
    for mode in ("predictEtaMean", "predictEtaMeanField"):
        for nn, no_cells in [(sizes[0], False)] + [(n, True) for n in sizes]:
            what = f"{mode} nn = {nn} cells={'False' if no_cells else 'True'}"
            if not in_budget(what):
                continue
            r = spawn("map", mode, nn, S, no_cells=no_cells)
            ph = r["phases"]
            dev = sum(ph.values())
            say(f"  {what}: call {r['wall']:.2f} s ({'one run' if r['reps'] == 1 else 'median of three'}), peak RSS "
                f"{r['rss_mb']:.0f} MB")
            say("      phases (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in ph.items()))
            rates = []
            if ph["summary"] > 0:
                rates.append(f"summary kernel {S * nn * ns / ph['summary'] * 1e3:.2e} cells/s (README {README_SUMMARY})")
            rates.append(f"community kernel {S * nn * ns / ph['community'] * 1e3:.2e} cells/s (README {README_COMMUNITY})")
            say("      " + "; ".join(rates))
            say(f"      (c) trsm {ph['trsm']:.1f} ms = {ph['trsm'] / dev:.2f} of the phases' sum, {ph['trsm'] / (r['wall'] * 1e3):.2f} "
                f"of the call; {5.0 * NP * NP * nn / ph['trsm'] * 1e-9:.2f} TFLOP/s counting np^2 m per grid value in use (5)")


if __name__ == "__main__":
    main()
