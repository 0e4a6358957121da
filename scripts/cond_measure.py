"""Conditional prediction, predict(Yc, condBatch=True) (hmsc_predict_conditional, cond.hip: all
samples in one call) against condBatch=False (the per-sample loop over hmsc_set_state /
hmsc_update / hmsc_get_state), on one MI355X.

    python scripts/cond_measure.py [--out profiles/cond_measure.txt] [--z-us 77.8] [--shapes a,b]

Shape (a), a cross-validation fold: ny = 200, ns = 50, nc = 4, one level with np = ny, nf = 5,
S = 200 samples, mcmcStep = 10.  Shape (b), config 4: ny = 10 000, ns = 1 000, nc = 20, nf = 10,
S = 20, mcmcStep = 2.  Probit, the posterior of a short chain, 10 % of the species held out (their
columns of Yc are NA).  Each path: one warm-up call, then three timed calls of predict (wall, host
clock; predict ends in a device synchronisation).  The batched call's split is
hmsc_debug_cond_timing of the last call: uploads + allocation + factor launches (host clock), the Z
launches and the Eta launches (device events at the launch boundaries), the copy back.

--z-us: the z kernel's live time per launch at config 4 from ``bench.py`` (README: 77.8 us for
ny x ns = 1e7 cells), the yardstick for the Z launches of shape (b)."""
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
from hmsc_amd.workloads import synthetic_probit  # noqa: E402

SHAPES = dict(a=dict(ny=200, ns=50, nc=4, nf=5, S=200, mcmcStep=10),
              b=dict(ny=10000, ns=1000, nc=20, nf=10, S=20, mcmcStep=2))


def timed(hM, post, Yc, mcmc_step, cond_batch):
    t0 = time.perf_counter()
    pred = H.predict(hM, post=post, Yc=Yc, mcmcStep=mcmc_step, expected=True, seed=7, condBatch=cond_batch)
    return time.perf_counter() - t0, pred


def measure(name, z_us):
    sh = SHAPES[name]
    ny, ns, S, m = sh["ny"], sh["ns"], sh["S"], sh["mcmcStep"]
    hM = synthetic_probit(ny=ny, ns=ns, nc=sh["nc"], nf=sh["nf"])
    H.sampleMcmc(hM, samples=S, transient=20, nChains=1, seed=1, verbose=0)
    post = H.poolMcmcChains(hM.postList)
    held = np.arange(ns) % 10 == 9
    Yc = np.array(hM.Y, dtype=np.float64)
    Yc[:, held] = np.nan
    n_obs = float(ny) * int((~held).sum())
    res = {}
    for cb in (False, True):
        timed(hM, post[:2], Yc, m, cb)                      # warm-up: module load, allocator
        res[cb], last = [], None
        for _ in range(3):
            del last
            t, last = timed(hM, post, Yc, m, cb)
            res[cb].append(t)
            print(f"({name}) condBatch={cb}: {t:.3f} s", flush=True)
        if cb:
            ms = np.zeros(4)
            L.check(L.lib().hmsc_debug_cond_timing(L.fptr(ms)))
            diff = max(float(np.max(np.abs(a - b))) for a, b in zip(last, keep))
        else:
            keep = last
    # the conditioning step alone (predict's other work, hmsc_predict and its output, is common)
    Pm = importlib.import_module("hmsc_amd.predict")
    X = np.asarray(hM.X, dtype=np.float64)
    betas = [np.asarray(s["Beta"], dtype=np.float64) for s in post]
    step = {False: [], True: []}
    for cb in (False, True):
        for _ in range(3):
            rng = np.random.default_rng(7)
            t0 = time.perf_counter()
            if cb:
                Pm._conditional_etas_batched(hM, post, X, betas, hM.studyDesign, Yc, m, rng, 0)
            else:
                Pm._conditional_etas(hM, post, X, hM.studyDesign, Yc, m, rng, 0)
            step[cb].append(time.perf_counter() - t0)
        print(f"({name}) conditioning alone, condBatch={cb}: " + " / ".join(f"{t:.3f}" for t in step[cb]), flush=True)
    nr = hM.nr
    launches = 1 + m * (nr + 1)
    lines = [f"shape ({name}): ny = {ny}, ns = {ns}, nc = {sh['nc']}, nr = {nr}, np = ny, nf = {sh['nf']}, S = {S}, "
             f"mcmcStep = {m}, {int(held.sum())} of {ns} species held out",
             "  predict(Yc, condBatch=False), wall, 3 runs: " + " / ".join(f"{t:.3f}" for t in res[False]) + " s",
             "  predict(Yc, condBatch=True),  wall, 3 runs: " + " / ".join(f"{t:.3f}" for t in res[True]) + " s",
             f"  ratio of the medians (loop / batched): {np.median(res[False]) / np.median(res[True]):.1f}x",
             f"  max |expected value, batched - loop| over all samples: {diff:.2e}",
             "  the conditioning step alone (_conditional_etas / _conditional_etas_batched: host marshalling and "
             "device), wall, 3 runs:",
             "    per-sample loop: " + " / ".join(f"{t:.3f}" for t in step[False]) + " s;  batched: " +
             " / ".join(f"{t:.3f}" for t in step[True]) + f" s;  ratio of the medians "
             f"{np.median(step[False]) / np.median(step[True]):.1f}x",
             f"  batched call, last run (hmsc_debug_cond_timing): upload + allocation + factors {ms[0]:.2f} ms, "
             f"Z launches {ms[1]:.3f} ms ({m + 1} launches), Eta launches {ms[2]:.3f} ms ({m * nr} launches), "
             f"copy back {ms[3]:.2f} ms; {launches} launches in the loop of the one chunk",
             f"    the rest of predict's wall time is host work: the class finder, stacking the samples, "
             f"hmsc_predict and its {8e-6 * S * ny * ns:.0f} MB of output"]
    zt = ms[1] * 1e-3 / (m + 1)
    cells = S * n_obs
    zbytes = S * (8.0 * ny * ns + 8.0 * n_obs)
    lines.append(f"  one Z launch: {zt * 1e6:.1f} us for {cells:.3g} observed cells of {S} samples = {cells / zt:.3e} cells/s; "
                 f"Yc read + Z written {zbytes / 1e6:.0f} MB = {zbytes / zt / 1e9:.0f} GB/s")
    if name == "b" and z_us:
        zr = 1e7 / (z_us * 1e-6)
        lines.append(f"    yardstick: the chain's z kernel, live {z_us:.1f} us per launch at config 4 = {zr:.3e} cells/s "
                     f"(it writes 8 B per cell: {8 * zr / 1e9:.0f} GB/s of Z); a Z launch here reaches "
                     f"{cells / zt / zr:.2f} of its cell rate")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_measure.txt"))
    ap.add_argument("--z-us", type=float, default=77.8)
    ap.add_argument("--shapes", default="a,b")
    args = ap.parse_args()
    lines = ["Conditional prediction, batched (cond.hip) against the per-sample loop, one MI355X: "
             "python scripts/cond_measure.py", ""]
    for name in args.shapes.split(","):
        lines += measure(name, args.z_us) + [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
