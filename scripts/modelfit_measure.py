"""evaluateModelFit on the device (hmsc_model_fit, modelfit.hip) against the host function at the
config-4 shape, on one MI355X.

    python scripts/modelfit_measure.py [--out profiles/modelfit_measure.txt]

ny = 10 000, ns = 1 000; the summary is computePredictedValues(summary=True, expected=False) of
scripts/summary_measure.py's model and seeded posterior stacks at S = 20.  Two shapes: all probit,
and the same with the first 100 columns Poisson (Y replaced by counts) and the next 100 normal.
Per shape one warm-up of each path, then three timed rounds, host and device alternating on the same
inputs; medians.  The device call is split into the host's column-major copies of the matrices
(timed apart, the same copies), the C call (hmsc_debug_model_fit_timing: whole call, uploads,
kernels) and the rest (allocation, zero fill, the copy back, Python).  The device result is held to
the host's with the tests' assertions (AUC, O.AUC bit-equal, every other key within 1e-10)."""
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
from hmsc_amd.workloads import synthetic_probit  # noqa: E402
import modelfit_reference as MR  # noqa: E402
from summary_measure import NC, NF, NS, NY, make_post  # noqa: E402


def fit_ms():
    ms = np.zeros(3)
    L.check(L.lib().hmsc_debug_model_fit_timing(L.fptr(ms)))
    return ms


def host(hM, sm):
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        mf = H.evaluateModelFit(hM, summary=sm)
    return time.perf_counter() - t0, mf


def device(hM, sm):
    t0 = time.perf_counter()
    mf = H.evaluateModelFit(hM, summary=sm, device=0)
    return time.perf_counter() - t0, mf, fit_ms()


def layout_s(mats):
    """The column-major copies model_fit_device makes of its matrices, timed on their own."""
    t0 = time.perf_counter()
    for a in mats:
        L.colmajor_ptr(a, [])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modelfit_measure.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hM = synthetic_probit(ny=NY, ns=NS, nc=NC, nf=NF)
    hM.postList = [make_post(20)]
    med = lambda v: float(np.median(v))  # noqa: E731
    say(f"modelfit_measure: ny = {NY}, ns = {NS}; summary of computePredictedValues(summary=True, expected=False) "
        f"at S = 20; medians of three after one warm-up, host and device alternating")
    for shape in ("all probit", "100 Poisson, 100 normal, 800 probit"):
        if shape != "all probit":
            rng = np.random.default_rng(4)
            hM.distr[:100, 0] = 3
            hM.distr[100:200, 0] = 1
            Y = np.array(hM.Y, dtype=np.float64)
            Y[:, :100] = rng.poisson(np.exp(rng.normal(-0.3, 1.0, (NY, 100))))
            Y[:, 100:200] = rng.standard_normal((NY, 100))
            hM.Y = Y
        sm = H.computePredictedValues(hM, expected=False, seed=3, summary=True)
        fam = hM.distr[:, 0]
        pois = fam == 3
        nmat = 3 if pois.any() else 2
        host(hM, sm), device(hM, sm)
        th, td, tl = [], [], []
        for _ in range(3):
            h = host(hM, sm)
            d = device(hM, sm)
            th.append(h[0]), td.append((d[0],) + tuple(d[2]))
            tl.append(layout_s([np.asarray(hM.Y, dtype=np.float64)] * nmat))
        MR.assert_close_to_host(d[1], h[1], 1e-10, shape)
        worst = max(float(np.nanmax(np.abs(d[1][k] - h[1][k]))) if np.isfinite(h[1][k]).any() else 0.0 for k in h[1])
        eq = all(np.array_equal(d[1][k], h[1][k], equal_nan=True) for k in ("AUC", "O.AUC") if k in h[1])
        call, c_all, up, kn = (med([t[k] for t in td]) for k in range(4))
        mb = nmat * NY * NS * 8e-6
        say()
        say(f"{shape}")
        say(f"  host   evaluateModelFit(summary=)            {med(th):.3f} s")
        say(f"  device evaluateModelFit(summary=, device=0)  {call:.3f} s = {med(th) / call:.1f}x the host")
        say(f"    column-major copies of the {nmat} matrices (host)  {1e3 * med(tl):.1f} ms")
        say(f"    hmsc_model_fit, whole C call                 {c_all:.1f} ms")
        say(f"      uploads ({nmat} x {NY * NS * 8e-6:.0f} MB = {mb:.0f} MB)            {up:.1f} ms = {mb / up:.1f} GB/s, "
            f"{100 * up / (1e3 * call):.0f} % of the device call")
        say(f"      kernels                                    {kn:.2f} ms, {100 * kn / (1e3 * call):.1f} % of the device call")
        say(f"      allocation, zero fill, copy back           {c_all - up - kn:.1f} ms")
        say(f"    forming m and pO, the dict (Python)          {1e3 * call - c_all - 1e3 * med(tl):.1f} ms")
        say(f"  device against host: AUC / O.AUC bit-equal: {eq}; worst difference over all keys {worst:.2e}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
