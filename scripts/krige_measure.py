"""Kriging of new spatial units: the device call (hmsc_krige) against the host path
(hmsc_amd.predict._krige, unchanged since before the device path existed) on the same inputs.

    python scripts/krige_measure.py [--out profiles/krige_measure.txt]

'Full':  np = 2000 fitted units, nn = 4000 new units, S = 200 samples x nf = 4 factors, Alpha
         spread over 20 points of the default alphapw grid of the unit square.
'NNGP':  np = 5000, nn = 10000, k = 10, the same posterior shape.
The host is timed over its first 3 samples (--host-samples) and extrapolated linearly to S: its
cost is one solve / Cholesky per (sample, factor), so the extrapolation is a multiplication.
fp64 rates are against the 78.6 TFLOP/s matrix-core peak DESIGN.md section 4 uses."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hmsc_amd import _lib as L  # noqa: E402
from hmsc_amd.predict import _krige  # noqa: E402

PEAK = 78.6e12
PHASES = ["kernel matrices + gather + z", "potrf K11", "trsm [K12 | E]", "mean B'Y (+ colnorm)", "syrk W = K22 - B'B",
          "potrf W", "trmm L_W Z", "nn kernel"]


class _RL:
    """What _krige reads of a random level."""
    distMat = None

    def __init__(self, method, k=None):
        self.spatialMethod, self.nNeighbours = method, k


def inputs(npo, nn, S, nf, ngrid, seed):
    rng = np.random.default_rng(seed)
    xy = rng.random((npo + nn, 2))
    alphas = np.sqrt(2.0) * np.arange(101) / 100                      # the default grid of the unit square
    grid = np.sort(rng.choice(np.arange(5, 102), size=ngrid, replace=False))
    idx = grid[rng.integers(0, ngrid, (S, nf))].astype(np.int32)
    eta = rng.standard_normal((S, nf, npo))                            # S x (np x nf column-major)
    return xy, alphas, idx, eta


def device_call(xy, alphas, idx, eta, npo, mode, k=0, timing=False):
    S, nf = idx.shape
    nn = xy.shape[0] - npo
    keep = [np.ascontiguousarray(xy.T.ravel()), np.ascontiguousarray(alphas), np.ascontiguousarray(eta),
            np.ascontiguousarray(idx), np.zeros(8)]
    a = L.hmsc_krige_args()
    a.device, a.np, a.nn, a.sDim, a.G, a.S, a.nfmax, a.mode, a.nNeighbours, a.level = 0, npo, nn, 2, len(alphas), S, nf, mode, k, 0
    a.seed = 12345
    a.coords, a.alphas, a.Eta, a.alpha = L.fptr(keep[0]), L.fptr(keep[1]), L.fptr(keep[2]), L.iptr(keep[3])
    if timing:
        a.kernel_ms = L.fptr(keep[4])
    out = np.empty((S, nf, nn))
    t0 = time.perf_counter()
    L.check(L.lib().hmsc_krige(C.byref(a), L.fptr(out)))
    return time.perf_counter() - t0, keep[4], out


def host_time(xy, alphas, idx, eta, npo, method, k, nsamp):
    rl = _RL(method, k)
    apw = np.column_stack([alphas, np.ones_like(alphas)])
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    for s in range(nsamp):
        _krige(rl, eta[s].T, idx[s], apw, xy[:npo], xy[npo:], False, False, rng)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krige_measure.txt"))
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    S, nf, ngrid = 200, 4, 20
    lines = ["Kriging of new spatial units (krige.hip), one MI355X: python scripts/krige_measure.py", ""]

    # ---- 'Full'
    npo, nn = 2000, 4000
    xy, alphas, idx, eta = inputs(npo, nn, S, nf, ngrid, 1)
    device_call(xy[:npo + 64], alphas, idx[:2], eta[:2], npo, 2)        # warm-up: module load, allocator
    walls = [device_call(xy, alphas, idx, eta, npo, 2)[0] for _ in range(3)]
    _, ms, _ = device_call(xy, alphas, idx, eta, npo, 2, timing=True)
    groups = np.unique(idx)
    cs = [int((idx == g).sum()) for g in groups]
    fl_trsm = sum(float(npo) ** 2 * (nn + c) for c in cs)
    fl_syrk = len(groups) * float(nn) ** 2 * npo
    fl_potrf = len(groups) * float(nn) ** 3 / 3
    lines += [f"'Full': np = {npo}, nn = {nn}, S = {S}, nf = {nf}; {len(groups)} grid points in use, "
              f"{min(cs)}-{max(cs)} (sample, factor) pairs each",
              "  device call, wall (upload, kernels, download), 3 runs: " + " / ".join(f"{w:.3f}" for w in walls) + " s",
              "  per-kernel time from events, summed over the grid points (ms):"]
    lines += [f"    {PHASES[p]:32s} {ms[p]:10.2f}" for p in range(7)]
    lines += [f"    {'sum':32s} {ms[:7].sum():10.2f}",
              "  achieved fp64 rate (flops counted: trsm np^2 (nn + c), syrk nn^2 np, potrf nn^3 / 3):"]
    for name, fl, p in (("trsm", fl_trsm, 2), ("syrk", fl_syrk, 4), ("potrf W", fl_potrf, 5)):
        r = fl / (ms[p] * 1e-3)
        lines.append(f"    {name:8s} {fl / 1e9:9.1f} GFLOP  {r / 1e12:6.2f} TFLOP/s  {100 * r / PEAK:5.1f} % of 78.6")
    if not args.skip_host:
        th = host_time(xy, alphas, idx, eta, npo, "Full", None, args.host_samples)
        ext = th / args.host_samples * S
        lines += [f"  host path, first {args.host_samples} samples ({args.host_samples * nf} factors): {th:.1f} s measured; "
                  f"x {S}/{args.host_samples} = {ext:.0f} s for the {S} samples (an extrapolation, not a measurement)",
                  f"  ratio host (extrapolated) / device wall (median): {ext / np.median(walls):.0f}x"]
    lines.append("")

    # ---- 'NNGP'
    npo, nn, k = 5000, 10000, 10
    xy, alphas, idx, eta = inputs(npo, nn, S, nf, ngrid, 2)
    walls = [device_call(xy, alphas, idx, eta, npo, 3, k)[0] for _ in range(3)]
    _, ms, _ = device_call(xy, alphas, idx, eta, npo, 3, k, timing=True)
    lines += [f"'NNGP': np = {npo}, nn = {nn}, k = {k}, S = {S}, nf = {nf}; {len(np.unique(idx))} grid points in use",
              "  device call, wall, 3 runs: " + " / ".join(f"{w:.3f}" for w in walls) + " s",
              f"  krige_nn_kernel from events: {ms[7]:.2f} ms"]
    if not args.skip_host:
        th = host_time(xy, alphas, idx, eta, npo, "NNGP", k, args.host_samples)
        ext = th / args.host_samples * S
        lines += [f"  host path, first {args.host_samples} samples: {th:.1f} s measured; x {S}/{args.host_samples} = {ext:.0f} s "
                  f"(an extrapolation)",
                  f"  ratio host (extrapolated) / device wall (median): {ext / np.median(walls):.0f}x"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
