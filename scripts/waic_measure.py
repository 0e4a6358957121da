"""computeWAIC on the device (hmsc_waic, waic.hip) at the headline shape, against the host loop.

    python scripts/waic_measure.py [--out profiles/waic_measure.txt] [--z-us 77.8] [--errors FILE]

Config 4 (ny = 10 000, ns = 1 000, nc = 20, nf = 10, probit), S = 200 samples recorded from a short
chain.  Reports the device call's wall time split into allocation + upload and kernels (host
clock around stream synchronisations, hmsc_debug_waic_timing), kernel A's cells/s, and the host
function's time over its first 3 samples (--host-samples) extrapolated linearly to S: its cost is
one pass over ny x ns per sample, so the extrapolation is a multiplication.

--z-us: the z kernel's live time per launch from ``bench.py`` on the same machine
(``kernels_live_us.z``), the yardstick: kernel A's per-cell work is a subset of z's and it stores
nothing per cell; the target is half z's cells/s.
--errors: the printed lines of ``pytest tests/test_gpu_waic.py -s`` (max errors against mpmath),
copied into the report."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hmsc_amd as H  # noqa: E402
from hmsc_amd import _lib as L  # noqa: E402
from hmsc_amd import post as P  # noqa: E402
from hmsc_amd.workloads import synthetic_probit  # noqa: E402


def device_call(a, ny):
    waic, site, ms = np.zeros(1), np.zeros(2 * ny), np.zeros(3)
    t0 = time.perf_counter()
    L.check(L.lib().hmsc_waic(C.byref(a), L.fptr(waic), L.fptr(site), None))
    wall = time.perf_counter() - t0
    L.check(L.lib().hmsc_debug_waic_timing(L.fptr(ms)))
    return wall, ms, float(waic[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waic_measure.txt"))
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--z-us", type=float, default=None)
    ap.add_argument("--errors", default=None)
    args = ap.parse_args()
    S = args.samples
    hM = synthetic_probit()
    ny, ns = hM.ny, hM.ns
    H.sampleMcmc(hM, samples=S, transient=20, nChains=1, seed=1, verbose=0)
    post = P.poolMcmcChains(hM.postList)
    t0 = time.perf_counter()
    a, keep, dims = P._waic_args(hM, post, 11, 0)
    t_marshal = time.perf_counter() - t0
    w2, keep2, _ = P._waic_args(hM, post[:2], 11, 0)
    device_call(w2, ny)                                        # warm-up: module load, allocator
    runs = [device_call(a, ny) for _ in range(3)]
    cells = float(S) * ny * ns
    K = hM.nc + sum(dims["nf"])
    lines = ["computeWAIC on the device (waic.hip), one MI355X: python scripts/waic_measure.py", "",
             f"config 4: ny = {ny}, ns = {ns}, nc = {hM.nc}, nf = {dims['nf']}, K = {K}, probit; S = {S} samples of a "
             f"short chain; {cells:.3g} cells",
             f"  WAIC = {runs[0][2]!r} (3 runs bit-equal: {len({r[2] for r in runs}) == 1})",
             f"  stacking the samples into the C ABI's arrays (numpy, host): {t_marshal:.3f} s",
             "  device call, wall, 3 runs: " + " / ".join(f"{r[0]:.3f}" for r in runs) + " s",
             "    allocation + upload:     " + " / ".join(f"{r[1][0]:.1f}" for r in runs) + " ms",
             "    kernel A (val):          " + " / ".join(f"{r[1][1]:.1f}" for r in runs) + " ms",
             "    kernel B + mean + copy:  " + " / ".join(f"{r[1][2]:.2f}" for r in runs) + " ms"]
    ka = float(np.median([r[1][1] for r in runs])) * 1e-3
    rate = cells / ka
    lines.append(f"  kernel A: {rate:.3e} cells/s (median run; host clock around the launches of each chunk)")
    bytes_per_sample = 8.0 * (ny * ns + ny * K + K * ns + ns + ny)
    lines.append(f"    bytes per sample: Y {8 * ny * ns / 1e6:.0f} MB re-read, operands {8 * (ny * K + K * ns + ns) / 1e6:.1f} MB, "
                 f"val {8 * ny / 1e3:.0f} kB written: {bytes_per_sample * S / ka / 1e9:.0f} GB/s")
    if args.z_us:
        zr = float(ny) * ns / (args.z_us * 1e-6)
        lines.append(f"  yardstick: z kernel live {args.z_us:.1f} us per launch on this machine = {zr:.3e} cells/s; "
                     f"kernel A reaches {rate / zr:.2f} of it (target 0.5)")
    if args.host_samples > 0:
        t0 = time.perf_counter()
        P._waic_val_host(hM, post[:args.host_samples], 11)
        th = time.perf_counter() - t0
        ext = th / args.host_samples * S
        wall = float(np.median([r[0] for r in runs]))
        lines += [f"  host loop, first {args.host_samples} samples: {th:.2f} s measured; x {S}/{args.host_samples} = {ext:.0f} s "
                  f"for the {S} samples (an extrapolation, not a measurement)",
                  f"  ratio host (extrapolated) / device wall (median): {ext / wall:.0f}x"]
    if args.errors and os.path.exists(args.errors):
        lines += ["", "max errors against mpmath (pytest tests/test_gpu_waic.py -s):"]
        with open(args.errors) as f:
            lines += ["  " + ln.strip().lstrip(".") for ln in f if "max " in ln and "bound" in ln]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
