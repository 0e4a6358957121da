"""Omega convergence diagnostics on the device (hmsc_omega_diagnostics, post.hip) at the headline
shape, against the coda route on the host.

    python scripts/omega_diag_measure.py [--out profiles/omega_diag_measure.txt] [--errors FILE]

Config 4's Omega: ns = 1000 species, nf = 10 factors, 2 chains x 1000 samples; Lambda is AR(1) over
the samples (phi = 0.6) from a seed.  Reports, as medians of three calls: the whole call (host
clock, upload and download included), the series kernel (A) and the ESS kernel (B) from device
events summed over the slabs (hmsc_debug_omega_diag_timing), and kernel A's written GB/s beside the
2.8-3.0 TB/s the project's other streaming kernels reach (README).

The existing route -- convertToCodaObject -> effectiveSize + gelman_diag -- is timed on a subset of
10^4 pairs (Omega materialised for those pairs only, the ESS on the device as effectiveSize runs
it) and extrapolated linearly to ns^2 columns; the host bytes the full route would hold are
computed, not allocated.
--errors: the printed lines of ``pytest tests/test_gpu_omega_diag.py -s``, copied into the report."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hmsc_amd as H  # noqa: E402
from hmsc_amd import _lib as L  # noqa: E402
from hmsc_amd import post as P  # noqa: E402


def ar1_lambda(m, n, ns, nf, phi, seed):
    """(m, n, ns, nf): each sample nf x ns column-major, AR(1) over the samples."""
    lam = np.zeros((m, n, ns, nf))
    for c in range(m):
        rng = np.random.default_rng(seed + c)
        for t in range(1, n):
            lam[c, t] = phi * lam[c, t - 1] + rng.standard_normal((ns, nf))
    return lam


def device_call(lam, nf, scratch=0):
    t0 = time.perf_counter()
    res = P._omega_diag_device(lam, nf, scratch_bytes=scratch)
    wall = time.perf_counter() - t0
    ms = np.zeros(3)
    L.check(L.lib().hmsc_debug_omega_diag_timing(L.fptr(ms)))
    return wall, ms, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "omega_diag_measure.txt"))
    ap.add_argument("--ns", type=int, default=1000)
    ap.add_argument("--nf", type=int, default=10)
    ap.add_argument("--chains", type=int, default=2)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--subset", type=int, default=10000)
    ap.add_argument("--errors", default=None)
    args = ap.parse_args()
    m, n, ns, nfm = args.chains, args.samples, args.ns, args.nf
    lam = ar1_lambda(m, n, ns, nfm, 0.6, seed=1)
    nf = np.full((m, n), nfm, dtype=np.int32)
    device_call(lam[:, :8, :64], nf[:, :8])                    # warm-up: module load, allocator
    runs = [device_call(lam, nf) for _ in range(3)]
    same = all(np.array_equal(a, b) for r in runs[1:] for a, b in zip(r[2][:4], runs[0][2][:4]))
    npairs = ns * (ns + 1) // 2
    slab_bytes = 8.0 * npairs * n                              # per chain, written once by A, read by B
    med = lambda k: float(np.median([r[1][k] for r in runs]))  # noqa: E731
    ka, kb = med(1), med(2)
    lines = ["Omega convergence diagnostics on the device (post.hip), one MI355X: python scripts/omega_diag_measure.py",
             "",
             f"config 4's Omega: ns = {ns}, nf = {nfm}, {m} chains x {n} samples (Lambda AR(1), phi = 0.6, seed 1); "
             f"{npairs} pairs i <= j per chain",
             f"  Lambda uploaded: {lam.nbytes / 1e6:.0f} MB; series slab: {slab_bytes / 1e9:.2f} GB per chain, "
             f"{m * slab_bytes / 1e9:.2f} GB in all, in slabs of at most 1 GiB; returned: {m * ns * ns * 28 / 1e6:.0f} MB",
             f"  three calls bit-equal: {same}",
             "  whole call, host clock, 3 runs:  " + " / ".join(f"{r[0] * 1e3:.0f}" for r in runs) + " ms"
             f" (median {float(np.median([r[0] for r in runs])) * 1e3:.0f} ms)",
             "    kernel A (series), all slabs:  " + " / ".join(f"{r[1][1]:.1f}" for r in runs) + f" ms (median {ka:.1f})",
             "    kernel B (ESS), all slabs:     " + " / ".join(f"{r[1][2]:.1f}" for r in runs) + f" ms (median {kb:.1f})",
             f"  kernel A writes {m * slab_bytes / 1e9:.2f} GB in {ka:.1f} ms = {m * slab_bytes / ka / 1e6:.0f} GB/s "
             "(the project's other streaming kernels reach 2800-3000 GB/s of HBM, README)",
             f"  kernel B: {m * npairs / kb / 1e3:.2f} M series/s; it reads the slab {m * slab_bytes / kb / 1e6:.0f} GB/s "
             "counted once (each series is passed over 5 + order.max times, from cache after the first)"]
    # the existing route on a subset of pairs
    rng = np.random.default_rng(2)
    sub = rng.choice(ns * ns, size=min(args.subset, ns * ns), replace=False)
    ii, jj = sub % ns, sub // ns
    t0 = time.perf_counter()
    coda = [np.einsum("sph,sph->sp", lam[c][:, ii, :], lam[c][:, jj, :]) for c in range(m)]
    t_mat = time.perf_counter() - t0
    H.effectiveSize([x[:, :64] for x in coda])
    t0 = time.perf_counter()
    ess = H.effectiveSize(coda)
    t_ess = time.perf_counter() - t0
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        psrf = H.gelman_diag(coda)[0]
    t_gel = time.perf_counter() - t0
    d = runs[0][2]
    de = (d[0][0] + d[0][1])[ii, jj]
    scale = ns * ns / len(sub)
    lines += ["",
              f"the coda route on {len(sub)} random entries of Omega (host, the ESS through hmsc_effective_size):",
              f"  materialise {t_mat:.2f} s + effectiveSize {t_ess:.2f} s + gelman_diag {t_gel:.2f} s = "
              f"{t_mat + t_ess + t_gel:.2f} s; x {scale:.0f} = {(t_mat + t_ess + t_gel) * scale:.0f} s for ns^2 = {ns * ns} "
              "columns (an extrapolation, not a measurement)",
              f"  host bytes of the full coda object: {8.0 * ns * ns * n / 1e9:.0f} GB per chain, "
              f"{8.0 * ns * ns * n * m / 1e9:.0f} GB for {m} chains (plus gelman_diag's stacked copy of the same size)",
              f"  ratio route (extrapolated) / device call (median wall): "
              f"{(t_mat + t_ess + t_gel) * scale / float(np.median([r[0] for r in runs])):.0f}x",
              f"  agreement on the subset: ESS max rel diff {np.max(np.abs(de - ess) / np.maximum(ess, 1e-300)):.2e}, "
              f"PSRF max rel diff {np.nanmax(np.abs(P.gelman_from_moments(d[1], d[2], n)[0][ii, jj] / psrf - 1)):.2e}"]
    if args.errors and os.path.exists(args.errors):
        lines += ["", "figures printed by pytest tests/test_gpu_omega_diag.py -s:"]
        with open(args.errors) as f:
            lines += ["  " + ln.strip().lstrip(".") for ln in f if ("worst" in ln or "AIC gap" in ln) and ": " in ln
                      and "print(" not in ln and "fake" not in ln]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
