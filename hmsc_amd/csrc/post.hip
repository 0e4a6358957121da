// Post-sampling statistics on the device: the per-sample loops of
// computeAssociations (R/computeAssociations.R), computeVariancePartitioning
// (R/computeVariancePartitioning.R:37-204) and coda::effectiveSize (spectrum0.ar, the ESS
// behind BASELINE's "Beta ESS/sec").  At ns = 1000 one posterior sample of Omega is 8 MB and
// X Beta 80 MB: these loops are reductions over samples of ns^2 / ny ns work each, so they run
// where the samples are small (Lambda, Beta, Gamma) and only the summaries come back.
// Every reduction is in a fixed order (samples in order, fixed lane trees): results repeat
// bit for bit.  The numpy restatements in oracle/post_oracle.py are the checkers.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/hmsc_amd.h"
#include "common.h"
#include "devmem.h"

namespace hmsc {

// ---------------------------------------------------------------------------------------
// computeAssociations: OmegaCor_s = cov2cor(Lambda_s' Lambda_s); mean over samples and
// support = mean(OmegaCor_s > 0); plus the posterior mean of Omega_s itself (getPostEstimate
// "Omega").  A 64 x 64 output tile per workgroup (16 x 16 threads, 4 x 4 outputs each); per
// sample the tile's two 64-species blocks of Lambda_s are staged in LDS.
// ---------------------------------------------------------------------------------------
constexpr int OT = 64, OF_MAX = HMSC_KCAP;

__global__ __launch_bounds__(256) void omega_assoc_kernel(int S, int ns, int nfmax, const int* nf, const double* Lam,
                                                           double* mean_cor, double* support, double* support_neg,
                                                           double* mean_omega) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* LI = smem;                // [h][species in block], h < nfmax
  double* LJ = smem + nfmax * OT;
  const int ntile = (ns + OT - 1) / OT;
  const int bi = blockIdx.x % ntile, bj = blockIdx.x / ntile;
  const int i0 = bi * OT, j0 = bj * OT, t = threadIdx.x, ti = t & 15, tj = t >> 4;
  double sc[4][4], sp[4][4], sn[4][4], so[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) sc[u][v] = sp[u][v] = sn[u][v] = so[u][v] = 0.0;
  for (int s = 0; s < S; ++s) {
    const int f = nf[s];
    const double* L = Lam + (size_t)s * nfmax * ns;
    __syncthreads();
    for (int q = t; q < f * OT; q += 256) {
      const int h = q / OT, c = q - h * OT;
      LI[q] = i0 + c < ns ? L[h + (size_t)nfmax * (i0 + c)] : 0.0;
      LJ[q] = j0 + c < ns ? L[h + (size_t)nfmax * (j0 + c)] : 0.0;
    }
    __syncthreads();
    double o[4][4], di[4], dj[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      di[u] = dj[u] = 0.0;
#pragma unroll
      for (int v = 0; v < 4; ++v) o[u][v] = 0.0;
    }
    for (int h = 0; h < f; ++h) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = LI[h * OT + ti + 16 * u];
        b[u] = LJ[h * OT + tj + 16 * u];
        di[u] = fma(a[u], a[u], di[u]);
        dj[u] = fma(b[u], b[u], dj[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) o[u][v] = fma(a[u], b[v], o[u][v]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        // cov2cor (its diagonal set to exactly 1, as R's)
        const double c = i0 + ti + 16 * u == j0 + tj + 16 * v ? 1.0 : o[u][v] / sqrt(di[u] * dj[v]);
        sc[u][v] += c;
        sp[u][v] += c > 0.0 ? 1.0 : 0.0;
        sn[u][v] += o[u][v] < 0.0 ? 1.0 : 0.0;
        so[u][v] += o[u][v];
      }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + ti + 16 * u, j = j0 + tj + 16 * v;
      if (i < ns && j < ns) {
        const size_t o = i + (size_t)ns * j;
        mean_cor[o] = sc[u][v] / S;
        support[o] = sp[u][v] / S;
        support_neg[o] = sn[u][v] / S;
        mean_omega[o] = so[u][v] / S;
      }
    }
}

// ---------------------------------------------------------------------------------------
// computeVariancePartitioning, one workgroup per posterior sample s:
//   mu = Gamma Tr' (nc x ns), R2T.Beta[k] += cor(Beta[k,], mu[k,])^2            (:126-128)
//   a = X mu, f = X Beta, rows centred over species; res1 = sum_i (a_i . f_i / (ns-1))^2,
//   res2 = sum_i |a_i|^2 |f_i|^2 / (ns-1)^2, R2T.Y += res1 / res2                (:133-141)
// With Mc, Bc the rows of mu, Beta centred over species, a_i - mean = x_i Mc and
// f_i - mean = x_i Bc exactly, so a_i . f_i = x_i (Mc Bc') x_i': three nc x nc Gram matrices
// replace the two ny x ns products (ny nc^2 instead of ny ns nc work; their diagonals are
// the sums of R2T.Beta's correlations).
//   fixed1[j] = Beta_j' cM Beta_j, fixedsplit1[j, g] over the group's rows / columns,
//   random1[j, r] = sum_h Lambda_r[h, j]^2, then the per-sample normalisations   (:142-173)
// The sample's terms go to a per-sample slot; vp_reduce_kernel adds them in sample order.
// ---------------------------------------------------------------------------------------
constexpr int VP_NC = HMSC_KCAP;
constexpr size_t VP_LDS_MAX = 150 * 1024;  // the three Gram matrices in LDS up to here, else global

struct VpArgs {
  int ny, ns, nc, nt, S, ngroups, nr;
  const int* group;      // nc, 1-based
  const double* X;       // ny x nc
  const double* Tr;      // ns x nt
  const double* cM;      // nc x nc
  const double* Beta;    // S x nc x ns
  const double* Gamma;   // S x nc x nt
  const int* nf;         // nr x S
  int nfmax[HMSC_MAX_LEVELS];
  const double* Lambda[HMSC_MAX_LEVELS];  // S x nfmax_r x ns
  double* work;          // S x slot
  size_t slot;           // doubles per sample: nc + 1 + ns (1 + nr + ngroups)
  double* gram;          // S x 3 nc^2 when they do not fit LDS (nc > 80), else null
};

__global__ __launch_bounds__(256) void vp_sample_kernel(VpArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ double mB[VP_NC], mM[VP_NC], red[8];
  const int s = blockIdx.x, t = threadIdx.x, nc = a.nc, ns = a.ns, nt = a.nt;
  double* Cb = a.gram ? a.gram + (size_t)s * 3 * nc * nc : smem;
  double* C[3] = {Cb, Cb + (size_t)nc * nc, Cb + (size_t)2 * nc * nc};  // Mc Bc', Mc Mc', Bc Bc'

  const double* B = a.Beta + (size_t)s * nc * ns;
  const double* G = a.Gamma + (size_t)s * nc * nt;
  double* out = a.work + (size_t)s * a.slot;
  auto mu = [&](int k, int j) {
    double v = 0.0;
    for (int q = 0; q < nt; ++q) v = fma(G[k + (size_t)nc * q], a.Tr[j + (size_t)ns * q], v);
    return v;
  };
  // row means over species
  for (int k = t; k < nc; k += 256) {
    double sb = 0.0, sm = 0.0;
    for (int j = 0; j < ns; ++j) sb += B[k + (size_t)nc * j], sm += mu(k, j);
    mB[k] = sb / ns;
    mM[k] = sm / ns;
  }
  __syncthreads();
  for (int p = t; p < nc * nc; p += 256) {
    const int k = p % nc, l = p / nc;
    double caf = 0.0, caa = 0.0, cff = 0.0;
    for (int j = 0; j < ns; ++j) {
      const double mk = mu(k, j) - mM[k], ml = mu(l, j) - mM[l];
      const double bk = B[k + (size_t)nc * j] - mB[k], bl = B[l + (size_t)nc * j] - mB[l];
      caf = fma(mk, bl, caf);
      caa = fma(mk, ml, caa);
      cff = fma(bk, bl, cff);
    }
    C[0][p] = caf;
    C[1][p] = caa;
    C[2][p] = cff;
  }
  __syncthreads();
  for (int k = t; k < nc; k += 256)  // cor(Beta[k,], mu[k,])^2
    out[k] = C[0][k + nc * k] * C[0][k + nc * k] / (C[2][k + nc * k] * C[1][k + nc * k]);
  // per-site quadratic forms (sites strided over the threads, fixed order per thread)
  const double dn = 1.0 / (ns - 1);
  double r1 = 0.0, r2 = 0.0;
  for (int i = t; i < a.ny; i += 256) {
    double qaf = 0.0, qaa = 0.0, qff = 0.0;
    for (int l = 0; l < nc; ++l) {
      const double xl = a.X[i + (size_t)a.ny * l];
      double uaf = 0.0, uaa = 0.0, uff = 0.0;
      for (int k = 0; k < nc; ++k) {
        const double xk = a.X[i + (size_t)a.ny * k];
        uaf = fma(xk, C[0][k + nc * l], uaf);
        uaa = fma(xk, C[1][k + nc * l], uaa);
        uff = fma(xk, C[2][k + nc * l], uff);
      }
      qaf = fma(uaf, xl, qaf);
      qaa = fma(uaa, xl, qaa);
      qff = fma(uff, xl, qff);
    }
    qaf *= dn, qaa *= dn, qff *= dn;
    r1 = fma(qaf, qaf, r1);
    r2 = fma(qaa, qff, r2);
  }
  for (int o = 32; o > 0; o >>= 1) r1 += __shfl_xor(r1, o), r2 += __shfl_xor(r2, o);
  if ((t & 63) == 0) red[t >> 6] = r1, red[4 + (t >> 6)] = r2;
  __syncthreads();
  if (t == 0) out[nc] = ((red[0] + red[1]) + (red[2] + red[3])) / ((red[4] + red[5]) + (red[6] + red[7]));
  // species terms
  double* fx = out + nc + 1;            // ns
  double* rnd = fx + ns;                // nr x ns
  double* fsp = rnd + (size_t)a.nr * ns;  // ngroups x ns
  for (int j = t; j < ns; j += 256) {
    const double* b = B + (size_t)nc * j;
    double f1 = 0.0;
    for (int l = 0; l < nc; ++l) {
      double u = 0.0;
      for (int k = 0; k < nc; ++k) u = fma(a.cM[k + (size_t)nc * l], b[k], u);
      f1 = fma(u, b[l], f1);
    }
    double fsum = 0.0;
    for (int g = 1; g <= a.ngroups; ++g) {  // Beta[sel, j]' cM[sel, sel] Beta[sel, j]
      double fg = 0.0;
      for (int l = 0; l < nc; ++l) {
        if (a.group[l] != g) continue;
        double u = 0.0;
        for (int k = 0; k < nc; ++k)
          if (a.group[k] == g) u = fma(a.cM[k + (size_t)nc * l], b[k], u);
        fg = fma(u, b[l], fg);
      }
      fsp[(size_t)(g - 1) * ns + j] = fg;
      fsum += fg;
    }
    for (int g = 0; g < a.ngroups; ++g) fsp[(size_t)g * ns + j] /= fsum;
    double tot = f1;
    for (int r = 0; r < a.nr; ++r) {
      const int f = a.nf[r * a.S + s];
      const double* lam = a.Lambda[r] + (size_t)s * a.nfmax[r] * ns + (size_t)a.nfmax[r] * j;
      double v = 0.0;
      for (int h = 0; h < f; ++h) v = fma(lam[h], lam[h], v);
      rnd[(size_t)r * ns + j] = v;
      tot += v;
    }
    fx[j] = a.nr > 0 ? f1 / tot : 1.0;
    for (int r = 0; r < a.nr; ++r) rnd[(size_t)r * ns + j] /= tot;
  }
}

// sum over samples in order, divided by S; out: [R2T.Beta (nc) | R2T.Y | fixed (ns) |
// random (nr x ns) | fixedsplit (ngroups x ns)]
__global__ __launch_bounds__(256) void vp_reduce_kernel(const double* work, size_t slot, int S, double* out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= slot) return;
  double v = 0.0;
  for (int s = 0; s < S; ++s) v += work[(size_t)s * slot + e];
  out[e] = v / S;
}

// ---------------------------------------------------------------------------------------
// coda::effectiveSize = n var(x) / spectrum0.ar(x)$spec per column (one wave per column):
// linear-trend residual check, autocovariances to order.max = min(n - 1, 10 log10 n),
// Levinson-Durbin (R's eureka), AIC order choice, var.pred / (1 - sum ar)^2.
// ---------------------------------------------------------------------------------------
constexpr int ESS_OMAX = 64;

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// x: n x p on the device, a column's n values contiguous.  mean_out / var_out (may be null):
// the column's mean and sxx / (n - 1), which the ESS is made of.
__global__ __launch_bounds__(256) void ess_kernel(int n, int p, const double* x, double* ess, int* order_out,
                                                  double* mean_out, double* var_out) {
  __shared__ double rr[4][ESS_OMAX + 1];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = blockIdx.x * 4 + w;
  if (col >= p) return;  // whole waves exit together: no workgroup barrier below
  const double* c = x + (size_t)n * col;
  double s = 0.0, amax = 0.0;
  for (int i = lane; i < n; i += 64) s += c[i], amax = fmax(amax, fabs(c[i]));
  const double mean = wave_sum(s) / n;
  for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
  const double zm = 0.5 * (n + 1);
  double szx = 0.0, szz = 0.0, sxx = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double zc = (i + 1) - zm, xc = c[i] - mean;
    szx = fma(zc, xc, szx);
    szz = fma(zc, zc, szz);
    sxx = fma(xc, xc, sxx);
  }
  szx = wave_sum(szx), szz = wave_sum(szz), sxx = wave_sum(sxx);
  const double beta = szx / szz;
  double srr = 0.0, srm = 0.0;
  for (int i = lane; i < n; i += 64) srm += (c[i] - mean) - ((i + 1) - zm) * beta;
  srm = wave_sum(srm) / n;
  for (int i = lane; i < n; i += 64) {
    const double rsd = (c[i] - mean) - ((i + 1) - zm) * beta - srm;
    srr = fma(rsd, rsd, srr);
  }
  srr = wave_sum(srr);
  const bool constant = sqrt(srr / (n - 1)) <= 1.5e-8 * fmax(amax, 1e-300);
  const int omax = min(min(n - 1, (int)floor(10.0 * log10((double)n))), ESS_OMAX);
  for (int k = 0; k <= omax; ++k) {
    double v = 0.0;
    for (int i = lane; i + k < n; i += 64) v = fma(c[i] - mean, c[i + k] - mean, v);
    v = wave_sum(v);
    if (lane == 0) rr[w][k] = v / n;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane != 0) return;
  const double* r = rr[w];
  const double r0 = r[0] > 0.0 ? r[0] : 1.0;
  double a[ESS_OMAX + 1], an[ESS_OMAX + 1], asum[ESS_OMAX + 1], vars[ESS_OMAX + 1];
  for (int m = 0; m <= omax; ++m) a[m] = 0.0;
  double v = r0;
  vars[0] = r0;
  asum[0] = 0.0;
  for (int m = 1; m <= omax; ++m) {
    double acc = r[m];
    for (int j = 1; j < m; ++j) acc -= a[j] * r[m - j];
    const double k = acc / v;
    for (int j = 1; j < m; ++j) an[j] = a[j] - k * a[m - j];
    for (int j = 1; j < m; ++j) a[j] = an[j];
    a[m] = k;
    v = v * (1.0 - k * k);
    vars[m] = v;
    double sm = 0.0;
    for (int j = 1; j <= m; ++j) sm += a[j];
    asum[m] = sm;
  }
  // order = which.min(xaic) as numpy's argmin: the first NaN if any, else the first minimum
  int order = 0;
  double best = INFINITY;
  bool seen_val = false;
  for (int m = 0; m <= omax; ++m) {
    const double xa = n * log(vars[m]) + 2.0 * m + 2.0;
    if (xa != xa) {
      order = m;
      break;
    }
    if (!seen_val || xa < best) best = xa, order = m, seen_val = true;
  }
  const double var_pred = vars[order] * n / (n - (order + 1));
  const double spec = constant ? 0.0 : var_pred / ((1.0 - asum[order]) * (1.0 - asum[order]));
  const double var = sxx / (n - 1);
  ess[col] = spec == 0.0 ? 0.0 : n * var / spec;
  if (order_out) order_out[col] = order;
  if (mean_out) mean_out[col] = mean;
  if (var_out) var_out[col] = var;
}

// ---------------------------------------------------------------------------------------
// Convergence diagnostics of Omega = Lambda' Lambda (coda::effectiveSize and gelman.diag on
// convertToCodaObject(m)$Omega[[r]]) without the ns^2 x samples coda matrix: the series
// w_ij(s) = sum_{h < nf_s} lambda_hi lambda_hj (one fma chain in ascending h) of the pairs
// i <= j are formed into a device slab, pair-major (a pair's n samples contiguous, canonical
// pair p = i + j (j + 1) / 2), and ess_kernel runs on the slab's columns.
//
// omega_series_kernel: a workgroup takes a 16 x 16 tile of pairs (one per thread) and a
// segment of the samples.  Lambda_s' two 16-species blocks are staged in LDS for sg samples at
// a time (read from global along h, the contiguous index); the outputs of QC = 32 samples are
// collected in LDS [pair][sample] and written out sample-fastest: 32 lanes x 8 B = one 256 B run
// per pair, where a direct store would scatter every thread's values n * 8 B apart.  Row
// strides are odd (QC + 1, QT + 1 doubles) so neither the column-wise writes nor the row-wise
// reads of the transposes pile on one bank.
// ---------------------------------------------------------------------------------------
constexpr int QT = 16, QTP = QT + 1, QC = 32, QLD = QC + 1, QSTAGE = 2048;

__global__ __launch_bounds__(256) void omega_series_kernel(int n, int ns, int nfmax, int sg, int j0, int j1,
                                                            const int* nf, const double* Lam, double* slab) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ long long pbase[QT * QT];  // the pair's offset in the slab, -1: no pair of this slab
  double* OUT = smem;                   // [pair][sample of the chunk], stride QLD
  double* LI = smem + QT * QT * QLD;    // [sample of the stage][h][species in block], stride QTP
  double* LJ = LI + (size_t)sg * nfmax * QTP;
  const int t = threadIdx.x, ti = t & (QT - 1), tj = t / QT;
  const int it0 = blockIdx.x * QT, jt0 = j0 + blockIdx.y * QT;
  if (it0 > min(jt0 + QT, j1) - 1) return;  // a tile above the diagonal: the whole workgroup leaves
  {
    const int i = it0 + ti, j = jt0 + tj;
    const size_t p0 = (size_t)j0 * (j0 + 1) / 2;
    pbase[t] = i <= j && j < j1 ? (long long)(((size_t)i + (size_t)j * (j + 1) / 2 - p0) * n) : -1;
  }
  const int nchunk = (n + QC - 1) / QC;
  const int c0 = (int)((long long)nchunk * blockIdx.z / gridDim.z);
  const int c1 = (int)((long long)nchunk * (blockIdx.z + 1) / gridDim.z);
  const int blk = nfmax * QT;
  for (int ch = c0; ch < c1; ++ch) {
    const int s0 = ch * QC, cnt = min(QC, n - s0);
    for (int g0 = 0; g0 < cnt; g0 += sg) {
      const int gn = min(sg, cnt - g0);
      __syncthreads();  // the stage's (and, at g0 = 0, the flush's) readers are done
      for (int q = t; q < gn * blk; q += 256) {
        const int g = q / blk, r = q - g * blk, c = r / nfmax, h = r - c * nfmax;
        const double* L = Lam + (size_t)(s0 + g0 + g) * nfmax * ns;
        const int o = (g * nfmax + h) * QTP + c;
        LI[o] = it0 + c < ns ? L[h + (size_t)nfmax * (it0 + c)] : 0.0;
        LJ[o] = jt0 + c < ns ? L[h + (size_t)nfmax * (jt0 + c)] : 0.0;
      }
      __syncthreads();
      for (int g = 0; g < gn; ++g) {
        const int f = nf[s0 + g0 + g];
        const double *a = LI + (size_t)g * nfmax * QTP + ti, *b = LJ + (size_t)g * nfmax * QTP + tj;
        double o = 0.0;
        for (int h = 0; h < f; ++h) o = fma(a[h * QTP], b[h * QTP], o);
        OUT[t * QLD + g0 + g] = o;
      }
    }
    __syncthreads();
    for (int q = t; q < QT * QT * QC; q += 256) {
      const int pl = q / QC, c = q - pl * QC;
      const long long b = pbase[pl];
      if (b >= 0 && c < cnt) slab[(size_t)b + s0 + c] = OUT[pl * QLD + c];
    }
  }
}

// a slab's per-pair results to (i, j) and (j, i) of the ns x ns outputs; one thread per (i, j)
// of the slab's columns j0 <= j < j1
__global__ __launch_bounds__(256) void omega_scatter_kernel(int ns, int j0, int j1, const double* e, const double* m,
                                                             const double* v, const int* o, double* ess, double* mean,
                                                             double* var, int* order) {
  const int i = blockIdx.x * 256 + threadIdx.x, j = j0 + blockIdx.y;
  if (i > j || j >= j1) return;
  const size_t q = (size_t)i + (size_t)j * (j + 1) / 2 - (size_t)j0 * (j0 + 1) / 2;
  const size_t a = i + (size_t)ns * j, b = j + (size_t)ns * i;
  ess[a] = ess[b] = e[q];
  mean[a] = mean[b] = m[q];
  var[a] = var[b] = v[q];
  order[a] = order[b] = o[q];
}

// host sides: uploads, launches and downloads on one stream of an owner that drains it and
// frees everything on every exit; the caller's current device is restored
void post_omega(int device, int S, int ns, int nfmax, const int* nf, const double* Lambda, double* mean_cor,
                double* support, double* support_neg, double* mean_omega) {
  HMSC_REQUIRE(S > 0 && ns > 0 && nfmax > 0 && nfmax <= OF_MAX && nf && Lambda && mean_cor && support && support_neg &&
                   mean_omega,
               "hmsc_post_omega: bad arguments (nfmax <= 128)");
  for (int s = 0; s < S; ++s) HMSC_REQUIRE(nf[s] >= 1 && nf[s] <= nfmax, "hmsc_post_omega: nf out of range");
  DeviceGuard dg(device);
  DeviceOwner b;
  const hipStream_t st = b.stream();
  const size_t n2 = (size_t)ns * ns;
  const int* dnf = b.upload(nf, S, st);
  const double* dL = b.upload(Lambda, (size_t)S * nfmax * ns, st);
  double *mc = b.alloc<double>(n2), *sp = b.alloc<double>(n2), *sn = b.alloc<double>(n2), *mo = b.alloc<double>(n2);
  const int nt = (ns + OT - 1) / OT;
  omega_assoc_kernel<<<nt * nt, 256, (size_t)2 * nfmax * OT * sizeof(double), st>>>(S, ns, nfmax, dnf, dL, mc, sp, sn,
                                                                                     mo);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(mean_cor, mc, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(support, sp, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(support_neg, sn, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(mean_omega, mo, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}

void post_vp(const hmsc_vp_args* v, double* out) {
  HMSC_REQUIRE(v && out && v->ny > 1 && v->ns > 1 && v->nc >= 1 && v->nc <= VP_NC && v->nt >= 1 && v->S >= 1 &&
                   v->ngroups >= 1 && v->ngroups <= VP_NC && v->nr >= 0 && v->nr <= HMSC_MAX_LEVELS,
               "hmsc_variance_partitioning: bad dimensions (nc, ngroups <= 128)");
  for (int k = 0; k < v->nc; ++k)
    HMSC_REQUIRE(v->group[k] >= 1 && v->group[k] <= v->ngroups, "hmsc_variance_partitioning: group out of range");
  DeviceGuard dg(v->device);
  DeviceOwner b;
  const hipStream_t st = b.stream();
  VpArgs a{};
  a.ny = v->ny, a.ns = v->ns, a.nc = v->nc, a.nt = v->nt, a.S = v->S, a.ngroups = v->ngroups, a.nr = v->nr;
  a.group = b.upload(v->group, a.nc, st);
  a.X = b.upload(v->X, (size_t)a.ny * a.nc, st);
  a.Tr = b.upload(v->Tr, (size_t)a.ns * a.nt, st);
  a.cM = b.upload(v->cM, (size_t)a.nc * a.nc, st);
  a.Beta = b.upload(v->Beta, (size_t)a.S * a.nc * a.ns, st);
  a.Gamma = b.upload(v->Gamma, (size_t)a.S * a.nc * a.nt, st);
  a.nf = b.upload(v->nf, (size_t)std::max(1, a.nr) * a.S, st);
  for (int r = 0; r < a.nr; ++r) {
    a.nfmax[r] = v->nfmax[r];
    a.Lambda[r] = b.upload(v->Lambda[r], (size_t)a.S * v->nfmax[r] * a.ns, st);
  }
  a.slot = (size_t)a.nc + 1 + (size_t)a.ns * (1 + a.nr + a.ngroups);
  a.work = b.alloc<double>(a.slot * a.S);
  const size_t gram_bytes = (size_t)3 * a.nc * a.nc * sizeof(double);
  a.gram = gram_bytes > VP_LDS_MAX ? b.alloc<double>((size_t)a.S * 3 * a.nc * a.nc) : nullptr;
  vp_sample_kernel<<<a.S, 256, a.gram ? 0 : gram_bytes, st>>>(a);
  double* dout = b.alloc<double>(a.slot);
  vp_reduce_kernel<<<(unsigned)((a.slot + 255) / 256), 256, 0, st>>>(a.work, a.slot, a.S, dout);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(out, dout, a.slot * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}

void post_ess(int device, int n, int p, const double* x, double* ess, int* order) {
  HMSC_REQUIRE(n >= 3 && p >= 1 && x && ess, "hmsc_effective_size: bad arguments (n >= 3)");
  DeviceGuard dg(device);
  DeviceOwner b;
  const hipStream_t st = b.stream();
  const double* dx = b.upload(x, (size_t)n * p, st);
  double* de = b.alloc<double>(p);
  int* dord = b.alloc<int>(p);
  ess_kernel<<<(p + 3) / 4, 256, 0, st>>>(n, p, dx, de, dord, nullptr, nullptr);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(ess, de, (size_t)p * sizeof(double), hipMemcpyDeviceToHost, st));
  if (order) HIP_OK(hipMemcpyAsync(order, dord, (size_t)p * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}

// whole call (host clock), series kernel, ess kernel (device events, summed over the slabs;
// -1 when the call had more slabs than are timed) of this thread's last post_omega_diag, ms
static thread_local double g_omega_diag_ms[3] = {0.0, 0.0, 0.0};
void omega_diag_last_timing(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_omega_diag_ms[k];
}

void post_omega_diag(int device, int nchains, int n, int ns, int nfmax, const int* nf, const double* Lambda,
                     uint64_t scratch_bytes, double* ess, double* mean, double* var, int* order, double* series) {
  const auto t_start = std::chrono::steady_clock::now();
  HMSC_REQUIRE(nchains > 0 && ns > 0 && ns <= 65535 && nfmax > 0 && nf && Lambda && ess && mean && var,
               "hmsc_omega_diagnostics: bad arguments (nchains, ns, nfmax positive, ns <= 65535, no NULL but order / series)");
  HMSC_REQUIRE(n >= 3, "hmsc_omega_diagnostics: n = " + std::to_string(n) + " samples per chain, at least 3 are needed");
  HMSC_REQUIRE(nfmax <= OF_MAX, "hmsc_omega_diagnostics: nfmax = " + std::to_string(nfmax) + " exceeds HMSC_KCAP = " +
                                    std::to_string(OF_MAX));
  for (size_t s = 0; s < (size_t)nchains * n; ++s)
    HMSC_REQUIRE(nf[s] >= 1 && nf[s] <= nfmax, "hmsc_omega_diagnostics: nf = " + std::to_string(nf[s]) + " of sample " +
                                                   std::to_string(s % n) + " of chain " + std::to_string(s / n) +
                                                   " is outside 1..nfmax = " + std::to_string(nfmax));
  const size_t npairs = (size_t)ns * (ns + 1) / 2, n2 = (size_t)ns * ns;
  HMSC_REQUIRE(!series || (double)nchains * (double)npairs * n <= 268435456.0,
               "hmsc_omega_diagnostics: the debug output series is limited to 2^28 doubles");
  // slabs of whole species columns j (j + 1 pairs each) within scratch_bytes
  const uint64_t scratch = scratch_bytes ? scratch_bytes : (uint64_t)1 << 30;
  const size_t pair_bytes = (size_t)n * sizeof(double), cap = scratch / pair_bytes;
  HMSC_REQUIRE(cap >= (size_t)ns, "hmsc_omega_diagnostics: scratch_bytes = " + std::to_string(scratch) +
                                      " is too small for one species column's pairs (ns = " + std::to_string(ns) +
                                      " series of n = " + std::to_string(n) + " doubles: " +
                                      std::to_string((size_t)ns * pair_bytes) + " bytes)");
  std::vector<int> cut{0};  // slab k: columns cut[k] .. cut[k + 1]
  size_t slab_pairs = 0;
  for (int j = 0; j < ns;) {
    size_t have = 0;
    while (j < ns && have + j + 1 <= cap) have += ++j;
    slab_pairs = std::max(slab_pairs, have);
    cut.push_back(j);
  }
  const int nslab = (int)cut.size() - 1;
  DeviceGuard dg(device);
  const size_t lam_n = (size_t)n * nfmax * ns;
  const size_t need = lam_n * sizeof(double) + (size_t)nchains * n * sizeof(int) + slab_pairs * pair_bytes +
                      (slab_pairs + n2) * (3 * sizeof(double) + sizeof(int));
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  HMSC_REQUIRE(need <= free_b, "hmsc_omega_diagnostics: the call needs " + std::to_string(need) +
                                   " bytes of device memory (ns = " + std::to_string(ns) + ", n = " + std::to_string(n) +
                                   ", slab = " + std::to_string(slab_pairs * pair_bytes) + "), the device has " +
                                   std::to_string(free_b) + " bytes free");
  DeviceOwner b;
  const hipStream_t st = b.stream();
  const int* dnf = b.upload(nf, (size_t)nchains * n, st);
  double* dL = b.alloc<double>(lam_n);
  double* slab = b.alloc<double>(slab_pairs * n);
  double *se = b.alloc<double>(slab_pairs), *sm = b.alloc<double>(slab_pairs), *sv = b.alloc<double>(slab_pairs);
  int* so = b.alloc<int>(slab_pairs);
  double *de = b.alloc<double>(n2), *dm = b.alloc<double>(n2), *dv = b.alloc<double>(n2);
  int* dord = b.alloc<int>(n2);
  constexpr int TIMED_SLABS = 256;
  const bool timed = (size_t)nchains * nslab <= TIMED_SLABS;
  std::vector<hipEvent_t> ev;
  if (timed)
    for (int k = 0; k < 3 * nchains * nslab; ++k) ev.push_back(b.event());
  const int sg = std::max(1, std::min(QC, QSTAGE / (nfmax * QT)));
  const size_t lds = ((size_t)QT * QT * QLD + (size_t)2 * sg * nfmax * QTP) * sizeof(double);
  const int nchunk = (n + QC - 1) / QC;
  for (int c = 0; c < nchains; ++c) {
    HIP_OK(hipMemcpyAsync(dL, Lambda + (size_t)c * lam_n, lam_n * sizeof(double), hipMemcpyHostToDevice, st));
    for (int k = 0; k < nslab; ++k) {
      const int j0 = cut[k], j1 = cut[k + 1];
      const size_t p0 = (size_t)j0 * (j0 + 1) / 2, np_k = (size_t)j1 * (j1 + 1) / 2 - p0;
      // sample segments per tile: enough workgroups to fill the device when the slab has few tiles
      const unsigned gx = (j1 + QT - 1) / QT, gy = (j1 - j0 + QT - 1) / QT;
      const unsigned gz = (unsigned)std::max<size_t>(1, std::min<size_t>(nchunk, 4096 / ((size_t)gx * gy + 1)));
      hipEvent_t* e = timed ? &ev[3 * ((size_t)c * nslab + k)] : nullptr;
      if (e) HIP_OK(hipEventRecord(e[0], st));
      omega_series_kernel<<<dim3(gx, gy, gz), 256, lds, st>>>(n, ns, nfmax, sg, j0, j1, dnf + (size_t)c * n, dL, slab);
      if (e) HIP_OK(hipEventRecord(e[1], st));
      ess_kernel<<<(unsigned)((np_k + 3) / 4), 256, 0, st>>>(n, (int)np_k, slab, se, so, sm, sv);
      if (e) HIP_OK(hipEventRecord(e[2], st));
      omega_scatter_kernel<<<dim3((j1 + 255) / 256, j1 - j0), 256, 0, st>>>(ns, j0, j1, se, sm, sv, so, de, dm, dv, dord);
      HIP_OK(hipGetLastError());
      if (series)
        HIP_OK(hipMemcpyAsync(series + ((size_t)c * npairs + p0) * n, slab, np_k * pair_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipMemcpyAsync(ess + c * n2, de, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(mean + c * n2, dm, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(var + c * n2, dv, n2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (order) HIP_OK(hipMemcpyAsync(order + c * n2, dord, n2 * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  double ka = timed ? 0.0 : -1.0, kb = ka;
  for (size_t k = 0; timed && k + 2 < ev.size(); k += 3) {
    float a_ms = 0.f, b_ms = 0.f;
    HIP_OK(hipEventElapsedTime(&a_ms, ev[k], ev[k + 1]));
    HIP_OK(hipEventElapsedTime(&b_ms, ev[k + 1], ev[k + 2]));
    ka += a_ms, kb += b_ms;
  }
  g_omega_diag_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  g_omega_diag_ms[1] = ka, g_omega_diag_ms[2] = kb;
}

}  // namespace hmsc
