// computeWAIC on the device (R/computeWAIC.R:25-131; hmsc_waic in include/hmsc_amd.h).
//
// Kernel A (waic_val_kernel): val[s, i] = sum_j log p(y_ij | sample s), the cell terms as
// hmsc_amd/post.py::computeWAIC forms them.  A workgroup takes one sample and 64 sites (16 per
// wave) and walks all species itself in stages of 32, so a site's species sum has one fixed
// order: per lane over its species (16 apart), then a fixed xor tree over the 16 lanes of a site
// group.  No atomics, and nothing depends on which samples share a launch.
//   E = [X | Eta_r[Pi_r,]] [Beta; Lambda_r] on v_mfma_f64_16x16x4: a lane keeps its A operands
//   (one site row, every fourth k) in registers for the whole walk; the K x 32 coefficient block
//   of a stage is staged in LDS by the workgroup (contiguous in Beta / Lambda) and read as the B
//   operand with a row stride = 2 mod 32 doubles (conflict free).  MFMA row m of a wave is site
//   4 (m & 3) + (m >> 2), so that the four accumulators of a lane are four consecutive sites.
// Kernel B (waic_site_kernel): per site over samples in sample order, Bl = -(m + log mean exp(val
// - m)), m = max val, and the two-pass ddof = 1 variance.  waic_mean_kernel: mean(Bl + V) by one
// workgroup, strided partial sums then a fixed tree.
//
// The reference exponentiates val and the Poisson cell likelihoods unshifted (:111-112, :124) and
// overflows to Inf / -Inf for large ns; the shifted sums here equal the literal form to rounding
// wherever that is finite.
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/hmsc_amd.h"
#include "common.h"
#include "devmem.h"
#include "waic_math.h"
#include "z_kernel.h"  // d4, mfma_f64

namespace hmsc {

constexpr int WT_I = 64, WT_J = 32, WAIC_GH_MAX = 256;

struct WaicArgs {
  int ny, ns, nc, nr, K, ghN, cN, LD;
  int np[HMSC_MAX_LEVELS], nf[HMSC_MAX_LEVELS];
  const double* Y;       // ny x ns
  const double* X;       // ny x nc
  const int* family;     // ns
  const int* prank;      // ns: rank of a Poisson column among the Poisson columns, else -1
  const int* Pi;         // ny x nr, 0-based
  const double* gx;      // ghN: sqrt(2) x_g
  const double* glw;     // ghN: log w_g
  // the chunk's samples
  const double* Beta;    // chunk x nc x ns
  const double* sigma;   // chunk x ns
  const double* Eta[HMSC_MAX_LEVELS];
  const double* Lambda[HMSC_MAX_LEVELS];
  double* val;           // chunk x ny (the chunk's rows of the S x ny table)
};

// log(pi^(-1/2) sum_g w_g dpois(y_g, exp(E + sqrt2 x_g sd))) in max-shifted form over the log
// terms y eta - e^eta - lgamma(y + 1) + log w_g; y_g is the host function's recycled Y entry
// (post.py: index (i + ny c + ny cN g) mod (ny ns)); dpois is 0 off the non-negative integers.
__device__ __forceinline__ double pois_cell(const WaicArgs& a, int i, int c, double E, double sd) {
  double m = -INFINITY, sum = 0.0;
  for (int g = 0; g < a.ghN; ++g) {
    const int col = (int)(((int64_t)c + (int64_t)a.cN * g) % a.ns);
    const double y = a.Y[i + (size_t)a.ny * col];
    const double eta = fma(a.gx[g], sd, E);
    double t = -INFINITY;
    if (y != y) t = y;
    else if (y >= 0.0 && y == floor(y)) t = fma(y, eta, -exp(eta)) - lgamma(y + 1.0) + a.glw[g];
    if (t != t) return t;
    if (t == -INFINITY) continue;
    if (t > m) {
      sum = fma(sum, exp(m - t), 1.0);
      m = t;
    } else {
      sum += exp(t - m);
    }
  }
  if (m == -INFINITY) return m;
  return (m + log(sum)) - 0.5723649429247001;  // log(pi) / 2
}

__device__ __forceinline__ double cell_term(const WaicArgs& a, int fam, int c, int i, double y, double E, double sg) {
  if (y != y) return 0.0;  // NA
  if (fam == 2) {
    const double lp = log_pnorm(y == 0.0 ? -E : E);
    if (y == 0.0 || y == 1.0) return lp;
    return y * lp + (1.0 - y) * log_pnorm(-E);  // (as the host writes it, for a y off {0, 1})
  }
  if (fam == 1) {  // dnorm(y, E, sigma^(-1/2), log): -(y - E)^2 sigma / 2 + log(sigma) / 2 - log sqrt(2 pi)
    const double d = y - E;
    return fma(-0.5 * d * d, sg, fma(0.5, log(sg), -0.9189385332046728));
  }
  return pois_cell(a, i, c, E, 1.0 / sqrt(sg));
}

// K <= 32 (KQ <= 8): registers capped for 4 waves per SIMD.  The four inlined cell terms of a
// lane otherwise take ~250 VGPRs (2 waves); capped, part of them lives in scratch and the kernel
// is still 6 % faster at config 4 (25.8 -> 24.4 ms, same machine).  The wider variants, whose A
// operands alone are up to 64 VGPRs, are left as the compiler allocates them.
template <int KQ>
__global__ __launch_bounds__(256, KQ <= 8 ? 4 : 1) void waic_val_kernel(WaicArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sB[];  // [species of the stage][LD]
  const int t = threadIdx.x, w = t >> 6, l = t & 63, lm = l & 15, lk = l >> 4;
  const int s = blockIdx.y, ny = a.ny, ns = a.ns, nc = a.nc, K = a.K, LD = a.LD;
  const int ib = blockIdx.x * WT_I + 16 * w;
  // A operands: site row 4 (lm & 3) + (lm >> 2), k = 4 q + lk
  double av[KQ];
  {
    const int i = ib + 4 * (lm & 3) + (lm >> 2);
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      const int k = 4 * q + lk;
      double v = 0.0;
      if (i < ny && k < K) {
        if (k < nc) {
          v = a.X[i + (size_t)ny * k];
        } else {
          int kk = k - nc, r = 0;
          while (kk >= a.nf[r]) kk -= a.nf[r++];
          const int u = a.Pi[i + (size_t)ny * r];
          v = a.Eta[r][((size_t)s * a.nf[r] + kk) * a.np[r] + u];
        }
      }
      av[q] = v;
    }
  }
  const int i4 = ib + 4 * lk;  // this lane's four sites i4 .. i4 + 3
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const double* Beta = a.Beta + (size_t)s * nc * ns;
  const double* sigma = a.sigma + (size_t)s * ns;
  const int Kp = 4 * KQ;
  for (int j0 = 0; j0 < ns; j0 += WT_J) {
    __syncthreads();
    for (int p = t; p < WT_J * Kp; p += 256) {
      const int jj = p / Kp, k = p - jj * Kp, j = j0 + jj;
      double v = 0.0;
      if (j < ns && k < K) {
        if (k < nc) {
          v = Beta[k + (size_t)nc * j];
        } else {
          int kk = k - nc, r = 0;
          while (kk >= a.nf[r]) kk -= a.nf[r++];
          v = a.Lambda[r][((size_t)s * ns + j) * a.nf[r] + kk];
        }
      }
      sB[jj * LD + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < WT_J / 16; ++tt) {
      const int j = j0 + 16 * tt + lm;
      d4 e = {0.0, 0.0, 0.0, 0.0};
      const double* b = sB + (16 * tt + lm) * LD + lk;
#pragma unroll
      for (int q = 0; q < KQ; ++q) e = mfma_f64(av[q], b[4 * q], e);
      if (j < ns) {
        const int fam = a.family[j], c = a.prank[j];
        const double sg = sigma[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i4 + r;
          if (i < ny) acc[r] += cell_term(a, fam, c, i, a.Y[i + (size_t)ny * j], e[r], sg);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double v = acc[r];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    if (lm == 0 && i4 + r < ny) a.val[(size_t)s * ny + i4 + r] = v;
  }
}

// site[i] = Bl_i, site[ny + i] = V_i over the S samples of val (S x ny), in sample order
__global__ __launch_bounds__(256) void waic_site_kernel(int S, int ny, const double* val, double* site) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ny) return;
  double m = -INFINITY, mean = 0.0;
  for (int s = 0; s < S; ++s) {
    const double v = val[(size_t)s * ny + i];
    m = v > m || v != v ? v : m;
    mean += v;
  }
  mean /= S;
  double se = 0.0, ss = 0.0;
  for (int s = 0; s < S; ++s) {
    const double v = val[(size_t)s * ny + i];
    se += exp(v - m);
    const double d = v - mean;
    ss = fma(d, d, ss);
  }
  site[i] = -(m + log(se / S));
  site[ny + i] = ss / (S - 1);
}

__global__ __launch_bounds__(256) void waic_mean_kernel(int ny, const double* site, double* out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double v = 0.0;
  for (int i = t; i < ny; i += 256) v += site[i] + site[ny + i];
  red[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) out[0] = red[0] / ny;
}

static thread_local double g_waic_ms[3] = {0.0, 0.0, 0.0};
void waic_last_timing(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_waic_ms[k];
}

void run_waic(const hmsc_waic_args* p, double* waic, double* site, double* val) {
  HMSC_REQUIRE(p->ny > 0 && p->ns > 0 && p->nc >= 0, "hmsc_waic: ny and ns must be positive");
  HMSC_REQUIRE(p->nr >= 0 && p->nr <= HMSC_MAX_LEVELS, "hmsc_waic: bad nr");
  HMSC_REQUIRE(p->nsamples >= 2, "hmsc_waic: nsamples must be at least 2 (the variance over samples has ddof = 1)");
  HMSC_REQUIRE(p->sample_chunk >= 0, "hmsc_waic: sample_chunk must be non-negative");
  HMSC_REQUIRE(p->Y && p->X && p->Beta && p->sigma && p->family, "hmsc_waic: NULL Y / X / Beta / sigma / family");
  HMSC_REQUIRE(p->nr == 0 || (p->Pi && p->np && p->nf), "hmsc_waic: NULL Pi / np / nf");
  int K = p->nc;
  for (int r = 0; r < p->nr; ++r) {
    HMSC_REQUIRE(p->nf[r] >= 1 && p->np[r] >= 1, "hmsc_waic: every level needs nf >= 1 and np >= 1");
    HMSC_REQUIRE(p->Eta[r] && p->Lambda[r], "hmsc_waic: NULL Eta / Lambda");
    K += p->nf[r];
  }
  HMSC_REQUIRE(K >= 1, "hmsc_waic: nc + sum(nf) must be positive");
  HMSC_REQUIRE(K <= HMSC_KCAP, "hmsc_waic: nc + sum(nf) = " + std::to_string(K) + " exceeds HMSC_KCAP = " +
                                   std::to_string(HMSC_KCAP));
  const size_t S = p->nsamples, ny = p->ny, ns = p->ns, nc = p->nc;
  std::vector<int> prank(ns, -1);
  int cN = 0;
  for (size_t j = 0; j < ns; ++j) {
    HMSC_REQUIRE(p->family[j] >= 1 && p->family[j] <= 3, "hmsc_waic: family must be 1 (normal), 2 (probit) or 3 (Poisson)");
    if (p->family[j] == 3) prank[j] = cN++;
  }
  std::vector<double> gx(std::max(1, p->ghN)), glw(std::max(1, p->ghN));
  if (cN > 0) {
    HMSC_REQUIRE(p->ghN >= 1 && p->ghN <= WAIC_GH_MAX && p->gx && p->gw, "hmsc_waic: Poisson columns need 1 <= ghN <= 256 nodes gx and weights gw");
    for (int g = 0; g < p->ghN; ++g) {
      HMSC_REQUIRE(p->gw[g] > 0.0, "hmsc_waic: Gauss-Hermite weights must be positive");
      gx[g] = std::sqrt(2.0) * p->gx[g];
      glw[g] = std::log(p->gw[g]);
    }
  }
  std::vector<int> pi0(ny * std::max(1, p->nr));
  for (int r = 0; r < p->nr; ++r)
    for (size_t i = 0; i < ny; ++i) {
      const int u = p->Pi[i + ny * r] - 1;
      HMSC_REQUIRE(u >= 0 && u < p->np[r], "hmsc_waic: Pi out of range");
      pi0[i + ny * r] = u;
    }
  // samples resident at once: the caller's, else what keeps a chunk's stacks near 256 MB
  size_t per = nc * ns + ns;
  for (int r = 0; r < p->nr; ++r) per += (size_t)p->nf[r] * ((size_t)p->np[r] + ns);
  size_t chunk = p->sample_chunk > 0 ? (size_t)p->sample_chunk : std::max<size_t>(1, ((size_t)256 << 20) / (8 * per));
  chunk = std::min(std::min(chunk, S), (size_t)65535);

  DeviceGuard dg(p->device);
  DeviceOwner own;  // drains the stream and frees everything on every exit
  const hipStream_t st = own.stream();
  auto t0 = std::chrono::steady_clock::now();
  WaicArgs a{};
  a.ny = p->ny, a.ns = p->ns, a.nc = p->nc, a.nr = p->nr, a.K = K, a.ghN = cN > 0 ? p->ghN : 0, a.cN = cN;
  const int KQ = K <= 8 ? 2 : K <= 32 ? 8 : K <= 64 ? 16 : 32;
  a.LD = ((4 * KQ + 29) / 32) * 32 + 2;  // >= 4 KQ, = 2 mod 32
  a.Y = own.upload(p->Y, ny * ns, st);
  a.X = own.upload(p->X, ny * nc, st);
  a.family = own.upload(p->family, ns, st);
  a.prank = own.upload(prank.data(), ns, st);
  a.Pi = own.upload(pi0.data(), pi0.size(), st);
  a.gx = own.upload(gx.data(), gx.size(), st);
  a.glw = own.upload(glw.data(), glw.size(), st);
  double* dBeta = own.alloc<double>(chunk * nc * ns);
  double* dSigma = own.alloc<double>(chunk * ns);
  double *dEta[HMSC_MAX_LEVELS] = {}, *dLam[HMSC_MAX_LEVELS] = {};
  for (int r = 0; r < p->nr; ++r) {
    a.np[r] = p->np[r];
    a.nf[r] = p->nf[r];
    dEta[r] = own.alloc<double>(chunk * p->np[r] * p->nf[r]);
    dLam[r] = own.alloc<double>(chunk * p->nf[r] * ns);
    a.Eta[r] = dEta[r];
    a.Lambda[r] = dLam[r];
  }
  a.Beta = dBeta;
  a.sigma = dSigma;
  double* dVal = own.alloc<double>(S * ny);
  double* dSite = own.alloc<double>(2 * ny);
  double* dOut = own.alloc<double>(1);
  HIP_OK(hipStreamSynchronize(st));
  double up_ms = ms_since(t0), ka_ms = 0.0;
  const size_t smem = (size_t)WT_J * a.LD * sizeof(double);
  for (size_t s0 = 0; s0 < S; s0 += chunk) {
    const size_t c = std::min(chunk, S - s0);
    t0 = std::chrono::steady_clock::now();
    HIP_OK(hipMemcpyAsync(dBeta, p->Beta + s0 * nc * ns, c * nc * ns * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(dSigma, p->sigma + s0 * ns, c * ns * 8, hipMemcpyHostToDevice, st));
    for (int r = 0; r < p->nr; ++r) {
      const size_t ne = (size_t)p->np[r] * p->nf[r], nl = (size_t)p->nf[r] * ns;
      HIP_OK(hipMemcpyAsync(dEta[r], p->Eta[r] + s0 * ne, c * ne * 8, hipMemcpyHostToDevice, st));
      HIP_OK(hipMemcpyAsync(dLam[r], p->Lambda[r] + s0 * nl, c * nl * 8, hipMemcpyHostToDevice, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    up_ms += ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    a.val = dVal + s0 * ny;
    const dim3 grid((unsigned)((ny + WT_I - 1) / WT_I), (unsigned)c);
    if (KQ == 2) waic_val_kernel<2><<<grid, 256, smem, st>>>(a);
    else if (KQ == 8) waic_val_kernel<8><<<grid, 256, smem, st>>>(a);
    else if (KQ == 16) waic_val_kernel<16><<<grid, 256, smem, st>>>(a);
    else waic_val_kernel<32><<<grid, 256, smem, st>>>(a);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    ka_ms += ms_since(t0);
  }
  t0 = std::chrono::steady_clock::now();
  waic_site_kernel<<<(unsigned)((ny + 255) / 256), 256, 0, st>>>((int)S, (int)ny, dVal, dSite);
  HIP_OK(hipGetLastError());
  waic_mean_kernel<<<1, 256, 0, st>>>((int)ny, dSite, dOut);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(waic, dOut, 8, hipMemcpyDeviceToHost, st));
  if (site) HIP_OK(hipMemcpyAsync(site, dSite, 2 * ny * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  const double kb_ms = ms_since(t0);
  if (val) copy_sync(val, dVal, S * ny * 8, hipMemcpyDeviceToHost, st);
  g_waic_ms[0] = up_ms, g_waic_ms[1] = ka_ms, g_waic_ms[2] = kb_ms;
}

}  // namespace hmsc
