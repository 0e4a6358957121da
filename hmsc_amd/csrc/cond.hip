// Batched conditional prediction (R/predict.R:181-198; hmsc_predict_conditional in
// include/hmsc_amd.h): for every sample of a pooled posterior, Z = L, updateZ given Yc, then
// mcmcStep x (updateEta, updateZ) with the sample's Beta, sigma and Lambda fixed.  Samples are
// independent, so they are a grid axis of every launch: per resident chunk of samples the stream
// carries the prep launches, one Z launch, then mcmcStep x (one Eta launch per level, one Z
// launch).  No workgroup waits on another one: every dependency is a launch boundary of the one
// stream, and the host does not synchronise between the steps.
//
// cond_prec_kernel, once per chunk and level: for unit q, Q = I + sum_j c_qj isigma_j lambda_j
//   lambda_j^T with c_qj the number of q's rows in which species j is observed.  Q depends on q
//   only through the count vector, so the caller passes the distinct count vectors (classes) and
//   each unit's class; the kernel forms and factors Q = F F^T per (sample, class).  Lambda, sigma
//   and the NA mask do not move during the mcmcStep loop: nothing is refactored in it.
// cond_z_kernel, grid (64-site tiles, 32-species tiles, samples): E = [X | Eta_r[Pi_r,]] [Beta;
//   Lambda_r] on v_mfma_f64_16x16x4 with the species as the MFMA rows (coefficient block in LDS,
//   row m of a 16-species tile = species 4 (m & 3) + (m >> 2)) and the sites as its columns (site
//   rows in registers): a lane ends with one site and one species quad, the unit of updateZ's
//   Philox block, and the 16 lanes of a row group store 128-byte site runs.  Each observed cell is
//   drawn by the scalar functions of z_kernel.h.  In the first launch zPrev of a Poisson cell is E
//   itself (Z = L): there is no "Z = L" pass.
//   NA cells are neither drawn nor stored.  Nothing in scope reads them: every updateEta branch
//   served here sums over observed cells only (R/updateEta.R:59-70,80-87; :75-79 applies only
//   where nothing is NA and equals the masked sum there), and R's final L is formed from the
//   conditioned Eta, not from Z (R/predict.R:188-197).
// cond_eta_kernel, one launch per level, grid (units, samples), one wave per (unit, sample):
//   b = sum_{rows i of q} sum_{j observed} isigma_j lambda_j (Z_ij - L(-r)_ij), L(-r) recomputed
//   from the staged row as eta_na_row_kernel does; eta = F^-T (F^-1 b + xi).  Lanes run over
//   species, rows come by the unit CSR; a lane adds its cells in (row, species) order and the 64
//   lanes combine in a fixed xor tree, so the sums do not depend on the chunking.  The lanes read
//   the coefficients from a copy with the species contiguous (cond_blt_kernel, once per chunk).
//   A unit with no observed cell has Q = I, b = 0: a fresh N(0, I) draw, as in R.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hmsc_amd.h"
#include "common.h"
#include "devmem.h"
#include "rng.h"
#include "z_kernel.h"  // d4, mfma_f64, z_probit_draw, z_poisson_draw

namespace hmsc {

constexpr int CT_I = 64, CT_J = 32, COND_NF_MAX = 32;
constexpr size_t COND_SLAB_CAP = (size_t)16 << 30;  // bytes of the default chunk's Z slab

struct CondArgs {
  int ny, ns, nc, nr, K, LD, steps;  // steps = 2 mcmcStep + 1 iterations per sample
  int np[HMSC_MAX_LEVELS], nf[HMSC_MAX_LEVELS];
  const double* X;     // ny x nc
  const double* Yc;    // ny x ns, NaN = NA
  const int* family;   // ns
  const int* Pi;       // ny x nr, 0-based
  // the chunk's samples
  const double* Beta;  // chunk x nc x ns
  const double* sigma; // chunk x ns
  double* Eta[HMSC_MAX_LEVELS];           // chunk x np x nf, updated in place
  const double* Lambda[HMSC_MAX_LEVELS];  // chunk x nf x ns
  double* Z;           // chunk x ny x ns
  const double* BLT;   // chunk x (K + 1) x ns: the rows of [Beta; Lambda_r], species contiguous, then 1 / sigma
  Key key;
  uint32_t s0;         // index of the chunk's first sample in the call
};

// Philox iteration of sample s (in the chunk) at offset off of its 2 mcmcStep + 1 iterations
__device__ __forceinline__ uint32_t cond_iter(const CondArgs& a, int s, uint32_t off) {
  return 1u + (a.s0 + (uint32_t)s) * (uint32_t)a.steps + off;
}

// level of column k >= nc of [X | Eta_0 | Eta_1 ...] and the factor in it
__device__ __forceinline__ int cond_level(const CondArgs& a, int k, int* kk) {
  int f = k - a.nc, r = 0;
  while (f >= a.nf[r]) f -= a.nf[r++];
  *kk = f;
  return r;
}

__global__ __launch_bounds__(64) void cond_prec_kernel(CondArgs a, int r, int ncls, const int* cnt, double* F,
                                                       int* bad) {
  extern __shared__ __attribute__((aligned(16))) double sQ[];  // nf x nf, then the flag
  const int t = threadIdx.x, c = blockIdx.x, s = blockIdx.y, nf = a.nf[r], ns = a.ns;
  int* flag = (int*)(sQ + nf * nf);
  const double* lam = a.Lambda[r] + (size_t)s * ns * nf;
  const double* sigma = a.sigma + (size_t)s * ns;
  const int* cc = cnt + (size_t)c * ns;
  for (int p = t; p < nf * nf; p += 64) {
    const int h1 = p % nf, h2 = p / nf;
    double q = h1 == h2 ? 1.0 : 0.0;
    for (int j = 0; j < ns; ++j) {
      const int n = cc[j];
      if (n) q += ((double)n * (1.0 / sigma[j])) * lam[h1 + (size_t)nf * j] * lam[h2 + (size_t)nf * j];
    }
    sQ[p] = q;
  }
  __syncthreads();
  const bool ok = wg_chol(sQ, nf, nf, flag);
  if (!ok && t == 0) atomicOr(bad, 1);
  double* Fq = F + ((size_t)s * ncls + c) * nf * nf;
  for (int p = t; p < nf * nf; p += 64) Fq[p] = sQ[p];  // lower triangle: the factor
}

// The coefficient block of a sample with the species contiguous, for the Eta launches (a lane per
// species): row k < K of [Beta; Lambda_0; Lambda_1 ...], then the row of 1 / sigma.
__global__ __launch_bounds__(256) void cond_blt_kernel(CondArgs a, double* BLT) {
  const int s = blockIdx.y, ns = a.ns, nc = a.nc, K = a.K;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)(K + 1) * ns) return;
  const int k = (int)(p / ns), j = (int)(p - (size_t)k * ns);
  double v;
  if (k == K) {
    v = 1.0 / a.sigma[(size_t)s * ns + j];
  } else if (k < nc) {
    v = a.Beta[(size_t)s * nc * ns + k + (size_t)nc * j];
  } else {
    int kk;
    const int r = cond_level(a, k, &kk);
    v = a.Lambda[r][((size_t)s * ns + j) * a.nf[r] + kk];
  }
  BLT[(size_t)s * (K + 1) * ns + p] = v;
}

template <int KQ>
__global__ __launch_bounds__(256) void cond_z_kernel(CondArgs a, uint32_t off, int first) {
  extern __shared__ __attribute__((aligned(16))) double sB[];  // [species of the tile][LD]
  const int t = threadIdx.x, w = t >> 6, l = t & 63, lm = l & 15, lk = l >> 4;
  const int s = blockIdx.z, j0 = blockIdx.y * CT_J, ny = a.ny, ns = a.ns, nc = a.nc, K = a.K, LD = a.LD;
  const int i = blockIdx.x * CT_I + 16 * w + lm;  // this lane's site
  // B operands: site i, k = 4 q + lk
  double av[KQ];
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const int k = 4 * q + lk;
    double v = 0.0;
    if (i < ny && k < K) {
      if (k < nc) {
        v = a.X[i + (size_t)ny * k];
      } else {
        int kk;
        const int r = cond_level(a, k, &kk);
        const int u = a.Pi[i + (size_t)ny * r];
        v = a.Eta[r][((size_t)s * a.nf[r] + kk) * a.np[r] + u];
      }
    }
    av[q] = v;
  }
  const double* Beta = a.Beta + (size_t)s * nc * ns;
  const double* sigma = a.sigma + (size_t)s * ns;
  double* Z = a.Z + (size_t)s * ny * ns;
  constexpr int Kp = 4 * KQ;
  for (int p = t; p < CT_J * Kp; p += 256) {
    const int jj = p / Kp, k = p - jj * Kp, j = j0 + jj;
    double v = 0.0;
    if (j < ns && k < K) {
      if (k < nc) {
        v = Beta[k + (size_t)nc * j];
      } else {
        int kk;
        const int r = cond_level(a, k, &kk);
        v = a.Lambda[r][((size_t)s * ns + j) * a.nf[r] + kk];
      }
    }
    sB[jj * LD + k] = v;
  }
  __syncthreads();
  const uint32_t iter = cond_iter(a, s, off);
#pragma unroll
  for (int tt = 0; tt < CT_J / 16; ++tt) {
    d4 e = {0.0, 0.0, 0.0, 0.0};
    // MFMA row lm = species 4 (lm & 3) + (lm >> 2) of the 16: result row lk + 4 r = species 4 lk + r
    const double* b = sB + (16 * tt + 4 * (lm & 3) + (lm >> 2)) * LD + lk;
#pragma unroll
    for (int q = 0; q < KQ; ++q) e = mfma_f64(b[4 * q], av[q], e);
    const int jq = j0 + 16 * tt + 4 * lk;  // this lane's species quad jq .. jq + 3
    U4 qw{0u, 0u, 0u, 0u};
    bool have = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = jq + r;
      if (i >= ny || j >= ns) continue;
      const size_t cell = (size_t)i + (size_t)ny * j;
      const double y = a.Yc[cell];
      if (y != y) continue;  // NA: not drawn, not stored
      const int fam = a.family[j];
      double z = y;          // normal: Z = Y   R/updateZ.R:40-41
      if (fam != 1) {
        const double is = 1.0 / sigma[j], sd = 1.0 / sqrt(is);
        if (fam == 2) {
          if (!have) {
            qw = philox4x32_10(U4{(uint32_t)((size_t)i + (size_t)ny * (uint32_t)(jq >> 2)), 0u, (uint32_t)S_Z, iter}, a.key);
            have = true;
          }
          const uint32_t wd = r == 0 ? qw.x : r == 1 ? qw.y : r == 2 ? qw.z : qw.w;
          z = z_probit_draw(e[r], sd, sqrt(is), y != 0.0 ? 1 : 0, u32o(wd), 0);
        } else {
          const double zprev = first ? e[r] : Z[cell];
          z = z_poisson_draw(e[r], sd, y, zprev, uniforms(a.key, (uint32_t)cell, 0u, (uint32_t)S_ZPOIS, iter), 0);
        }
      }
      Z[cell] = z;
    }
  }
}

template <int NFB>
__global__ __launch_bounds__(64) void cond_eta_kernel(CondArgs a, int r, uint32_t off, int ncls, const int* unit_ptr,
                                                      const int* unit_rows, const int* unit_class, const double* F) {
  extern __shared__ __attribute__((aligned(16))) double sx[];  // the row of [X | Eta[Pi,]] (K), then b (32)
  const int lane = threadIdx.x, q = blockIdx.x, s = blockIdx.y;
  const int ny = a.ny, ns = a.ns, nc = a.nc, K = a.K, nf = a.nf[r];
  double* sb = sx + K;
  int loff = nc;
  for (int r2 = 0; r2 < r; ++r2) loff += a.nf[r2];
  const double* T = a.BLT + (size_t)s * (K + 1) * ns;  // coefficient rows, species contiguous
  const double* Tis = T + (size_t)K * ns;              // 1 / sigma
  const double* Tr = T + (size_t)loff * ns;            // level r's loadings
  const double* Z = a.Z + (size_t)s * ny * ns;
  double acc[NFB];
#pragma unroll
  for (int h = 0; h < NFB; ++h) acc[h] = 0.0;
  const int pb = unit_ptr[q], pe = unit_ptr[q + 1];
  for (int p = pb; p < pe; ++p) {
    const int i = unit_rows[p];
    __syncthreads();
    for (int k = lane; k < K; k += 64) {
      double v = 0.0;  // level r's own columns stay 0: L(-r)
      if (k < nc) {
        v = a.X[i + (size_t)ny * k];
      } else if (k < loff || k >= loff + nf) {
        int kk;
        const int r2 = cond_level(a, k, &kk);
        v = a.Eta[r2][((size_t)s * a.nf[r2] + kk) * a.np[r2] + a.Pi[i + (size_t)ny * r2]];
      }
      sx[k] = v;
    }
    __syncthreads();
    for (int j = lane; j < ns; j += 64) {
      const size_t cell = (size_t)i + (size_t)ny * j;
      const double y = a.Yc[cell];
      if (y != y) continue;
      double lp = 0.0;  // L(-r): the staged row is 0 in level r's columns
      for (int k = 0; k < K; ++k) lp = fma(sx[k], T[(size_t)k * ns + j], lp);
      const double wgt = (Z[cell] - lp) * Tis[j];
#pragma unroll
      for (int h = 0; h < NFB; ++h)
        if (h < nf) acc[h] = fma(Tr[(size_t)h * ns + j], wgt, acc[h]);
    }
  }
#pragma unroll
  for (int h = 0; h < NFB; ++h) {
    if (h < nf) {  // (uniform)
      double v = acc[h];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) sb[h] = v;
    }
  }
  __syncthreads();
  // y = F^-1 b; y += xi; eta = F^-T y  (= Q^-1 b + R^-1 xi, R = F^T: R/updateEta.R:56,69,90)
  const double* Fq = F + ((size_t)s * ncls + unit_class[q]) * nf * nf;
  wg_forward(Fq, nf, nf, sb);
  if (lane < nf)
    sb[lane] += normal(a.key, (uint32_t)q, (uint32_t)lane, (uint32_t)S_ETA + LEVEL_STRIDE * (uint32_t)r, cond_iter(a, s, off));
  __syncthreads();
  wg_backward_t(Fq, nf, nf, sb);
  if (lane < nf) a.Eta[r][((size_t)s * nf + lane) * a.np[r] + q] = sb[lane];
}

static thread_local double g_cond_ms[4] = {0.0, 0.0, 0.0, 0.0};
void cond_last_timing(double out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = g_cond_ms[k];
}

void run_cond(const hmsc_cond_args* p, double* const* EtaOut) {
  for (int k = 0; k < 4; ++k) g_cond_ms[k] = 0.0;
  HMSC_REQUIRE(p->nsamples >= 0, "hmsc_predict_conditional: nsamples must be non-negative");
  if (p->nsamples == 0) return;
  HMSC_REQUIRE(p->ny > 0 && p->ns > 0 && p->nc >= 0, "hmsc_predict_conditional: ny and ns must be positive");
  HMSC_REQUIRE(p->nr >= 0 && p->nr <= HMSC_MAX_LEVELS, "hmsc_predict_conditional: bad nr");
  HMSC_REQUIRE(p->mcmcStep >= 0, "hmsc_predict_conditional: mcmcStep must be non-negative");
  HMSC_REQUIRE(p->sample_chunk >= 0, "hmsc_predict_conditional: sample_chunk must be non-negative");
  if (p->nr == 0) return;  // no latent factors to condition
  HMSC_REQUIRE(p->X && p->Beta && p->sigma && p->family && p->Yc,
               "hmsc_predict_conditional: NULL X / Beta / sigma / family / Yc");
  HMSC_REQUIRE(p->Pi && p->np && p->nf && p->ncls, "hmsc_predict_conditional: NULL Pi / np / nf / ncls");
  const size_t S = p->nsamples, ny = p->ny, ns = p->ns, nc = p->nc;
  const int nr = p->nr;
  int K = p->nc;
  for (int r = 0; r < nr; ++r) {
    HMSC_REQUIRE(p->nf[r] >= 1 && p->np[r] >= 1, "hmsc_predict_conditional: every level needs nf >= 1 and np >= 1");
    HMSC_REQUIRE(p->nf[r] <= COND_NF_MAX, "hmsc_predict_conditional: nf = " + std::to_string(p->nf[r]) + " of level " +
                                              std::to_string(r) + " exceeds 32");
    HMSC_REQUIRE(p->Eta[r] && p->Lambda[r] && EtaOut[r], "hmsc_predict_conditional: NULL Eta / Lambda / EtaOut");
    HMSC_REQUIRE(p->ncls[r] >= 1 && p->cnt[r] && p->unit_class[r], "hmsc_predict_conditional: NULL cnt / unit_class");
    K += p->nf[r];
  }
  HMSC_REQUIRE(K <= HMSC_KCAP, "hmsc_predict_conditional: nc + sum(nf) = " + std::to_string(K) +
                                   " exceeds HMSC_KCAP = " + std::to_string(HMSC_KCAP));
  HMSC_REQUIRE(ny * ns < ((size_t)1 << 32), "hmsc_predict_conditional: ny * ns = " + std::to_string(ny * ns) +
                                                " does not fit the 32-bit cell counter (ny * ns < 2^32)");
  HMSC_REQUIRE((ns + CT_J - 1) / CT_J <= 65535, "hmsc_predict_conditional: ns exceeds 65535 * 32");
  const size_t steps = 2 * (size_t)p->mcmcStep + 1;
  HMSC_REQUIRE(1 + S * steps < ((size_t)1 << 32), "hmsc_predict_conditional: nsamples * (2 mcmcStep + 1) does not fit "
                                                   "the 32-bit iteration counter");
  for (size_t j = 0; j < ns; ++j)
    HMSC_REQUIRE(p->family[j] >= 1 && p->family[j] <= 3,
                 "hmsc_predict_conditional: family must be 1 (normal), 2 (probit) or 3 (Poisson)");
  for (size_t k = 0; k < S * ns; ++k)
    HMSC_REQUIRE(std::isfinite(p->sigma[k]) && p->sigma[k] > 0.0,
                 "hmsc_predict_conditional: sigma of sample " + std::to_string(k / ns) + ", species " +
                     std::to_string(k % ns) + " is not finite and positive");
  std::vector<int> pi0(ny * nr);
  for (int r = 0; r < nr; ++r)
    for (size_t i = 0; i < ny; ++i) {
      const int u = p->Pi[i + ny * r] - 1;
      HMSC_REQUIRE(u >= 0 && u < p->np[r], "hmsc_predict_conditional: Pi out of range");
      pi0[i + ny * r] = u;
    }
  bool any_obs = false;
  for (size_t c = 0; c < ny * ns && !any_obs; ++c) any_obs = !std::isnan(p->Yc[c]);
  if (!any_obs) {  // nothing to condition on: the input Eta, unchanged
    for (int r = 0; r < nr; ++r)
      if (EtaOut[r] != p->Eta[r]) std::memcpy(EtaOut[r], p->Eta[r], S * p->np[r] * p->nf[r] * sizeof(double));
    return;
  }
  // the unit CSR of every level, and the caller's classes held to the count matrix of (Yc, Pi)
  std::vector<std::vector<int>> uptr(nr), urows(nr);
  size_t fac_per = 0;  // doubles of one sample's factors
  for (int r = 0; r < nr; ++r) {
    const size_t npr = p->np[r];
    uptr[r].assign(npr + 1, 0);
    urows[r].resize(ny);
    for (size_t i = 0; i < ny; ++i) ++uptr[r][pi0[i + ny * r] + 1];
    for (size_t q = 0; q < npr; ++q) uptr[r][q + 1] += uptr[r][q];
    std::vector<int> fill(uptr[r].begin(), uptr[r].end() - 1);
    for (size_t i = 0; i < ny; ++i) urows[r][fill[pi0[i + ny * r]]++] = (int)i;
    for (size_t q = 0; q < npr; ++q)
      HMSC_REQUIRE(p->unit_class[r][q] >= 0 && p->unit_class[r][q] < p->ncls[r],
                   "hmsc_predict_conditional: unit_class out of range");
    std::vector<int> cq(npr);  // species by species (Yc's columns are contiguous)
    for (size_t j = 0; j < ns; ++j) {
      std::fill(cq.begin(), cq.end(), 0);
      const double* y = p->Yc + ny * j;
      const int* pr = pi0.data() + ny * r;
      for (size_t i = 0; i < ny; ++i) cq[pr[i]] += std::isnan(y[i]) ? 0 : 1;
      for (size_t q = 0; q < npr; ++q)
        HMSC_REQUIRE(cq[q] == p->cnt[r][(size_t)p->unit_class[r][q] * ns + j],
                     "hmsc_predict_conditional: cnt of the class of unit " + std::to_string(q) + " of level " +
                         std::to_string(r) + " is not the unit's count of observed rows per species");
    }
    fac_per += (size_t)p->ncls[r] * p->nf[r] * p->nf[r];
  }

  DeviceGuard dg(p->device);
  DeviceOwner own;  // drains the stream and frees everything on every exit
  const hipStream_t st = own.stream();
  auto t0 = std::chrono::steady_clock::now();
  CondArgs a{};
  a.ny = p->ny, a.ns = p->ns, a.nc = p->nc, a.nr = nr, a.K = K, a.steps = (int)steps;
  a.key = Key{(uint32_t)(p->seed & 0xFFFFFFFFu), (uint32_t)(p->seed >> 32)};
  const int KQ = K <= 8 ? 2 : K <= 32 ? 8 : K <= 64 ? 16 : 32;
  a.LD = ((4 * KQ + 29) / 32) * 32 + 2;  // >= 4 KQ, = 2 mod 32 (waic.hip)
  a.X = own.upload(p->X, ny * nc, st);
  a.Yc = own.upload(p->Yc, ny * ns, st);
  a.family = own.upload(p->family, ns, st);
  a.Pi = own.upload(pi0.data(), pi0.size(), st);
  const int *dPtr[HMSC_MAX_LEVELS] = {}, *dRows[HMSC_MAX_LEVELS] = {}, *dCls[HMSC_MAX_LEVELS] = {},
            *dCnt[HMSC_MAX_LEVELS] = {};
  for (int r = 0; r < nr; ++r) {
    a.np[r] = p->np[r];
    a.nf[r] = p->nf[r];
    dPtr[r] = own.upload(uptr[r].data(), uptr[r].size(), st);
    dRows[r] = own.upload(urows[r].data(), urows[r].size(), st);
    dCls[r] = own.upload(p->unit_class[r], (size_t)p->np[r], st);
    dCnt[r] = own.upload(p->cnt[r], (size_t)p->ncls[r] * ns, st);
  }
  int* dBad = own.alloc<int>(1);
  // samples resident at once: the Z slab, the stacks and the factors of a chunk.  The caller's
  // count, else what fits in 3/4 of the free device memory with the slab capped at 16 GiB.
  size_t per = ny * ns + nc * ns + ns + ((size_t)K + 1) * ns + fac_per;
  for (int r = 0; r < nr; ++r) per += (size_t)p->nf[r] * ((size_t)p->np[r] + ns);
  per *= sizeof(double);
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  const size_t budget = free_b / 4 * 3;
  HMSC_REQUIRE(per <= budget, "hmsc_predict_conditional: one sample needs " + std::to_string(per) +
                                  " bytes on the device, " + std::to_string(budget) + " are available");
  size_t chunk = p->sample_chunk > 0
                     ? (size_t)p->sample_chunk
                     : std::min(budget / per, std::max<size_t>(1, COND_SLAB_CAP / (ny * ns * sizeof(double))));
  chunk = std::max<size_t>(1, std::min(std::min(chunk, S), (size_t)65535));
  double* dBeta = own.alloc<double>(chunk * nc * ns);
  double* dSigma = own.alloc<double>(chunk * ns);
  double *dLam[HMSC_MAX_LEVELS] = {}, *dF[HMSC_MAX_LEVELS] = {};
  for (int r = 0; r < nr; ++r) {
    a.Eta[r] = own.alloc<double>(chunk * p->np[r] * p->nf[r]);
    dLam[r] = own.alloc<double>(chunk * p->nf[r] * ns);
    a.Lambda[r] = dLam[r];
    dF[r] = own.alloc<double>(chunk * p->ncls[r] * p->nf[r] * p->nf[r]);
  }
  a.Beta = dBeta;
  a.sigma = dSigma;
  a.Z = own.alloc<double>(chunk * ny * ns);
  double* dBLT = own.alloc<double>(chunk * ((size_t)K + 1) * ns);
  a.BLT = dBLT;
  // one event per launch boundary of a chunk: the Z and Eta launch times without a host sync
  const size_t n_launch = steps + (size_t)p->mcmcStep * nr;
  std::vector<hipEvent_t> ev(n_launch + 1);
  for (auto& e : ev) e = own.event();
  std::vector<char> is_z(n_launch);
  HIP_OK(hipStreamSynchronize(st));
  double up_ms = ms_since(t0), z_ms = 0.0, eta_ms = 0.0, back_ms = 0.0;

  const size_t zsmem = (size_t)CT_J * a.LD * sizeof(double);
  auto launch_z = [&](size_t c, uint32_t off, int first) {
    const dim3 grid((unsigned)((ny + CT_I - 1) / CT_I), (unsigned)((ns + CT_J - 1) / CT_J), (unsigned)c);
    if (KQ == 2) cond_z_kernel<2><<<grid, 256, zsmem, st>>>(a, off, first);
    else if (KQ == 8) cond_z_kernel<8><<<grid, 256, zsmem, st>>>(a, off, first);
    else if (KQ == 16) cond_z_kernel<16><<<grid, 256, zsmem, st>>>(a, off, first);
    else cond_z_kernel<32><<<grid, 256, zsmem, st>>>(a, off, first);
    HIP_OK(hipGetLastError());
  };
  auto launch_eta = [&](size_t c, int r, uint32_t off) {
    const dim3 grid((unsigned)p->np[r], (unsigned)c);
    const size_t smem = (size_t)(K + COND_NF_MAX) * sizeof(double);
    const int nf = p->nf[r];
    if (nf <= 8) cond_eta_kernel<8><<<grid, 64, smem, st>>>(a, r, off, p->ncls[r], dPtr[r], dRows[r], dCls[r], dF[r]);
    else if (nf <= 16) cond_eta_kernel<16><<<grid, 64, smem, st>>>(a, r, off, p->ncls[r], dPtr[r], dRows[r], dCls[r], dF[r]);
    else cond_eta_kernel<32><<<grid, 64, smem, st>>>(a, r, off, p->ncls[r], dPtr[r], dRows[r], dCls[r], dF[r]);
    HIP_OK(hipGetLastError());
  };

  for (size_t s0 = 0; s0 < S; s0 += chunk) {
    const size_t c = std::min(chunk, S - s0);
    t0 = std::chrono::steady_clock::now();
    a.s0 = (uint32_t)s0;
    HIP_OK(hipMemcpyAsync(dBeta, p->Beta + s0 * nc * ns, c * nc * ns * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(dSigma, p->sigma + s0 * ns, c * ns * 8, hipMemcpyHostToDevice, st));
    for (int r = 0; r < nr; ++r) {
      const size_t ne = (size_t)p->np[r] * p->nf[r], nl = (size_t)p->nf[r] * ns;
      HIP_OK(hipMemcpyAsync(a.Eta[r], p->Eta[r] + s0 * ne, c * ne * 8, hipMemcpyHostToDevice, st));
      HIP_OK(hipMemcpyAsync(dLam[r], p->Lambda[r] + s0 * nl, c * nl * 8, hipMemcpyHostToDevice, st));
    }
    cond_blt_kernel<<<dim3((unsigned)((((size_t)K + 1) * ns + 255) / 256), (unsigned)c), 256, 0, st>>>(a, dBLT);
    HIP_OK(hipGetLastError());
    for (int r = 0; r < nr; ++r) {
      const int nf = p->nf[r];
      cond_prec_kernel<<<dim3((unsigned)p->ncls[r], (unsigned)c), 64, (size_t)(nf * nf + 2) * sizeof(double), st>>>(
          a, r, p->ncls[r], dCnt[r], dF[r], dBad);
      HIP_OK(hipGetLastError());
    }
    int bad = 0;
    HIP_OK(hipMemcpyAsync(&bad, dBad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HMSC_REQUIRE(bad == 0, "hmsc_predict_conditional: a unit's precision I + sum_j c_j lambda_j lambda_j' / sigma_j "
                           "is not positive definite (non-finite Lambda?)");
    up_ms += ms_since(t0);
    // the chunk's whole loop, queued without a host sync
    size_t n = 0;
    HIP_OK(hipEventRecord(ev[0], st));
    launch_z(c, 0u, 1);
    is_z[n] = 1;
    HIP_OK(hipEventRecord(ev[++n], st));
    for (int m = 0; m < p->mcmcStep; ++m) {
      for (int r = 0; r < nr; ++r) {
        launch_eta(c, r, 1u + 2u * (uint32_t)m);
        is_z[n] = 0;
        HIP_OK(hipEventRecord(ev[++n], st));
      }
      launch_z(c, 2u + 2u * (uint32_t)m, 0);
      is_z[n] = 1;
      HIP_OK(hipEventRecord(ev[++n], st));
    }
    HIP_OK(hipEventSynchronize(ev[n]));
    t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < nr; ++r) {
      const size_t ne = (size_t)p->np[r] * p->nf[r];
      HIP_OK(hipMemcpyAsync(EtaOut[r] + s0 * ne, a.Eta[r], c * ne * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    back_ms += ms_since(t0);
    for (size_t k = 0; k < n; ++k) {
      float ms = 0.f;
      HIP_OK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      (is_z[k] ? z_ms : eta_ms) += ms;
    }
  }
  g_cond_ms[0] = up_ms, g_cond_ms[1] = z_ms, g_cond_ms[2] = eta_ms, g_cond_ms[3] = back_ms;
}

}  // namespace hmsc
