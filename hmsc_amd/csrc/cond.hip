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
//
// Spatial 'Full' levels (hmsc_predict_conditional_spatial; R/updateEta.R:111-140, spatial.hip): the
// units of a level are coupled through iW, so a level is one system of N = np nf unknowns in the
// unit-fastest order, iUEta = bdiag_h(iW[g(s, h)]) + kron(LDL, diag(n_q)), LDL = Lambda diag(1 /
// sigma) Lambda^T.  Nothing in it moves during the mcmcStep loop, so it is assembled and factored
// once per (sample, level) and chunk, and the factors stay resident: an Eta step is the rhs
// (cond_eta_kernel's wave sum over all species, written straight into the level's Eta slot, which
// nothing reads while level r is updated), two triangular solves and the noise.  iW is built once
// per call for the grid values the posterior uses (spatial_full_grid).  Up to N = 1024 one
// workgroup per sample factors and solves (wg_chol, wg_forward, wg_backward_t, the samples as the
// grid); above, dense.hip's blocked routines run sample by sample on the call's stream.  R's
// spatial branch sums over all cells, so with a spatial level the Z launches draw and store the NA
// cells too (N(E, sd) by the cell's word of the quad block, R/updateZ.R:92); the other levels of
// such a model keep their masked sums.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hmsc_amd.h"
#include "common.h"
#include "devmem.h"
#include "rng.h"
#include "state.h"     // dense_potrf_lower, dense_trsv_lower, spatial_full_grid
#include "z_kernel.h"  // d4, mfma_f64, z_probit_draw, z_poisson_draw

namespace hmsc {

constexpr int CT_I = 64, CT_J = 32, COND_NF_MAX = 32;
constexpr size_t COND_SLAB_CAP = (size_t)16 << 30;  // bytes of the default chunk's Z slab
constexpr int COND_SP_WG_N = 1024;    // np nf up to which one workgroup factors a sample's system (SP_BLOCKED_N)
constexpr int COND_SP_GRID_MAX = 101; // grid values of a level (R's alphapw)

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

// NA: the NA cells are drawn and stored too (a model with a spatial level)
template <int KQ, bool NA>
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
      const bool na = y != y;
      if (na && !NA) continue;  // NA: not drawn, not stored
      const int fam = a.family[j];
      double z = y;          // normal: Z = Y   R/updateZ.R:40-41
      if (fam != 1 || (NA && na)) {
        const double is = 1.0 / sigma[j], sd = 1.0 / sqrt(is);
        if (fam == 2 || (NA && na)) {  // an NA cell of any family: N(E, sd), as z_wave_kernel
          if (!have) {
            qw = philox4x32_10(U4{(uint32_t)((size_t)i + (size_t)ny * (uint32_t)(jq >> 2)), 0u, (uint32_t)S_Z, iter}, a.key);
            have = true;
          }
          const uint32_t wd = r == 0 ? qw.x : r == 1 ? qw.y : r == 2 ? qw.z : qw.w;
          z = z_probit_draw(e[r], sd, sqrt(is), (NA && na) ? -1 : y != 0.0 ? 1 : 0, u32o(wd), 0);
        } else {
          const double zprev = first ? e[r] : Z[cell];
          z = z_poisson_draw(e[r], sd, y, zprev, uniforms(a.key, (uint32_t)cell, 0u, (uint32_t)S_ZPOIS, iter), 0);
        }
      }
      Z[cell] = z;
    }
  }
}

// SP (a spatial level): the sums run over all species (NA cells hold their draw) and the wave
// leaves fS[q, h] at Eta_r[q, h] -- the rhs of the level's system, solved in place by the launches
// that follow; unit_class and F are not read.
template <int NFB, bool SP>
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
      if (!SP && y != y) continue;
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
  if (SP) {
    if (lane < nf) a.Eta[r][((size_t)s * nf + lane) * a.np[r] + q] = sb[lane];
    return;
  }
  // y = F^-1 b; y += xi; eta = F^-T y  (= Q^-1 b + R^-1 xi, R = F^T: R/updateEta.R:56,69,90)
  const double* Fq = F + ((size_t)s * ncls + unit_class[q]) * nf * nf;
  wg_forward(Fq, nf, nf, sb);
  if (lane < nf)
    sb[lane] += normal(a.key, (uint32_t)q, (uint32_t)lane, (uint32_t)S_ETA + LEVEL_STRIDE * (uint32_t)r, cond_iter(a, s, off));
  __syncthreads();
  wg_backward_t(Fq, nf, nf, sb);
  if (lane < nf) a.Eta[r][((size_t)s * nf + lane) * a.np[r] + q] = sb[lane];
}

// ---- spatial 'Full' levels.  One sample's system: U (N x N, ld N, lower triangle), N = np nf.

// LDL[h1 + nf h2] = sum_j lambda_h1j lambda_h2j / sigma_j per sample (eta_spatial_full_kernel's sum)
__global__ __launch_bounds__(64) void cond_ldl_kernel(CondArgs a, int r, double* LDL) {
  const int s = blockIdx.x, nf = a.nf[r], ns = a.ns;
  const double* lam = a.Lambda[r] + (size_t)s * ns * nf;
  const double* sigma = a.sigma + (size_t)s * ns;
  for (int p = threadIdx.x; p < nf * nf; p += 64) {
    const int h1 = p % nf, h2 = p / nf;
    double v = 0.0;
    for (int j = 0; j < ns; ++j) v = fma(lam[h1 + (size_t)nf * j] * (1.0 / sigma[j]), lam[h2 + (size_t)nf * j], v);
    LDL[(size_t)s * nf * nf + p] = v;
  }
}

// lower triangle of iUEta = bdiag_h(iW[g(s, h)]) + kron(LDL, diag(n_q)); grid (N / 256, N, samples)
__global__ __launch_bounds__(256) void cond_sp_assemble_kernel(CondArgs a, int r, const double* iWg, const int* aidx,
                                                               const int* unit_ptr, const double* LDL, double* U) {
  const int np = a.np[r], nf = a.nf[r], N = np * nf, s = blockIdx.z;
  const int r2 = blockIdx.y, r1 = blockIdx.x * 256 + threadIdx.x;
  if (r1 >= N || r1 < r2) return;
  const int q1 = r1 % np, h1 = r1 / np, q2 = r2 % np, h2 = r2 / np;
  double v = 0.0;
  if (h1 == h2) {
    const int g = aidx[((size_t)a.s0 + s) * nf + h1];
    v = iWg[q1 + (size_t)np * q2 + (size_t)np * np * g];
  }
  if (q1 == q2) v = fma(LDL[(size_t)s * nf * nf + h1 + nf * h2], (double)(unit_ptr[q1 + 1] - unit_ptr[q1]), v);
  U[(size_t)s * N * N + r1 + (size_t)N * r2] = v;
}

// N <= 1024: a workgroup per sample factors its system in place; bad[s] is raised if it is not
// positive definite
__global__ __launch_bounds__(1024) void cond_sp_chol_kernel(int N, double* U, int* bad) {
  __shared__ int flag;
  const int s = blockIdx.x;
  if (!wg_chol(U + (size_t)s * N * N, N, N, &flag) && threadIdx.x == 0) bad[s] = 1;
}

// ... and solves: eta = L^-T (L^-1 fS + xi) in place in the level's Eta slot (R/updateEta.R:134-138)
__global__ __launch_bounds__(1024) void cond_sp_solve_kernel(CondArgs a, int r, uint32_t off, const double* U) {
  const int s = blockIdx.x, np = a.np[r], N = np * a.nf[r];
  const double* Us = U + (size_t)s * N * N;
  double* x = a.Eta[r] + (size_t)s * N;
  wg_forward(Us, N, N, x);
  const uint32_t iter = cond_iter(a, s, off);
  for (int e = threadIdx.x; e < N; e += blockDim.x)
    x[e] += normal(a.key, (uint32_t)(e % np), (uint32_t)(e / np), (uint32_t)S_ETA + LEVEL_STRIDE * (uint32_t)r, iter);
  __syncthreads();
  wg_backward_t(Us, N, N, x);
}

// the noise between the two blocked solves; grid (N / 256, samples)
__global__ __launch_bounds__(256) void cond_sp_noise_kernel(CondArgs a, int r, uint32_t off) {
  const int s = blockIdx.y, np = a.np[r], N = np * a.nf[r], e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  a.Eta[r][(size_t)s * N + e] +=
      normal(a.key, (uint32_t)(e % np), (uint32_t)(e / np), (uint32_t)S_ETA + LEVEL_STRIDE * (uint32_t)r, cond_iter(a, s, off));
}

// ---- 'GPP' levels (R/updateEta.R:148-196; launch_eta_gpp of spatial.hip with the sample as a grid
// axis).  Once per (sample, level): B1_i = (LDL + diag(idD[i, g(s, h)]))^-1 and LB1_i = chol(B1_i)
// per unit, iAW = bdiag(B1_i) W with W = bdiag_h(idDW12g[,, g(s, h)]), H = bdiag_h(Fg[,, g(s, h)]) -
// W' iAW and its factor L_H.  A step is eta = iA fS + iAW L_H^-T (L_H^-1 iAW' fS + xi2) + LiA xi1:
// the chain's T (T' fS + xi2) with T = iAW L_H^-T, as two triangular solves of one workgroup.
constexpr uint32_t COND_GPP_XI2_SUB = 1024;  // GPP_XI2_SUB of spatial.hip
constexpr int COND_GPP_NF_MAX = 16, COND_GPP_KF_MAX = 1024;

struct CondGpp {
  int nK;
  const double *idDg, *idDW12g, *Fg;  // np x G, np x nK x G, nK x nK x G over the grid values in use
  const int* aidx;                    // nsamples x nf
  double *B1, *LB1;                   // chunk x np x nf x nf
  double* iAW;                        // chunk x (np nf) x (nK nf)
  double* u;                          // chunk x (nK nf)
};

__global__ __launch_bounds__(256) void cond_gpp_unit_kernel(CondArgs a, int r, CondGpp g, const double* LDL, int* bad) {
  const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, nf = a.nf[r], np = a.np[r];
  if (i >= np) return;
  const double* ldl = LDL + (size_t)s * nf * nf;
  const int* ai = g.aidx + ((size_t)a.s0 + s) * nf;
  double A[COND_GPP_NF_MAX * COND_GPP_NF_MAX], Li[COND_GPP_NF_MAX * COND_GPP_NF_MAX];
  for (int c = 0; c < nf; ++c)
    for (int h = 0; h < nf; ++h) A[h + nf * c] = ldl[h + nf * c] + (h == c ? g.idDg[i + (size_t)np * ai[h]] : 0.0);
  bool ok = t_chol_inv(A, Li, nf);  // A <- L0 (lower), Li = L0^-1
  double* b1 = g.B1 + ((size_t)s * np + i) * nf * nf;
  double* lb = g.LB1 + ((size_t)s * np + i) * nf * nf;
  for (int c = 0; c < nf; ++c)
    for (int h = 0; h < nf; ++h) {  // B1 = L0^-T L0^-1
      double v = 0.0;
      for (int k = (h > c ? h : c); k < nf; ++k) v += Li[k + nf * h] * Li[k + nf * c];
      b1[h + nf * c] = v;
      A[h + nf * c] = v;
    }
  ok = t_chol_inv(A, Li, nf) && ok;  // A <- chol(B1)
  for (int c = 0; c < nf; ++c)
    for (int h = 0; h < nf; ++h) lb[h + nf * c] = h >= c ? A[h + nf * c] : 0.0;
  if (!ok) bad[s] = 1;
}

// iAW[e, c] = B1_i[h, h'] idDW12g[i, k, g(s, h')],  e = i + np h, c = k + nK h'; grid (NP / 256, KF, samples)
__global__ __launch_bounds__(256) void cond_gpp_iaw_kernel(CondArgs a, int r, CondGpp g) {
  const int np = a.np[r], nf = a.nf[r], nK = g.nK, NP = np * nf, KF = nK * nf, s = blockIdx.z;
  const int e = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (e >= NP) return;
  const int i = e % np, h = e / np, k = c % nK, h2 = c / nK;
  const double w = g.idDW12g[i + (size_t)np * k + (size_t)np * nK * g.aidx[((size_t)a.s0 + s) * nf + h2]];
  g.iAW[(size_t)s * NP * KF + e + (size_t)NP * c] = g.B1[((size_t)s * np + i) * nf * nf + h + nf * h2] * w;
}

// H = bdiag_h(Fg[,, g(s, h)]) - W' iAW, one workgroup per entry of the lower triangle; grid (KF, KF, samples)
__global__ __launch_bounds__(256) void cond_gpp_h_kernel(CondArgs a, int r, CondGpp g, double* H) {
  const int np = a.np[r], nf = a.nf[r], nK = g.nK, NP = np * nf, KF = nK * nf, s = blockIdx.z;
  const int c1 = blockIdx.x, c2 = blockIdx.y, k = c1 % nK, h = c1 / nK;
  if (c1 < c2) return;  // (uniform)
  const int gh = g.aidx[((size_t)a.s0 + s) * nf + h];
  const double* w = g.idDW12g + (size_t)np * k + (size_t)np * nK * gh;
  const double* x = g.iAW + (size_t)s * NP * KF + (size_t)np * h + (size_t)NP * c2;
  double v = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) v = fma(w[i], x[i], v);
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int k2 = c2 % nK, h2 = c2 / nK;
    const double f = h == h2 ? g.Fg[k + (size_t)nK * k2 + (size_t)nK * nK * gh] : 0.0;
    H[(size_t)s * KF * KF + c1 + (size_t)KF * c2] = f - ((red[0] + red[1]) + (red[2] + red[3]));
  }
}

// u[c] = iAW[, c]' fS, fS in the level's Eta slot; grid (KF, samples)
__global__ __launch_bounds__(256) void cond_gpp_u_kernel(CondArgs a, int r, CondGpp g) {
  const int NP = a.np[r] * a.nf[r], KF = g.nK * a.nf[r], c = blockIdx.x, s = blockIdx.y;
  const double* col = g.iAW + (size_t)s * NP * KF + (size_t)NP * c;
  const double* fS = a.Eta[r] + (size_t)s * NP;
  double v = 0.0;
  for (int e = threadIdx.x; e < NP; e += 256) v = fma(col[e], fS[e], v);
  __shared__ double red[4];
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) g.u[(size_t)s * KF + c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// u <- L_H^-T (L_H^-1 u + xi2), a workgroup per sample
__global__ __launch_bounds__(1024) void cond_gpp_solve_kernel(CondArgs a, int r, uint32_t off, CondGpp g, const double* H) {
  const int s = blockIdx.x, nK = g.nK, KF = nK * a.nf[r];
  const double* Hs = H + (size_t)s * KF * KF;
  double* x = g.u + (size_t)s * KF;
  wg_forward(Hs, KF, KF, x);
  const uint32_t iter = cond_iter(a, s, off);
  for (int c = threadIdx.x; c < KF; c += blockDim.x)
    x[c] += normal(a.key, (uint32_t)(c % nK), COND_GPP_XI2_SUB + (uint32_t)(c / nK),
                   (uint32_t)S_ETA + LEVEL_STRIDE * (uint32_t)r, iter);
  __syncthreads();
  wg_backward_t(Hs, KF, KF, x);
}

// eta_i = B1_i fS_i + LB1_i xi1_i + iAW[i, ] u, a thread per unit (it reads fS_i before it writes eta_i)
__global__ __launch_bounds__(256) void cond_gpp_eta_kernel(CondArgs a, int r, uint32_t off, CondGpp g) {
  const int np = a.np[r], nf = a.nf[r], NP = np * nf, KF = g.nK * nf, s = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  double* x = a.Eta[r] + (size_t)s * NP;
  const double* b1 = g.B1 + ((size_t)s * np + i) * nf * nf;
  const double* lb = g.LB1 + ((size_t)s * np + i) * nf * nf;
  const double* aw = g.iAW + (size_t)s * NP * KF;
  const double* u = g.u + (size_t)s * KF;
  const uint32_t iter = cond_iter(a, s, off);
  double f[COND_GPP_NF_MAX], xi[COND_GPP_NF_MAX], out[COND_GPP_NF_MAX];
  for (int h = 0; h < nf; ++h) {
    f[h] = x[i + (size_t)np * h];
    xi[h] = normal(a.key, (uint32_t)i, (uint32_t)h, (uint32_t)S_ETA + LEVEL_STRIDE * (uint32_t)r, iter);
  }
  for (int h = 0; h < nf; ++h) {
    double v = 0.0;
    for (int h2 = 0; h2 < nf; ++h2) v = fma(b1[h + nf * h2], f[h2], v);
    for (int h2 = 0; h2 <= h; ++h2) v = fma(lb[h + nf * h2], xi[h2], v);
    for (int c = 0; c < KF; ++c) v = fma(aw[i + (size_t)np * h + (size_t)NP * c], u[c], v);
    out[h] = v;
  }
  for (int h = 0; h < nf; ++h) x[i + (size_t)np * h] = out[h];
}

static thread_local double g_cond_ms[4] = {0.0, 0.0, 0.0, 0.0};
void cond_last_timing(double out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = g_cond_ms[k];
}

void run_cond(const hmsc_cond_args* p, const hmsc_cond_spatial* sp, double* const* EtaOut) {
  for (int k = 0; k < 4; ++k) g_cond_ms[k] = 0.0;
  const auto spatial = [&](int r) { return sp != nullptr && sp[r].method != 0; };
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
  bool any_sp = false;  // a spatial level: the Z launches store the NA cells too
  for (int r = 0; r < nr; ++r) {
    HMSC_REQUIRE(p->nf[r] >= 1 && p->np[r] >= 1, "hmsc_predict_conditional: every level needs nf >= 1 and np >= 1");
    HMSC_REQUIRE(p->nf[r] <= COND_NF_MAX, "hmsc_predict_conditional: nf = " + std::to_string(p->nf[r]) + " of level " +
                                              std::to_string(r) + " exceeds 32");
    HMSC_REQUIRE(p->Eta[r] && p->Lambda[r] && EtaOut[r], "hmsc_predict_conditional: NULL Eta / Lambda / EtaOut");
    K += p->nf[r];
    if (!spatial(r)) {
      HMSC_REQUIRE(p->ncls[r] >= 1 && p->cnt[r] && p->unit_class[r], "hmsc_predict_conditional: NULL cnt / unit_class");
      continue;
    }
    const hmsc_cond_spatial& q = sp[r];
    const std::string lev = " of level " + std::to_string(r);
    HMSC_REQUIRE(q.method != 2, "hmsc_predict_conditional: spatial method 2 (NNGP)" + lev + " is not served: its factor "
                                "lives in the chain's band order");
    HMSC_REQUIRE(q.method == 1 || q.method == 3,
                 "hmsc_predict_conditional: unknown spatial method " + std::to_string(q.method) + lev);
    HMSC_REQUIRE(q.nalpha >= 1 && q.nalpha <= COND_SP_GRID_MAX && q.AlphaIdx,
                 "hmsc_predict_conditional: 1 .. 101 grid values in use and AlphaIdx are needed" + lev);
    if (q.method == 1) {
      HMSC_REQUIRE((q.coords != nullptr) != (q.dist != nullptr) && (q.dist || q.sDim >= 1),
                   "hmsc_predict_conditional: a 'Full' level takes coordinates with sDim >= 1 or a distance matrix" + lev);
      HMSC_REQUIRE(q.alphas != nullptr, "hmsc_predict_conditional: NULL alphas" + lev);
      for (int g = 0; g < q.nalpha; ++g)
        HMSC_REQUIRE(std::isfinite(q.alphas[g]) && q.alphas[g] >= 0.0,
                     "hmsc_predict_conditional: grid value " + std::to_string(g) + lev + " is not finite and non-negative");
      HMSC_REQUIRE((size_t)p->np[r] * p->nf[r] <= 65535, "hmsc_predict_conditional: np * nf" + lev + " exceeds 65535");
    } else {
      HMSC_REQUIRE(q.nK >= 1 && q.idDg && q.idDW12g && q.Fg, "hmsc_predict_conditional: a 'GPP' level needs nK >= 1 and "
                                                             "idDg / idDW12g / Fg" + lev);
      HMSC_REQUIRE(p->nf[r] <= COND_GPP_NF_MAX, "hmsc_predict_conditional: nf = " + std::to_string(p->nf[r]) +
                                                    " of the 'GPP' level " + std::to_string(r) + " exceeds 16");
      HMSC_REQUIRE((size_t)q.nK * p->nf[r] <= COND_GPP_KF_MAX,
                   "hmsc_predict_conditional: nK * nf = " + std::to_string((size_t)q.nK * p->nf[r]) + " of the 'GPP' level " +
                       std::to_string(r) + " exceeds 1024");
      HMSC_REQUIRE(p->np[r] == p->ny, "hmsc_predict_conditional: the 'GPP' level " + std::to_string(r) +
                                          " needs one row per unit (np = " + std::to_string(p->np[r]) + ", ny = " +
                                          std::to_string(p->ny) + ")");
    }
    for (size_t k = 0; k < S * p->nf[r]; ++k)
      HMSC_REQUIRE(q.AlphaIdx[k] >= 0 && q.AlphaIdx[k] < q.nalpha,
                   "hmsc_predict_conditional: grid index " + std::to_string(q.AlphaIdx[k]) + " of sample " +
                       std::to_string(k / p->nf[r]) + ", factor " + std::to_string(k % p->nf[r]) + lev +
                       " is outside the " + std::to_string(q.nalpha) + " grid values in use");
    any_sp = true;
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
    if (spatial(r)) {  // (its factor is sized below)
      for (size_t q = 0; q < npr && sp[r].method == 3; ++q)
        HMSC_REQUIRE(uptr[r][q + 1] - uptr[r][q] == 1, "hmsc_predict_conditional: the 'GPP' level " + std::to_string(r) +
                                                           " needs one row per unit (unit " + std::to_string(q) + " has " +
                                                           std::to_string(uptr[r][q + 1] - uptr[r][q]) + ")");
      continue;
    }
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
    if (spatial(r)) continue;
    dCls[r] = own.upload(p->unit_class[r], (size_t)p->np[r], st);
    dCnt[r] = own.upload(p->cnt[r], (size_t)p->ncls[r] * ns, st);
  }
  int* dBad = own.alloc<int>(1);
  // spatial levels: the index table of every sample and, once per call (before the chunk is
  // sized: the free memory below is what they leave), the grid arrays of the values in use -- a
  // 'Full' level's iW, built here, a 'GPP' level's low-rank arrays, uploaded
  const double* dIW[HMSC_MAX_LEVELS] = {};
  const int* dAidx[HMSC_MAX_LEVELS] = {};
  int spN[HMSC_MAX_LEVELS] = {};  // order of a sample's dense system: np nf ('Full'), nK nf ('GPP')
  CondGpp gpp[HMSC_MAX_LEVELS] = {};
  const auto is_gpp = [&](int r) { return spatial(r) && sp[r].method == 3; };
  int* dSync = nullptr;
  for (int r = 0; r < nr; ++r) {
    if (!spatial(r)) continue;
    const hmsc_cond_spatial& q = sp[r];
    const size_t npr = p->np[r], n2 = npr * npr;
    dAidx[r] = own.upload(q.AlphaIdx, S * p->nf[r], st);
    if (is_gpp(r)) {
      const size_t nK = q.nK, G = q.nalpha;
      spN[r] = (int)(nK * p->nf[r]);
      gpp[r].nK = q.nK;
      gpp[r].idDg = own.upload(q.idDg, npr * G, st);
      gpp[r].idDW12g = own.upload(q.idDW12g, npr * nK * G, st);
      gpp[r].Fg = own.upload(q.Fg, nK * nK * G, st);
      gpp[r].aidx = dAidx[r];
      continue;
    }
    spN[r] = (int)(npr * p->nf[r]);
    const double* geo = q.coords ? own.upload(q.coords, npr * q.sDim, st) : own.upload(q.dist, n2, st);
    double* iW = own.alloc<double>(n2 * q.nalpha);
    double* RiW = own.alloc<double>(n2 * q.nalpha);
    double* det = own.alloc<double>(q.nalpha);
    spatial_full_grid(st, (int)npr, q.coords ? q.sDim : 0, q.coords ? geo : nullptr, q.coords ? nullptr : geo, q.alphas,
                      q.nalpha, iW, RiW, det, dBad);
    int bad = 0;
    copy_sync(&bad, dBad, sizeof(int), hipMemcpyDeviceToHost, st);
    HMSC_REQUIRE(bad == 0, "hmsc_predict_conditional: a grid matrix of level " + std::to_string(r) +
                               " is not positive definite");
    own.free(RiW);
    own.free(det);
    own.free(const_cast<double*>(geo));
    dIW[r] = iW;
    if (spN[r] > COND_SP_WG_N && !dSync) dSync = own.alloc<int>(DENSE_SYNC_INTS);  // the dense handshake block, zeroed
  }
  // samples resident at once: the Z slab, the stacks and the factors of a chunk.  The caller's
  // count, else what fits in 3/4 of the free device memory with the slab capped at 16 GiB.
  size_t per = ny * ns + nc * ns + ns + ((size_t)K + 1) * ns + fac_per;
  for (int r = 0; r < nr; ++r) per += (size_t)p->nf[r] * ((size_t)p->np[r] + ns);
  for (int r = 0; r < nr; ++r) {  // a spatial level's factor, the blocked routines' workspace, LDL
    if (!spatial(r)) continue;
    per += (size_t)spN[r] * spN[r] + (spN[r] > COND_SP_WG_N ? dense_ws_doubles(spN[r]) : 0) + (size_t)p->nf[r] * p->nf[r];
    if (is_gpp(r))  // iAW, B1 and LB1, u
      per += (size_t)p->np[r] * p->nf[r] * (spN[r] + 2 * (size_t)p->nf[r]) + spN[r];
  }
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
  double *dLam[HMSC_MAX_LEVELS] = {}, *dF[HMSC_MAX_LEVELS] = {}, *dLDL[HMSC_MAX_LEVELS] = {}, *dWs[HMSC_MAX_LEVELS] = {};
  for (int r = 0; r < nr; ++r) {
    a.Eta[r] = own.alloc<double>(chunk * p->np[r] * p->nf[r]);
    dLam[r] = own.alloc<double>(chunk * p->nf[r] * ns);
    a.Lambda[r] = dLam[r];
    if (!spatial(r)) {
      dF[r] = own.alloc<double>(chunk * p->ncls[r] * p->nf[r] * p->nf[r]);
      continue;
    }
    dF[r] = own.alloc<double>(chunk * spN[r] * spN[r]);  // the sample's system, then its factor
    dLDL[r] = own.alloc<double>(chunk * p->nf[r] * p->nf[r]);
    if (spN[r] > COND_SP_WG_N) dWs[r] = own.alloc<double>(chunk * dense_ws_doubles(spN[r]));
    if (is_gpp(r)) {
      const size_t NP = (size_t)p->np[r] * p->nf[r];
      gpp[r].B1 = own.alloc<double>(chunk * NP * p->nf[r]);
      gpp[r].LB1 = own.alloc<double>(chunk * NP * p->nf[r]);
      gpp[r].iAW = own.alloc<double>(chunk * NP * spN[r]);
      gpp[r].u = own.alloc<double>(chunk * spN[r]);
    }
  }
  int* dBadS = any_sp ? own.alloc<int>(chunk) : nullptr;  // per sample: a spatial system is not positive definite
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
    auto* kern = KQ == 2 ? (any_sp ? cond_z_kernel<2, true> : cond_z_kernel<2, false>)
                 : KQ == 8 ? (any_sp ? cond_z_kernel<8, true> : cond_z_kernel<8, false>)
                 : KQ == 16 ? (any_sp ? cond_z_kernel<16, true> : cond_z_kernel<16, false>)
                            : (any_sp ? cond_z_kernel<32, true> : cond_z_kernel<32, false>);
    kern<<<grid, 256, zsmem, st>>>(a, off, first);
    HIP_OK(hipGetLastError());
  };
  auto launch_eta = [&](size_t c, int r, uint32_t off) {
    const dim3 grid((unsigned)p->np[r], (unsigned)c);
    const size_t smem = (size_t)(K + COND_NF_MAX) * sizeof(double);
    const int nf = p->nf[r];
    if (!spatial(r)) {
      if (nf <= 8) cond_eta_kernel<8, false><<<grid, 64, smem, st>>>(a, r, off, p->ncls[r], dPtr[r], dRows[r], dCls[r], dF[r]);
      else if (nf <= 16) cond_eta_kernel<16, false><<<grid, 64, smem, st>>>(a, r, off, p->ncls[r], dPtr[r], dRows[r], dCls[r], dF[r]);
      else cond_eta_kernel<32, false><<<grid, 64, smem, st>>>(a, r, off, p->ncls[r], dPtr[r], dRows[r], dCls[r], dF[r]);
      HIP_OK(hipGetLastError());
      return;
    }
    // a spatial level: the rhs into the Eta slot, then eta = L^-T (L^-1 fS + xi) in place
    if (nf <= 8) cond_eta_kernel<8, true><<<grid, 64, smem, st>>>(a, r, off, 0, dPtr[r], dRows[r], nullptr, nullptr);
    else if (nf <= 16) cond_eta_kernel<16, true><<<grid, 64, smem, st>>>(a, r, off, 0, dPtr[r], dRows[r], nullptr, nullptr);
    else cond_eta_kernel<32, true><<<grid, 64, smem, st>>>(a, r, off, 0, dPtr[r], dRows[r], nullptr, nullptr);
    HIP_OK(hipGetLastError());
    const int N = spN[r];
    if (is_gpp(r)) {
      cond_gpp_u_kernel<<<dim3((unsigned)N, (unsigned)c), 256, 0, st>>>(a, r, gpp[r]);
      cond_gpp_solve_kernel<<<(unsigned)c, 1024, 0, st>>>(a, r, off, gpp[r], dF[r]);
      cond_gpp_eta_kernel<<<dim3((unsigned)((p->np[r] + 255) / 256), (unsigned)c), 256, 0, st>>>(a, r, off, gpp[r]);
      HIP_OK(hipGetLastError());
      return;
    }
    if (N <= COND_SP_WG_N) {
      cond_sp_solve_kernel<<<(unsigned)c, 1024, 0, st>>>(a, r, off, dF[r]);
      HIP_OK(hipGetLastError());
      return;
    }
    const size_t wsd = dense_ws_doubles(N);
    for (size_t s = 0; s < c; ++s)
      dense_trsv_lower(st, dF[r] + s * N * N, N, N, a.Eta[r] + s * N, 0, dWs[r] + s * wsd, 0, dSync);
    cond_sp_noise_kernel<<<dim3((unsigned)((N + 255) / 256), (unsigned)c), 256, 0, st>>>(a, r, off);
    HIP_OK(hipGetLastError());
    for (size_t s = 0; s < c; ++s)
      dense_trsv_lower(st, dF[r] + s * N * N, N, N, a.Eta[r] + s * N, 1, dWs[r] + s * wsd, 0, dSync);
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
      if (spatial(r)) {  // the sample's system and its factor, resident for the chunk
        const int N = spN[r];
        cond_ldl_kernel<<<(unsigned)c, 64, 0, st>>>(a, r, dLDL[r]);
        if (is_gpp(r)) {
          const unsigned g1 = (unsigned)(((size_t)p->np[r] * nf + 255) / 256);
          cond_gpp_unit_kernel<<<dim3((unsigned)((p->np[r] + 255) / 256), (unsigned)c), 256, 0, st>>>(a, r, gpp[r], dLDL[r],
                                                                                                 dBadS);
          cond_gpp_iaw_kernel<<<dim3(g1, (unsigned)N, (unsigned)c), 256, 0, st>>>(a, r, gpp[r]);
          cond_gpp_h_kernel<<<dim3((unsigned)N, (unsigned)N, (unsigned)c), 256, 0, st>>>(a, r, gpp[r], dF[r]);
        } else {
          cond_sp_assemble_kernel<<<dim3((unsigned)((N + 255) / 256), (unsigned)N, (unsigned)c), 256, 0, st>>>(
              a, r, dIW[r], dAidx[r], dPtr[r], dLDL[r], dF[r]);
        }
        HIP_OK(hipGetLastError());
        if (N <= COND_SP_WG_N) {  // (always, for a 'GPP' level's H)
          cond_sp_chol_kernel<<<(unsigned)c, 1024, 0, st>>>(N, dF[r], dBadS);
          HIP_OK(hipGetLastError());
        } else {
          for (size_t s = 0; s < c; ++s)
            dense_potrf_lower(st, dF[r] + s * N * N, N, N, dWs[r] + s * dense_ws_doubles(N), dBadS + s, 0, dSync);
        }
        std::vector<int> bs(c);
        HIP_OK(hipMemcpyAsync(bs.data(), dBadS, c * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (size_t s = 0; s < c; ++s)
          HMSC_REQUIRE(bs[s] == 0, "hmsc_predict_conditional: the spatial system (iUEta of a 'Full' level, the unit "
                                   "blocks or H of a 'GPP' level) of sample " + std::to_string(s0 + s) + ", level " +
                                       std::to_string(r) + " is not positive definite");
        continue;
      }
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
    int hs = 0;
    if (dSync) HIP_OK(hipMemcpyAsync(&hs, dSync + DENSE_SYNC_ERR, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    HMSC_REQUIRE(hs == 0, "hmsc_predict_conditional: an in-launch handshake of the blocked Cholesky timed out (error "
                          "bits " + std::to_string(hs) + ")");
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
