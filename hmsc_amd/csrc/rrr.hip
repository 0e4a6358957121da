// Reduced-rank regression covariates on gfx950: updatewRRR (R/updatewRRR.R), updatewRRRPriors
// (R/updatewRRRPriors.R), their initial draws (R/computeInitialParameters.R:20-27) and the
// refresh of everything the chain derives from the design matrix, whose last ncRRR columns
// are XRRR wRRR^T (R/updatewRRR.R:62-73).
//
// updatewRRR samples vec(wRRR) (element e = k + ncRRR c) from N(iU^-1 mu1, iU^-1) with
//   iU  = diag(vec(PsiRRR o tau)) + kron(XRRR^T XRRR, A1),  A1 = BetaRRR D BetaRRR^T   (:49-54)
//   mu1 = vec(BetaRRR D S^T XRRR),  S = Z - LFix - LRan,  D = diag(iSigma)            (:44-57)
// The one large operand is Z (ny x ns).  With C1 = BetaRRR D BL^T (ncRRR x K; BL = [Beta;
// Lambda_1; ...], so A1 is its RRR columns) and XEta = [X, Eta_1[Pi_1,], ...]
//   mu1 = (Z W)^T-contracted-with-XRRR - sum over the K - ncRRR other columns kappa of
//         C1[, kappa] (XEta[, kappa]^T XRRR),      W = D BetaRRR^T  (ns x ncRRR)
// so one pass streams Z (rrr_z_kernel: T = Z W per site, contracted with XRRR while the tile
// is on chip), the same launch contracts XEta's Eta columns with XRRR, X_A^T XRRR and
// XRRR^T XRRR are constants of the model, and everything else is small: one workgroup
// (rrr_draw_kernel) forms C1, mu1 and iU, factors it and draws.
//
// Deviation from Hmsc 3.0-4: R/updatewRRR.R:43 subtracts LRan only when nr > 1, so with one
// random level the reference samples from the wrong conditional; LRan is subtracted for
// every nr >= 1 here.
//
// Every sum is taken in a fixed order (per-workgroup partials, then slab_sum_body): no
// floating-point atomics, so a graph replay repeats an eager sweep bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "rng.h"
#include "state.h"

namespace hmsc {

// the Z pass' tile: RRR_TS sites (one per thread, loads coalesced along sites) by RRR_SC species
// per workgroup; the grid is (site tiles) x (species chunks + groups of RRR_MAX_K Eta columns)
constexpr int RRR_TS = 256;
constexpr int RRR_SC = 64;
constexpr int RRR_JS = 4;  // species stripes of C1's sums in rrr_draw_kernel

int rrr_tile_sites() { return RRR_TS; }
int rrr_tile_species() { return RRR_SC; }

static int rrr_ntile(const State& s) { return (s.ny + RRR_TS - 1) / RRR_TS; }
static int rrr_nchunk(const State& s) { return (s.nsl + RRR_SC - 1) / RRR_SC; }

size_t rrr_part_doubles(const State& s) {
  return (size_t)rrr_ntile(s) * ((size_t)rrr_nchunk(s) * s.ncRRR * s.ncORRR + (size_t)std::max(1, s.NFmax) * s.ncORRR);
}

// rrrWork: Mraw (n) | EtR (NFmax ncORRR) | C1 (ncRRR Kmax) | its stripes (RRR_JS ncRRR Kmax) | mu (n) | iU (n n)
struct RrrWork {
  double *Mraw, *EtR, *C1, *red, *mu, *iU;
};
static RrrWork rrr_work(const State& s) {
  const size_t n = (size_t)s.ncRRR * s.ncORRR;
  RrrWork w;
  w.Mraw = s.rrrWork;
  w.EtR = w.Mraw + n;
  w.C1 = w.EtR + (size_t)std::max(1, s.NFmax) * s.ncORRR;
  w.red = w.C1 + (size_t)s.ncRRR * s.Kmax;
  w.mu = w.red + (size_t)RRR_JS * s.ncRRR * s.Kmax;
  w.iU = w.mu + n;
  return w;
}
size_t rrr_work_doubles(const State& s) {
  const size_t n = (size_t)s.ncRRR * s.ncORRR;
  return 2 * n + n * n + (size_t)std::max(1, s.NFmax) * s.ncORRR + (size_t)(1 + RRR_JS) * s.ncRRR * s.Kmax + 16;
}

// ---------------------------------------------------------------------------
// The pass over Z.  Workgroup (tile, cy):
//   cy < nchunk   T[i, k] = sum_{j in chunk cy} Z[i, j] iSigma[j] BetaRRR[k, j] for its sites i
//   cy >= nchunk  T[i, k] = XEta[i, nc + 8 (cy - nchunk) + k]  (Eta columns, RRR_MAX_K at a time)
// then out[k, c] = sum_{i in tile} T[i, k] XRRR[i, c]: wave w takes columns c = w, w + 4, ...,
// its lanes the tile's sites (coalesced), combined by a butterfly (the same order every run).
// Z holds the imputed values at NA cells (R/updateZ.R:92), so no mask is applied, as in R.
// ---------------------------------------------------------------------------
struct RrrZArgs {
  const double* Z;
  const double* BL;
  const double* iSigma;
  const double* XRRR;
  const double* XEta;
  int ny, ns, K, nc, ncN, ncRRR, ncORRR, NF, nchunk;
  double* partZ;  // [tile][chunk][k + ncRRR c]
  double* partE;  // [tile][h + NF c]
};

__global__ __launch_bounds__(256) void rrr_z_kernel(RrrZArgs a) {
  __shared__ double sW[RRR_SC * RRR_MAX_K];  // [species of the chunk][k]
  __shared__ double sT[RRR_MAX_K][RRR_TS];
  const int t = threadIdx.x, tile = blockIdx.x, cy = blockIdx.y;
  const int i = tile * RRR_TS + t;
  const bool in = i < a.ny;
  int nk, ldk;
  double* out;
  if (cy < a.nchunk) {
    const int j0 = cy * RRR_SC, jn = min(RRR_SC, a.ns - j0);
    nk = a.ncRRR;
    for (int p = t; p < jn * nk; p += 256) {
      const int jj = p / nk, k = p - jj * nk;
      sW[jj * RRR_MAX_K + k] = a.iSigma[j0 + jj] * a.BL[a.ncN + k + (size_t)a.K * (j0 + jj)];
    }
    __syncthreads();
    double acc[RRR_MAX_K];
#pragma unroll
    for (int k = 0; k < RRR_MAX_K; ++k) acc[k] = 0.0;
    if (in) {
      const double* z = a.Z + i + (size_t)a.ny * j0;
      int jj = 0;
      for (; jj + 8 <= jn; jj += 8) {  // eight columns' loads in flight per lane
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = z[(size_t)a.ny * (jj + u)];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int k = 0; k < RRR_MAX_K; ++k)
            if (k < nk) acc[k] = fma(v[u], sW[(jj + u) * RRR_MAX_K + k], acc[k]);
      }
      for (; jj < jn; ++jj) {
        const double v = z[(size_t)a.ny * jj];
#pragma unroll
        for (int k = 0; k < RRR_MAX_K; ++k)
          if (k < nk) acc[k] = fma(v, sW[jj * RRR_MAX_K + k], acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < RRR_MAX_K; ++k) sT[k][t] = acc[k];
    out = a.partZ + ((size_t)tile * a.nchunk + cy) * ((size_t)nk * a.ncORRR);
    ldk = nk;
  } else {
    const int h0 = (cy - a.nchunk) * RRR_MAX_K;
    nk = min(RRR_MAX_K, a.NF - h0);
#pragma unroll
    for (int k = 0; k < RRR_MAX_K; ++k)
      sT[k][t] = (in && k < nk) ? a.XEta[i + (size_t)a.ny * (a.nc + h0 + k)] : 0.0;
    out = a.partE + (size_t)tile * ((size_t)a.NF * a.ncORRR) + h0;
    ldk = a.NF;
  }
  __syncthreads();
  const int lane = t & 63, w = t >> 6;
  for (int c = w; c < a.ncORRR; c += 4) {
    double acc[RRR_MAX_K];
#pragma unroll
    for (int k = 0; k < RRR_MAX_K; ++k) acc[k] = 0.0;
#pragma unroll
    for (int q = 0; q < RRR_TS / 64; ++q) {
      const int ii = lane + 64 * q, i2 = tile * RRR_TS + ii;
      const double x = i2 < a.ny ? a.XRRR[i2 + (size_t)a.ny * c] : 0.0;
#pragma unroll
      for (int k = 0; k < RRR_MAX_K; ++k)
        if (k < nk) acc[k] = fma(sT[k][ii], x, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < RRR_MAX_K; ++k)
      if (k < nk) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) out[k + (size_t)ldk * c] = v;
      }
  }
}

// ---------------------------------------------------------------------------
// The small algebra of updatewRRR, one workgroup (R/updatewRRR.R:49-60).
// ---------------------------------------------------------------------------
struct RrrDrawArgs {
  const double *BL, *iSigma, *XAtXR, *XRtXR, *PsiRRR, *DeltaRRR, *Mraw, *EtR;
  double *C1, *red, *mu, *iU, *wRRR;
  int ns, K, nc, ncN, ncRRR, ncORRR, NF;
  Key key;
  uint32_t iter;
  const uint32_t* iter_dev;
  int noise_zero;
  int* fail;
};

__global__ __launch_bounds__(256) void rrr_draw_kernel(RrrDrawArgs a) {
  __shared__ double tau[RRR_MAX_K];
  __shared__ int flag;
  const int t = threadIdx.x, nk = a.ncRRR, nco = a.ncORRR, n = nk * nco, K = a.K, O = nk * K;
  const uint32_t iter = SWEEP_ITER(a);
  // C1 = BetaRRR D BL^T (nk x K), species in RRR_JS stripes summed in stripe order
  for (int p = t; p < O * RRR_JS; p += 256) {
    const int o = p % O, js = p / O, k = o % nk, kap = o / nk;
    double v = 0.0;
    for (int j = js; j < a.ns; j += RRR_JS)
      v = fma(a.BL[a.ncN + k + (size_t)K * j] * a.iSigma[j], a.BL[kap + (size_t)K * j], v);
    a.red[(size_t)js * O + o] = v;
  }
  if (t == 0) {  // tau = cumprod(DeltaRRR)   (:52)
    double c = 1.0;
    for (int k = 0; k < nk; ++k) {
      c *= a.DeltaRRR[k];
      tau[k] = c;
    }
  }
  __syncthreads();
  for (int o = t; o < O; o += 256) {
    double v = 0.0;
    for (int js = 0; js < RRR_JS; ++js) v += a.red[(size_t)js * O + o];
    a.C1[o] = v;
  }
  __syncthreads();
  // mu1 = vec(BetaRRR D S^T XRRR)   (:57): the Z pass' sum less LFix' and LRan's shares
  for (int e = t; e < n; e += 256) {
    const int k = e % nk, c = e / nk;
    double v = a.Mraw[e];
    for (int q = 0; q < a.ncN; ++q) v -= a.C1[k + nk * q] * a.XAtXR[q + a.ncN * c];
    for (int f = 0; f < a.NF; ++f) v -= a.C1[k + nk * (a.nc + f)] * a.EtR[f + a.NF * c];
    a.mu[e] = v;
  }
  // iU = diag(vec(PsiRRR o tau)) + kron(XRRR^T XRRR, A1)   (:49-54)
  for (int p = t; p < n * n; p += 256) {
    const int e1 = p % n, e2 = p / n, k1 = e1 % nk, c1 = e1 / nk, k2 = e2 % nk, c2 = e2 / nk;
    double v = a.XRtXR[c1 + nco * c2] * a.C1[k1 + nk * (a.ncN + k2)];
    if (e1 == e2) v += a.PsiRRR[e1] * tau[k1];
    a.iU[e1 + (size_t)n * e2] = v;
  }
  __syncthreads();
  if (!wg_chol(a.iU, n, n, &flag) && t == 0) a.fail[0] = 1;  // iU = L L^T, RiU = L^T   (:55)
  // we = U mu1 + RiU^-1 xi = L^-T (L^-1 mu1 + xi)   (:56-59)
  wg_forward(a.iU, n, n, a.mu);
  if (!a.noise_zero)
    for (int e = t; e < n; e += 256) a.mu[e] += normal(a.key, (uint32_t)e, 0, S_WRRR, iter);
  __syncthreads();
  wg_backward_t(a.iU, n, n, a.mu);
  for (int e = t; e < n; e += 256) a.wRRR[e] = a.mu[e];
}

// ---------------------------------------------------------------------------
// After wRRR changed: X[, ncN + k] = XRRR wRRR[k, ]^T (R/updatewRRR.R:64-67) and the blocks
// of XX = X^T X that touch those columns, from the two constant cross-products:
//   XX[a, ncN + k] = (X_A^T XRRR) wRRR[k, ]^T,   XX[ncN + k, ncN + k'] = wRRR[k, ] (XRRR^T XRRR) wRRR[k', ]^T
// (the last workgroup).  V0gXX and V0gXXV0g are not read by any kernel.
// ---------------------------------------------------------------------------
struct RrrRefreshArgs {
  const double *XRRR, *wRRR, *XAtXR, *XRtXR;
  double *X, *XX;
  int ny, nc, ncN, ncRRR, ncORRR;
};

__global__ __launch_bounds__(256) void rrr_refresh_kernel(RrrRefreshArgs a) {
  __shared__ double sw[RRR_MAX_N];
  __shared__ double sv[RRR_MAX_N];
  const int t = threadIdx.x, nk = a.ncRRR, nco = a.ncORRR, n = nk * nco;
  for (int e = t; e < n; e += 256) sw[e] = a.wRRR[e];
  __syncthreads();
  if (blockIdx.x + 1 < gridDim.x) {
    const int i = blockIdx.x * 256 + t;
    if (i >= a.ny) return;
    double acc[RRR_MAX_K];
#pragma unroll
    for (int k = 0; k < RRR_MAX_K; ++k) acc[k] = 0.0;
    for (int c = 0; c < nco; ++c) {
      const double x = a.XRRR[i + (size_t)a.ny * c];
#pragma unroll
      for (int k = 0; k < RRR_MAX_K; ++k)
        if (k < nk) acc[k] = fma(x, sw[k + nk * c], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < RRR_MAX_K; ++k)
      if (k < nk) a.X[i + (size_t)a.ny * (a.ncN + k)] = acc[k];
    return;
  }
  const int nc = a.nc, ncN = a.ncN;
  for (int p = t; p < ncN * nk; p += 256) {
    const int q = p % ncN, k = p / ncN;
    double v = 0.0;
    for (int c = 0; c < nco; ++c) v = fma(a.XAtXR[q + ncN * c], sw[k + nk * c], v);
    a.XX[q + nc * (ncN + k)] = v;
    a.XX[(ncN + k) + nc * q] = v;
  }
  for (int p = t; p < n; p += 256) {  // V[c, k] = sum_c' (XRRR^T XRRR)[c, c'] wRRR[k, c']
    const int c = p % nco, k = p / nco;
    double v = 0.0;
    for (int c2 = 0; c2 < nco; ++c2) v = fma(a.XRtXR[c + nco * c2], sw[k + nk * c2], v);
    sv[p] = v;
  }
  __syncthreads();
  for (int p = t; p < nk * nk; p += 256) {
    const int k1 = p % nk, k2 = p / nk;
    if (k1 > k2) continue;
    double v = 0.0;
    for (int c = 0; c < nco; ++c) v = fma(sw[k1 + nk * c], sv[c + nco * k2], v);
    a.XX[(ncN + k1) + nc * (ncN + k2)] = v;
    a.XX[(ncN + k2) + nc * (ncN + k1)] = v;
  }
}

// ---------------------------------------------------------------------------
// updatewRRRPriors (R/updatewRRRPriors.R:3-27; its ns is ncORRR, its nf ncRRR) and the initial
// draws (R/computeInitialParameters.R:20-26), one workgroup each.  Gamma variates: psi of
// element e = k + ncRRR c is gamma(e, S_PSI_RRR), delta of component h gamma(h, S_DELTA_RRR).
// ---------------------------------------------------------------------------
struct RrrPriorArgs {
  double *wRRR, *PsiRRR, *DeltaRRR;
  int ncRRR, ncORRR;
  double nu, a1, b1, a2, b2;
  Key key;
  uint32_t iter;
  const uint32_t* iter_dev;
};

__global__ __launch_bounds__(256) void rrr_priors_kernel(RrrPriorArgs a) {
  __shared__ double sM[RRR_MAX_N];
  __shared__ double tau[RRR_MAX_K], rs[RRR_MAX_K], delta[RRR_MAX_K];
  const int t = threadIdx.x, nk = a.ncRRR, nco = a.ncORRR, n = nk * nco;
  const uint32_t iter = SWEEP_ITER(a);
  if (t == 0) {
    double c = 1.0;
    for (int k = 0; k < nk; ++k) {
      delta[k] = a.DeltaRRR[k];
      c *= delta[k];
      tau[k] = c;  // (:8)
    }
  }
  __syncthreads();
  for (int e = t; e < n; e += 256) {
    const int k = e % nk;
    const double lam2 = a.wRRR[e] * a.wRRR[e];
    const double bPsi = a.nu / 2 + 0.5 * lam2 * tau[k];                                          // (:12)
    const double psi = gamma_std(a.key, (uint32_t)e, S_PSI_RRR, iter, a.nu / 2 + 0.5) / bPsi;  // (:10,13)
    a.PsiRRR[e] = psi;
    sM[e] = psi * lam2;  // (:14)
  }
  __syncthreads();
  if (t < nk) {
    double v = 0.0;
    for (int c = 0; c < nco; ++c) v += sM[t + nk * c];
    rs[t] = v;
  }
  __syncthreads();
  if (t == 0) {
    for (int h = 0; h < nk; ++h) {  // (:15-23)
      double c = 1.0, sum = 0.0;
      for (int k = 0; k < nk; ++k) {
        c *= delta[k];
        if (k >= h) sum += c * rs[k];
      }
      const double ad = (h == 0 ? a.a1 : a.a2) + 0.5 * nco * (nk - h);
      const double bd = (h == 0 ? a.b1 : a.b2) + 0.5 * sum / delta[h];
      delta[h] = gamma_std(a.key, (uint32_t)h, S_DELTA_RRR, iter, ad) / bd;
    }
    for (int h = 0; h < nk; ++h) a.DeltaRRR[h] = delta[h];
  }
}

__global__ __launch_bounds__(256) void rrr_init_kernel(RrrPriorArgs a) {
  __shared__ double tau[RRR_MAX_K];
  const int t = threadIdx.x, nk = a.ncRRR, n = nk * a.ncORRR;
  if (t == 0) {  // DeltaRRR = c(rgamma(1, a1, b1), rgamma(ncRRR - 1, a2, b2))   (:21)
    double c = 1.0;
    for (int h = 0; h < nk; ++h) {
      const double d = gamma_std(a.key, (uint32_t)h, S_INIT_DELTA_RRR, 0, h == 0 ? a.a1 : a.a2) / (h == 0 ? a.b1 : a.b2);
      a.DeltaRRR[h] = d;
      c *= d;
      tau[h] = c;
    }
  }
  __syncthreads();
  for (int e = t; e < n; e += 256) {
    const double psi = gamma_std(a.key, (uint32_t)e, S_INIT_PSI_RRR, 0, a.nu / 2) / (a.nu / 2);  // (:22)
    a.PsiRRR[e] = psi;
    a.wRRR[e] = normal(a.key, (uint32_t)e, 0, S_INIT_WRRR, 0) / sqrt(psi * tau[e % nk]);        // (:25-26)
  }
}

static RrrPriorArgs rrr_prior_args(State& s, uint32_t iter) {
  RrrPriorArgs a{};
  a.wRRR = s.wRRR;
  a.PsiRRR = s.PsiRRR;
  a.DeltaRRR = s.DeltaRRR;
  a.ncRRR = s.ncRRR;
  a.ncORRR = s.ncORRR;
  a.nu = s.nuRRR;
  a.a1 = s.a1RRR;
  a.b1 = s.b1RRR;
  a.a2 = s.a2RRR;
  a.b2 = s.b2RRR;
  a.key = s.key;
  a.iter = iter;
  a.iter_dev = iter_src(s);
  return a;
}

// X's RRR columns and XX for the current wRRR; everything else derived from X is rebuilt by
// its next reader: XEta and G (launch_xeta), XZ (launch_zt_refresh / updateZ), Gamma2's prep
// matrices and a sharded chain's Gamma2 sums
void launch_rrr_refresh(State& s) {
  if (s.ncRRR == 0) return;
  RrrRefreshArgs a{};
  a.XRRR = s.XRRR;
  a.wRRR = s.wRRR;
  a.XAtXR = s.XAtXR;
  a.XRtXR = s.XRtXR;
  a.X = s.X;
  a.XX = s.XX;
  a.ny = s.ny;
  a.nc = s.nc;
  a.ncN = s.nc - s.ncRRR;
  a.ncRRR = s.ncRRR;
  a.ncORRR = s.ncORRR;
  rrr_refresh_kernel<<<(s.ny + 255) / 256 + 1, 256, 0, s.stream>>>(a);
  HIP_OK(hipGetLastError());
  s.xeta_valid = false;
  s.zt_valid = false;
  s.g2prep_valid = false;
  s.g2s_valid = false;
}

void launch_rrr_init(State& s) {
  if (s.ncRRR == 0) return;
  RrrPriorArgs a = rrr_prior_args(s, 0);
  a.iter_dev = nullptr;
  rrr_init_kernel<<<1, 256, 0, s.stream>>>(a);
  HIP_OK(hipGetLastError());
  launch_rrr_refresh(s);
}

void launch_wrrr_priors(State& s, uint32_t iter) {
  if (s.ncRRR == 0) return;
  rrr_priors_kernel<<<1, 256, 0, s.stream>>>(rrr_prior_args(s, iter));
  HIP_OK(hipGetLastError());
}

void launch_wrrr(State& s, uint32_t iter) {
  if (s.ncRRR == 0) return;
  if (s.NF > 0 && !s.xeta_valid) launch_xeta(s);  // the Eta columns of XEta for the current Eta
  const int ntile = rrr_ntile(s), nchunk = rrr_nchunk(s), n = s.ncRRR * s.ncORRR;
  const int neta = (s.NF + RRR_MAX_K - 1) / RRR_MAX_K;
  const RrrWork w = rrr_work(s);
  RrrZArgs z{};
  z.Z = s.Z;
  z.BL = s.BL;
  z.iSigma = s.iSigma;
  z.XRRR = s.XRRR;
  z.XEta = s.XEta;
  z.ny = s.ny;
  z.ns = s.nsl;
  z.K = s.K;
  z.nc = s.nc;
  z.ncN = s.nc - s.ncRRR;
  z.ncRRR = s.ncRRR;
  z.ncORRR = s.ncORRR;
  z.NF = s.NF;
  z.nchunk = nchunk;
  z.partZ = s.rrrPart;
  z.partE = s.rrrPart + (size_t)ntile * nchunk * n;
  {
    ProfScope ps(s, PROF_WRRR);
    rrr_z_kernel<<<dim3(ntile, nchunk + neta), 256, 0, s.stream>>>(z);
    HIP_OK(hipGetLastError());
  }
  launch_slab_sum2(z.partZ, w.Mraw, n, ntile * nchunk, z.partE, w.EtR, (int64_t)s.NF * s.ncORRR, ntile, s.stream);
  RrrDrawArgs d{};
  d.BL = s.BL;
  d.iSigma = s.iSigma;
  d.XAtXR = s.XAtXR;
  d.XRtXR = s.XRtXR;
  d.PsiRRR = s.PsiRRR;
  d.DeltaRRR = s.DeltaRRR;
  d.Mraw = w.Mraw;
  d.EtR = w.EtR;
  d.C1 = w.C1;
  d.red = w.red;
  d.mu = w.mu;
  d.iU = w.iU;
  d.wRRR = s.wRRR;
  d.ns = s.nsl;
  d.K = s.K;
  d.nc = s.nc;
  d.ncN = s.nc - s.ncRRR;
  d.ncRRR = s.ncRRR;
  d.ncORRR = s.ncORRR;
  d.NF = s.NF;
  d.key = s.key;
  d.iter = iter;
  d.iter_dev = iter_src(s);
  d.noise_zero = s.noise_mode;
  d.fail = s.dev_flags;
  rrr_draw_kernel<<<1, 256, 0, s.stream>>>(d);
  HIP_OK(hipGetLastError());
  launch_rrr_refresh(s);
}

}  // namespace hmsc
