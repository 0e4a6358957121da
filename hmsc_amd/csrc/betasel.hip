// Variable selection (Hmsc(XSelect = ...)) on gfx950: updateBetaSel (R/updateBetaSel.R), the
// initial BetaSel (R/computeInitialParameters.R:105-109) and the masked copy of BL every reader
// of the linear predictor takes.
//
// Selection i (i < ncsel) switches the covariates covGroup_i on or off per species group
// (spGroup_i, q_i).  R turns X into a per-species list X[[j]] = X diag(m_j), m_j[c] = 0 where a
// selection holding column c is off for j's group; that list is never built here.  BL stays raw
// (R's Beta keeps its draws in deselected rows; updateGammaV and the record read them) and
//   BLx = m o BL   (K x ns, rows >= nc copied)
// is what updateZ, updateEta, updateInvSigma and this updater multiply XEta with, so
// X[[j]] Beta[, j] = X (m_j o Beta[, j]).
//
// updateBetaSel, selection by selection (selection i + 1 sees the mask the decisions on i left),
// the groups of one selection in parallel (they hold disjoint species).  With beta = the rows
// covGroup_i of BL[, j], d_j = X[, covGroup_i] beta and r_j = Z[, j] - XEta BLx[, j]:
//   on -> off:  lldif = -1/2 sum_j iSigma_j (sum d_j^2 + 2 sum r_j d_j),  pridif = log(1 - q) - log q
//   off -> on:  lldif = -1/2 sum_j iSigma_j (sum d_j^2 - 2 sum r_j d_j),  pridif = log q - log(1 - q)
// accepted when exp(lldif + pridif) > u, u = uniforms(key, g, i, S_BETASEL, iter).a.
// For a species without NA no pass over Z is needed:
//   sum d^2 = beta^T G[cg, cg] beta,   sum r d = beta^T (xz[cg, j] - G[cg, ] BLx[, j])
// from G = XEta^T XEta and xz = XEta^T Z, which updateBetaLambda has just consumed.  A species
// with NA cells keeps xz over its observed rows only, while the reference sums over every row
// (Z is imputed at NA cells), so such a species takes a direct pass over its column of Z
// (betasel_na_kernel, one workgroup per NA column like gram_na_kernel).
//
// Deviation from Hmsc 3.0-4: R/updateBetaSel.R:53,79 evaluates pnorm(..., log.p = TRUE), a CDF
// where the density of Z belongs; the Gaussian log-density is used here (its constant cancels).
//
// Every sum is taken in a fixed order -- rows by a fixed tree, the species of a group in index
// order through a host-built permutation -- and there are no floating-point atomics, so a graph
// replay repeats an eager sweep bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "rng.h"
#include "state.h"

namespace hmsc {

struct SelArgs {
  int i;              // the selection
  int ncov;           // its covariates
  const int* cov;     // ncov column indices
  const int* perm;    // ns: the species sorted by group, index order within a group
  const int* goff;    // ng + 1 offsets into perm
  const double* q;    // ng
  double* B;          // ng: BetaSel of this selection (0 / 1)
  double* LR;         // ng: lldif + pridif of the last update, as evaluated
  double* Sc;         // ng: sum of the absolute values of the terms that entered lldif
  const int* na_cols;
  const int* na_index;  // per species: its NA column, or -1 (null: no NA at all)
  const int8_t* Ycode;
  const double* XEta;
  const double* Z;
  const double* G;
  const double* xz;
  const double* BL;
  double* BLx;
  double* M;          // nc x ns mask
  const double* iSigma;
  double* term;       // ns x 3: sum d^2, sum r d, their absolute scale (before iSigma)
  int ny, ns, nc, K, Kmax;
  Key key;
  uint32_t iter;
  const uint32_t* iter_dev;
};

// sum d^2, sum r d and the scale of one NA species over every row, Z as it stands
__global__ __launch_bounds__(256) void betasel_na_kernel(SelArgs a) {
  __shared__ double sb[HMSC_KCAP];       // BLx[, j]
  __shared__ double red[3][256];
  const int j = a.na_cols[blockIdx.x], t = threadIdx.x, K = a.K, ny = a.ny;
  for (int k = t; k < K; k += 256) sb[k] = a.BLx[k + (size_t)K * j];
  __syncthreads();
  double s2 = 0.0, srd = 0.0, sab = 0.0;
  for (int i = t; i < ny; i += 256) {
    double e = 0.0, d = 0.0;
    for (int k = 0; k < K; ++k) e += a.XEta[i + (size_t)ny * k] * sb[k];
    for (int c = 0; c < a.ncov; ++c) d += a.XEta[i + (size_t)ny * a.cov[c]] * a.BL[a.cov[c] + (size_t)K * j];
    const double r = a.Z[(size_t)i + (size_t)ny * j] - e;
    s2 += d * d;
    srd += r * d;
    sab += 0.5 * d * d + fabs(r * d);
  }
  red[0][t] = s2;
  red[1][t] = srd;
  red[2][t] = sab;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w)
      for (int v = 0; v < 3; ++v) red[v][t] += red[v][t + w];
    __syncthreads();
  }
  if (t < 3) a.term[(size_t)3 * j + t] = red[t][0];
}

// fixed-order sum over the lanes of a wave (the same butterfly every run)
__device__ __forceinline__ double sel_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one workgroup per group of the selection: the species' terms (through the Grams where the
// species has no NA; a wave per species, its lanes over the products), their sum in index order,
// the decision, and the group's mask and BLx
__global__ __launch_bounds__(256) void betasel_group_kernel(SelArgs a) {
  __shared__ double snew;
  const int g = blockIdx.x, t = threadIdx.x, K = a.K, nc = a.nc, lane = t & 63, w = t >> 6;
  const int p0 = a.goff[g], p1 = a.goff[g + 1];
  for (int p = p0 + w; p < p1; p += 4) {
    const int j = a.perm[p];
    if (a.na_index && a.na_index[j] >= 0) continue;  // betasel_na_kernel's
    const double* blx = a.BLx + (size_t)K * j;
    const double* bl = a.BL + (size_t)K * j;
    // every product of the three sums at once, the lanes over the pairs (covariate, column):
    //   s2 = sum beta_a G[a, b] beta_b,  e = sum beta_a G[a, k] BLx[k],  x = sum beta_a xz[a]
    double s2 = 0.0, s2a = 0.0, e = 0.0, ea = 0.0, x = 0.0, xa = 0.0;
    for (int p2 = lane; p2 < a.ncov * a.ncov; p2 += 64) {
      const int ra = a.cov[p2 / a.ncov], rb = a.cov[p2 % a.ncov];
      const double v = bl[ra] * a.G[ra + (size_t)a.Kmax * rb] * bl[rb];
      s2 += v;
      s2a += fabs(v);
    }
    for (int p2 = lane; p2 < a.ncov * K; p2 += 64) {
      const int ra = a.cov[p2 / K], k = p2 % K;
      const double v = bl[ra] * a.G[ra + (size_t)a.Kmax * k] * blx[k];
      e += v;
      ea += fabs(v);
    }
    for (int ca = lane; ca < a.ncov; ca += 64) {
      const int ra = a.cov[ca];
      const double v = bl[ra] * a.xz[ra + (size_t)K * j];
      x += v;
      xa += fabs(v);
    }
    s2 = sel_wave_sum(s2);
    const double srd = sel_wave_sum(x) - sel_wave_sum(e);
    const double sab = 0.5 * sel_wave_sum(s2a) + sel_wave_sum(xa) + sel_wave_sum(ea);
    if (lane == 0) {
      a.term[(size_t)3 * j] = s2;
      a.term[(size_t)3 * j + 1] = srd;
      a.term[(size_t)3 * j + 2] = sab;
    }
  }
  __syncthreads();
  if (t == 0) {
    double S2 = 0.0, SRD = 0.0, SC = 0.0;
    for (int p = p0; p < p1; ++p) {
      const int j = a.perm[p];
      const double is = a.iSigma[j];
      S2 += is * a.term[(size_t)3 * j];
      SRD += is * a.term[(size_t)3 * j + 1];
      SC += is * a.term[(size_t)3 * j + 2];
    }
    const bool cur = a.B[g] != 0.0;
    const double q = a.q[g];
    const double lldif = cur ? -0.5 * (S2 + 2.0 * SRD) : -0.5 * (S2 - 2.0 * SRD);
    const double pridif = cur ? log(1.0 - q) - log(q) : log(q) - log(1.0 - q);  // R/updateBetaSel.R:83-87
    const double u = uniforms(a.key, (uint32_t)g, (uint32_t)a.i, S_BETASEL, SWEEP_ITER(a)).a;
    const bool flip = exp(lldif + pridif) > u;                                   // :89
    const double nv = (cur != flip) ? 1.0 : 0.0;
    a.LR[g] = lldif + pridif;
    a.Sc[g] = SC;
    a.B[g] = nv;
    snew = nv;
  }
  __syncthreads();
  const double nv = snew;
  const int n = (p1 - p0) * a.ncov;
  for (int e = t; e < n; e += 256) {
    const int j = a.perm[p0 + e / a.ncov], c = a.cov[e % a.ncov];
    a.M[c + (size_t)nc * j] = nv;
    a.BLx[c + (size_t)K * j] = nv * a.BL[c + (size_t)K * j];
  }
}

// the mask and BLx from BetaSel and BL, all of it
__global__ __launch_bounds__(256) void sel_refresh_kernel(const double* B, const int* owner, const int* boff,
                                                          const int* spg, const double* BL, double* BLx, double* M,
                                                          int K, int nc, int ns) {
  const int64_t n = (int64_t)K * ns;
  for (int64_t p = blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const int k = (int)(p % K), j = (int)(p / K);
    double m = 1.0;
    if (k < nc) {
      const int i = owner[k];
      if (i >= 0) m = B[boff[i] + spg[j + (size_t)ns * i]];
      M[k + (size_t)nc * j] = m;
    }
    BLx[p] = k < nc ? m * BL[p] : BL[p];
  }
}

void launch_sel_refresh(State& s) {
  if (s.ncsel == 0) return;
  const int64_t n = (int64_t)s.K * s.nsl;
  const int grid = (int)std::min<int64_t>(1024, (n + 255) / 256);
  sel_refresh_kernel<<<grid, 256, 0, s.stream>>>(s.selB, s.selOwner, s.selBoff, s.selSpg, s.BL, s.BLx, s.selM, s.K, s.nc,
                                                 s.nsl);
  HIP_OK(hipGetLastError());
}

void launch_betasel(State& s, uint32_t iter) {
  if (s.ncsel == 0) return;
  // G and xz of the current Z and Eta: what updateBetaLambda has just read, rebuilt here when it
  // is switched off
  if (!s.xeta_valid) launch_xeta(s);
  flush_g(s);
  if (!s.zt_valid) launch_zt_refresh(s);
  ProfScope ps(s, PROF_BETASEL);
  for (int i = 0; i < s.ncsel; ++i) {
    SelArgs a{};
    a.i = i;
    a.ncov = s.selNcov[i];
    a.cov = s.selCov + (size_t)s.nc * i;
    a.perm = s.selPerm + (size_t)s.nsl * i;
    a.goff = s.selGoffD + s.selGoff[i];
    a.q = s.selQ + s.selOff[i];
    a.B = s.selB + s.selOff[i];
    a.LR = s.selLR + s.selOff[i];
    a.Sc = s.selSc + s.selOff[i];
    a.na_cols = s.na_cols;
    a.na_index = s.n_na_cols > 0 ? s.na_index : nullptr;
    a.Ycode = s.Ycode;
    a.XEta = s.XEta;
    a.Z = s.Z;
    a.G = s.G;
    a.xz = s.XZ;
    a.BL = s.BL;
    a.BLx = s.BLx;
    a.M = s.selM;
    a.iSigma = s.iSigma;
    a.term = s.selTerm;
    a.ny = s.ny;
    a.ns = s.nsl;
    a.nc = s.nc;
    a.K = s.K;
    a.Kmax = s.Kmax;
    a.key = s.key;
    a.iter = iter;
    a.iter_dev = iter_src(s);
    if (s.n_na_cols > 0) {
      betasel_na_kernel<<<s.n_na_cols, 256, 0, s.stream>>>(a);
      HIP_OK(hipGetLastError());
    }
    betasel_group_kernel<<<s.selNg[i], 256, 0, s.stream>>>(a);
    HIP_OK(hipGetLastError());
  }
}

}  // namespace hmsc
