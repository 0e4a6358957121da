// GPP kriging of the latent factors at new units (R/predictLatentFactor.R:161-203): the predictive
// process over nK knots, mode 4 of hmsc_krige and of a level of hmsc_predict_map.
//
// Per grid value a > 0 in use, with knots sK, fitted units s1 (np) and new units s2:
//   Wss = exp(-d(sK, sK) / a)   W12 = exp(-d(s1, sK) / a)   Wns = exp(-d(s2, sK) / a)
//   iWss = Wss^-1,  dD_i = 1 - W12[i,] iWss W12[i,]',  idD = 1 / dD
//   F = Wss + W12' diag(idD) W12,  iF = F^-1,  R = chol(iF) (upper: R'R = iF)
//   C[, j] = iF (W12' (idD o eta_j)) + R z_knot(., h_j, s_j)         for the value's pairs j = (s_j, h_j)
//   out[i, j] = Wns[i,] C[, j] + sqrt(max(dDn_i, 0)) z_new(i, h_j, s_j),  dDn_i = 1 - Wns[i,] iWss Wns[i,]'
// The sample's grid value is that of its last factor for every factor (R's ag = alpha[nf]); the
// caller groups the pairs accordingly.
//
// gpp_plan_group does everything up to C once per grid value: it is nK-sized or one pass over np x nK
// (W12 is formed once, F is a diag-scaled SYRK over np and W12' (idD o E) an np-deep product, both on
// the 64 x 64 MFMA tiles of krige_tile.h; the inverses are dense_potrf_lower, dense_trtri_lower and
// dense_lauum_lower).  What stays resident is iWss and C.  gpp_slab_group serves a slab of new units:
// gpp_quad_kernel (dDn) and gpp_slab_kernel (the product and the output) build their 64 x 64 chunks
// of Wns in LDS straight from the coordinates, so the rows x nK matrix never exists in global memory
// and a slab's workspace is its dDn vector.
//
// Draws: z_new is the Philox normal of (new unit, factor, S_KRIGE + 256 level, sample), z_knot that
// of (knot, factor, S_KRIGE_KNOT + 256 level, sample).  Every sum has a fixed order -- the knots in
// index order, chunk by chunk -- and a value depends on (unit, pair) alone, whatever tile, slab or
// group column it falls in.
//
// Guards: a fitted unit on a knot (its kernel entry is exactly 1) or with dD_i <= 0 is reported by
// its index (info[3]); a new unit on a knot has dDn = 0, and dDn is clamped at 0 elsewhere.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "krige_tile.h"
#include "state.h"

namespace hmsc {

namespace {

// exp(-|x_i - k_j| / a): unit i = row `i` of X (ld ldx), knot j = row j of Kn (ld nK); the dimensions
// summed in index order without contraction (the host's ((a - b) ** 2).sum(-1))
__device__ __forceinline__ double gp_w(const double* X, size_t ldx, int i, const double* Kn, int nK, int j, int sdim,
                                       double a) {
  double s = 0.0;
  for (int d = 0; d < sdim; ++d) {
    const double diff = X[(size_t)i + ldx * d] - Kn[(size_t)j + (size_t)nK * d];
    s = __dadd_rn(s, __dmul_rn(diff, diff));
  }
  return exp(-sqrt(s) / a);
}

// where a launch's rows live: row i is unit first + (unit ? unit[i] : i) of X
struct GpRows {
  const double* X;
  size_t ldx;
  const int* unit;
  int first, n;
};
__device__ __forceinline__ int gp_row(const GpRows& g, int i) { return g.first + kg_unit(g.unit, i); }

// the 64 x 64 chunk W[I0 + r, K0 + k] into S[r + KLD k], zero padded
__device__ __forceinline__ void gp_w_tile(double* S, const GpRows& g, int I0, int rows, const double* Kn, int nK, int K0,
                                          int sdim, double a) {
#pragma unroll 4
  for (int u = 0; u < KU; ++u) {
    const int p = threadIdx.x + 256 * u, r = p & 63, k = p >> 6;
    double w = 0.0;
    if (r < rows && K0 + k < nK) w = gp_w(g.X, g.ldx, gp_row(g, I0 + r), Kn, nK, K0 + k, sdim, a);
    S[r + KLD * k] = w;
  }
}

// Wss (nK x nK, full) and W12 (np x nK): one thread per entry, consecutive threads along a column
__global__ __launch_bounds__(256) void gpp_w_kernel(const double* coords, int N, int np, const double* Kn, int nK,
                                                    int sdim, double a, double* Wss, double* W12) {
  const bool ss = blockIdx.y == 0;
  const int rows = ss ? nK : np;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * nK) return;
  const int r = (int)(idx % rows), c = (int)(idx / rows);
  if (ss)
    Wss[idx] = gp_w(Kn, (size_t)nK, r, Kn, nK, c, sdim, a);
  else
    W12[idx] = gp_w(coords, (size_t)N, r, Kn, nK, c, sdim, a);
}

// q_i = 1 - W[i,] iWss W[i,]' for 64 rows per workgroup, W's chunks built in LDS.  Per 64 columns J
// of iWss: T = W iWss[, J] on the MFMA tiles (knot chunks in order), T o W[, J] laid out in LDS and
// each row summed by one thread in column order.
//   fitted (info != null): v_i = 1 / q_i; a unit on a knot or with q_i <= 0 raises *info to np - i
//                          (the lowest such i wins)
//   new:                   v_i = sqrt(max(q_i, 0)), 0 for a unit on a knot
__global__ __launch_bounds__(256) void gpp_quad_kernel(GpRows g, const double* Kn, int nK, int sdim, double a,
                                                       const double* iWss, double* v, int* info) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  __shared__ int onk[KB];
  const int I0 = blockIdx.x * KB, rows = min(KB, g.n - I0), t = threadIdx.x;
  if (t < KB) onk[t] = 0;
  double run = 0.0, vb[KU];
  for (int J0 = 0; J0 < nK; J0 += KB) {
    const int colsJ = min(KB, nK - J0);
    d4 acc[2][2];
    kg_zero(acc);
    for (int K0 = 0; K0 < nK; K0 += KB) {
      const int rowsK = min(KB, nK - K0);
      kg_load(vb, iWss, (size_t)nK, K0, J0, rowsK, colsJ);
      gp_w_tile(SA, g, I0, rows, Kn, nK, K0, sdim, a);
      kg_store<true>(SB, vb, rowsK, colsJ);  // SB[c][k] = iWss[K0 + k, J0 + c]
      __syncthreads();
      kg_mma(acc, SA, SB);
      __syncthreads();
    }
    kg_each(acc, [&](int r, int c, double tv) {
      double p = 0.0;
      if (r < rows && c < colsJ) {
        const double w = gp_w(g.X, g.ldx, gp_row(g, I0 + r), Kn, nK, J0 + c, sdim, a);
        if (w == 1.0) onk[r] = 1;
        p = tv * w;
      }
      SA[r + KLD * c] = p;
    });
    __syncthreads();
    if (t < KB)
      for (int c = 0; c < KB; ++c) run += SA[t + KLD * c];
    __syncthreads();
  }
  if (t < rows) {
    const double q = 1.0 - run;
    if (info) {
      if (onk[t] || !(q > 0.0)) atomicMax(info, g.n - (I0 + t));
      v[I0 + t] = 1.0 / q;
    } else {
      v[I0 + t] = onk[t] ? 0.0 : sqrt(fmax(q, 0.0));
    }
  }
}

// F = Wss + W12' diag(idD) W12 (nK x nK, all tiles), np deep: SA[r][k] = W12[K0 + k, I0 + r],
// SB[c][k] = idD[K0 + k] W12[K0 + k, J0 + c]; Wss's entry is formed again from the knots
__global__ __launch_bounds__(256) void gpp_f_kernel(const double* W12, const double* idD, int np, const double* Kn,
                                                    int nK, int sdim, double a, double* F) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  const int I0 = blockIdx.x * KB, J0 = blockIdx.y * KB, rowsI = min(KB, nK - I0), rowsJ = min(KB, nK - J0);
  d4 acc[2][2];
  kg_zero(acc);
  double va[KU], vb[KU];
  auto load = [&](int K0) {
    const int rowsK = min(KB, np - K0);
    kg_load(va, W12, (size_t)np, K0, I0, rowsK, rowsI);
    kg_load(vb, W12, (size_t)np, K0, J0, rowsK, rowsJ);
#pragma unroll
    for (int u = 0; u < KU; ++u) vb[u] = idD[K0 + min((int)((threadIdx.x + 256 * u) & 63), rowsK - 1)] * vb[u];
  };
  load(0);
  for (int K0 = 0; K0 < np; K0 += KB) {
    const int rowsK = min(KB, np - K0);
    kg_store<true>(SA, va, rowsK, rowsI);
    kg_store<true>(SB, vb, rowsK, rowsJ);
    __syncthreads();
    if (K0 + KB < np) load(K0 + KB);
    kg_mma(acc, SA, SB);
    __syncthreads();
  }
  kg_each(acc, [&](int r, int c, double v) {
    if (r < rowsI && c < rowsJ)
      F[(size_t)(I0 + r) + (size_t)nK * (J0 + c)] = gp_w(Kn, (size_t)nK, I0 + r, Kn, nK, J0 + c, sdim, a) + v;
  });
}

// E[:, j] = idD o Eta_s[:, h] of the group's column j
__global__ __launch_bounds__(256) void gpp_gather_kernel(const double* Eta, const double* idD, int np, int nfmax,
                                                         const int* col_s, const int* col_h, int c, double* E) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const double w = idD[i];
  for (int j = blockIdx.y; j < c; j += gridDim.y)
    E[(size_t)i + (size_t)np * j] = w * Eta[((size_t)col_s[j] * nfmax + col_h[j]) * np + i];
}

// Zk[k, j] = z_knot(k, h_j, s_j)
__global__ __launch_bounds__(256) void gpp_zknot_kernel(Key key, uint32_t stream, int nK, const int* col_s,
                                                        const int* col_h, int c, double* Zk) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nK) return;
  for (int j = blockIdx.y; j < c; j += gridDim.y)
    Zk[(size_t)k + (size_t)nK * j] = normal(key, (uint32_t)k, (uint32_t)col_h[j], stream, (uint32_t)col_s[j]);
}

// T = A' B (nK x c): A np x nK (ld np), B np x c (ld np), the np rows in index order
__global__ __launch_bounds__(256) void gpp_atb_kernel(const double* A, const double* B, int np, int nK, int c, double* T) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  const int I0 = blockIdx.x * KB, J0 = blockIdx.y * KB, rowsI = min(KB, nK - I0), colsJ = min(KB, c - J0);
  d4 acc[2][2];
  kg_zero(acc);
  double va[KU], vb[KU];
  kg_load(va, A, (size_t)np, 0, I0, min(KB, np), rowsI);
  kg_load(vb, B, (size_t)np, 0, J0, min(KB, np), colsJ);
  for (int K0 = 0; K0 < np; K0 += KB) {
    const int rowsK = min(KB, np - K0);
    kg_store<true>(SA, va, rowsK, rowsI);
    kg_store<true>(SB, vb, rowsK, colsJ);
    __syncthreads();
    if (K0 + KB < np) {
      kg_load(va, A, (size_t)np, K0 + KB, I0, min(KB, np - K0 - KB), rowsI);
      kg_load(vb, B, (size_t)np, K0 + KB, J0, min(KB, np - K0 - KB), colsJ);
    }
    kg_mma(acc, SA, SB);
    __syncthreads();
  }
  kg_each(acc, [&](int r, int cc, double v) {
    if (r < rowsI && cc < colsJ) T[(size_t)(I0 + r) + (size_t)nK * (J0 + cc)] = v;
  });
}

// C[k, j] = sum_l iF[k, l] T[l, j] + sum_{l >= k} L[l, k] Zk[l, j] (L = chol(iF) lower, so R = L'):
// the nK-deep remainder, one thread per entry, l in index order
__global__ __launch_bounds__(256) void gpp_c_kernel(const double* iF, const double* L, const double* T, const double* Zk,
                                                    int nK, int c, double* Cm) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nK) return;
  for (int j = blockIdx.y; j < c; j += gridDim.y) {
    const double* t = T + (size_t)nK * j;
    const double* z = Zk + (size_t)nK * j;
    double mu = 0.0, eps = 0.0;
    for (int l = 0; l < nK; ++l) mu = fma(iF[(size_t)k + (size_t)nK * l], t[l], mu);
    for (int l = k; l < nK; ++l) eps = fma(L[(size_t)l + (size_t)nK * k], z[l], eps);
    Cm[(size_t)k + (size_t)nK * j] = mu + eps;
  }
}

// out = Wns C + v o z_new for a 64-unit x 64-pair tile, the knots in chunks of 64: the Wns chunk is
// built in LDS from the coordinates, C's chunk comes from global memory (the next one during the
// MFMAs).  out[(s nfmax + h) ldo + i], as krige_mean_kernel's.
struct GppSlabArgs {
  GpRows g;
  const double* Kn;
  const double* Cm;  // nK x c
  const double* v;   // sqrt(dDn) of the launch's rows
  int nK, sdim, c, nfmax;
  double a;
  const int* col_s;
  const int* col_h;
  double* out;
  size_t ldo;
  Key key;
  uint32_t stream;
};

__global__ __launch_bounds__(256) void gpp_slab_kernel(GppSlabArgs a) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  const int I0 = blockIdx.x * KB, J0 = blockIdx.y * KB, rowsI = min(KB, a.g.n - I0), colsJ = min(KB, a.c - J0);
  d4 acc[2][2];
  kg_zero(acc);
  double vb[KU];
  kg_load(vb, a.Cm, (size_t)a.nK, 0, J0, min(KB, a.nK), colsJ);
  for (int K0 = 0; K0 < a.nK; K0 += KB) {
    const int rowsK = min(KB, a.nK - K0);
    gp_w_tile(SA, a.g, I0, rowsI, a.Kn, a.nK, K0, a.sdim, a.a);
    kg_store<true>(SB, vb, rowsK, colsJ);  // SB[c][k] = C[K0 + k, J0 + c]
    __syncthreads();
    if (K0 + KB < a.nK) kg_load(vb, a.Cm, (size_t)a.nK, K0 + KB, J0, min(KB, a.nK - K0 - KB), colsJ);
    kg_mma(acc, SA, SB);
    __syncthreads();
  }
  kg_each(acc, [&](int r, int c, double m) {
    if (r < rowsI && c < colsJ) {
      const int i = I0 + r, s = a.col_s[J0 + c], h = a.col_h[J0 + c];
      const double z = normal(a.key, (uint32_t)kg_unit(a.g.unit, i), (uint32_t)h, a.stream, (uint32_t)s);
      a.out[((size_t)s * a.nfmax + h) * a.ldo + i] = fma(a.v[i], z, m);
    }
  });
}

void gp_mark(hipStream_t st, hipEvent_t* ev, int k) {
  if (ev) HIP_OK(hipEventRecord(ev[k], st));
}

// A <- A^-1 (full symmetric) of the positive definite A (lower triangle read); M: n x n scratch
void gp_spd_inverse(hipStream_t st, double* A, int n, double* M, double* ws, int* info, int* sync) {
  dense_potrf_lower(st, A, n, n, ws, info, 0, sync);
  dense_trtri_lower(st, A, n, n, M, n, ws, true);
  dense_lauum_lower(st, M, n, n, A, n);
}

}  // namespace

GppWork gpp_carve(double* base, int np, int nK, int cmax) {
  const size_t k = (size_t)nK, n = (size_t)np, c = (size_t)cmax;
  GppWork w{};
  w.A = base, base += k * k;
  w.F = base, base += k * k;
  w.M = base, base += k * k;
  w.W12 = base, base += n * k;
  w.idD = base, base += n;
  w.E = base, base += n * c;
  w.T = base, base += k * c;
  w.Zk = base, base += k * c;
  w.ws = base;
  return w;
}

void gpp_plan_group(hipStream_t st, const KrigeDev& d, const GppWork& w, double a, int col0, int c, double* iWss,
                    double* Cm, int* info, hipEvent_t* ev) {
  const Key key{(uint32_t)d.seed, (uint32_t)(d.seed >> 32)};
  const int np = d.np, nK = d.nK, nt = (nK + KB - 1) / KB, gy = std::min(c, 65535);
  const int* cs = d.col_s + col0;
  const int* ch = d.col_h + col0;
  const size_t kk = (size_t)nK * nK * sizeof(double);
  gp_mark(st, ev, 0);
  const size_t big = (size_t)std::max(np, nK) * nK;
  gpp_w_kernel<<<dim3((unsigned)((big + 255) / 256), 2), 256, 0, st>>>(d.coords, d.N, np, d.knots, nK, d.sdim, a, iWss,
                                                                      w.W12);
  HIP_OK(hipGetLastError());
  gp_mark(st, ev, 1);
  gp_spd_inverse(st, iWss, nK, w.M, w.ws, info, d.sync);  // iWss
  gp_mark(st, ev, 2);
  GpRows fit{d.coords, (size_t)d.N, nullptr, 0, np};
  gpp_quad_kernel<<<(np + KB - 1) / KB, 256, 0, st>>>(fit, d.knots, nK, d.sdim, a, iWss, w.idD, info + 3);
  gpp_f_kernel<<<dim3(nt, nt), 256, 0, st>>>(w.W12, w.idD, np, d.knots, nK, d.sdim, a, w.A);
  HIP_OK(hipGetLastError());
  gp_mark(st, ev, 3);
  gp_spd_inverse(st, w.A, nK, w.M, w.ws, info + 1, d.sync);  // A = iF
  HIP_OK(hipMemcpyAsync(w.F, w.A, kk, hipMemcpyDeviceToDevice, st));
  dense_potrf_lower(st, w.F, nK, nK, w.ws, info + 2, 0, d.sync);  // F = chol(iF) lower: R = F'
  gp_mark(st, ev, 4);
  gpp_gather_kernel<<<dim3((np + 255) / 256, gy), 256, 0, st>>>(d.Eta, w.idD, np, d.nfmax, cs, ch, c, w.E);
  gpp_zknot_kernel<<<dim3((nK + 255) / 256, gy), 256, 0, st>>>(key, d.stream - S_KRIGE + S_KRIGE_KNOT, nK, cs, ch, c,
                                                               w.Zk);
  gpp_atb_kernel<<<dim3(nt, (c + KB - 1) / KB), 256, 0, st>>>(w.W12, w.E, np, nK, c, w.T);
  gpp_c_kernel<<<dim3((nK + 255) / 256, gy), 256, 0, st>>>(w.A, w.F, w.T, w.Zk, nK, c, Cm);
  HIP_OK(hipGetLastError());
  gp_mark(st, ev, 5);
}

void gpp_slab_group(hipStream_t st, const KrigeDev& d, double a, int col0, int c, const double* iWss, const double* Cm,
                    hipEvent_t* ev) {
  const Key key{(uint32_t)d.seed, (uint32_t)(d.seed >> 32)};
  const int nn = d.nn;
  GpRows rows{d.coords, (size_t)d.N, d.unit, d.np, nn};
  gp_mark(st, ev, 0);
  gpp_quad_kernel<<<(nn + KB - 1) / KB, 256, 0, st>>>(rows, d.knots, d.nK, d.sdim, a, iWss, d.v, nullptr);
  HIP_OK(hipGetLastError());
  gp_mark(st, ev, 1);
  GppSlabArgs sa{rows, d.knots, Cm, d.v, d.nK, d.sdim, c, d.nfmax, a, d.col_s + col0, d.col_h + col0, d.out, d.ldo,
                 key, d.stream};
  gpp_slab_kernel<<<dim3((nn + KB - 1) / KB, (c + KB - 1) / KB), 256, 0, st>>>(sa);
  HIP_OK(hipGetLastError());
  gp_mark(st, ev, 2);
}

}  // namespace hmsc
