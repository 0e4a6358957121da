// Kriging of the latent factors at new units of a spatial random level
// (R/predictLatentFactor.R:59-160), for all posterior samples of one level in
// one call (hmsc_krige: run_krige in krige_level.hip, which drives these launchers through a KrigeLevel).
//
// K11, K12 and K22 depend on the sample only through alpha[h], an index into the alphapw grid,
// so the (sample, factor) pairs are grouped by grid index g and every distinct g costs one
// factorization plus products over all of its pairs' columns.  Per group with a_g > 0
// (predictMean, predictMeanField and 'Full'; krige_launch_group):
//   krige_kernel_matrices  K11 (lower), K12 and -- 'Full' -- K22 (lower) = exp(-d / a_g)
//   dense_potrf_lower      K11 = L L^T (dense.hip; the diagonal-block inverses stay in ws)
//   dense_trsm_lower       R <- L^-1 R for R = [K12 | E_g], E_g the group's Eta columns: a
//                          workgroup owns 64 columns of R and walks the 64-row blocks itself,
//                          R_b <- Linv_b (R_b - sum_{j<b} L_bj R_j), all on MFMA tiles
//   krige_mean_kernel      M = B^T Y (B = L^-1 K12, Y = L^-1 E_g), written to the output with
//                          the mode's noise: none (:74-77) or sqrt(1 - colsum(B^2)) z (:80-85)
//   'Full' (:105-112)      W = K22 - B^T B (krige_syrk_kernel, lower tiles), its Cholesky, and
//                          out += L_W Z (krige_trmm_kernel, tiles above the diagonal skipped)
// a_g = 0: out = z (:86-91, :113-115).  'NNGP' (:118-160): krige_nn_kernel, one wave per new unit.
//
// z of new unit i, factor h, sample s is normal(key, i, h, S_KRIGE + LEVEL_STRIDE level, s): it
// does not depend on the grouping or the tiling.  Every sum has a fixed order (no floating-point
// atomics), so a call repeats bit for bit.
//
// hmsc_predict_map (map.hip, through the same KrigeLevel) walks its new units in slabs: krige_plan_group keeps per grid value
// what the fitted units alone decide (K11, its factor, Y), krige_slab_group does the rest per slab.
// The kernels therefore take the new units as an index list among the call's (KrigeDev::unit:
// the coordinate row and the counter of z) and write out[(s nfmax + h) ldo + i]; hmsc_krige is
// unit = null, ldo = nn.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "state.h"
#include "z_kernel.h"  // d4, mfma_f64
#include "wave_la.h"
#include "krige_tile.h"

namespace hmsc {

namespace {

// distance of units i and j: from the distance matrix (N x N), or Euclidean from the coordinates
// (N x sdim, column-major), the dimensions summed in index order without contraction (the
// host's ((a - b) ** 2).sum(-1))
__device__ __forceinline__ double kg_dist(const double* coords, const double* D, int N, int sdim, int i, int j) {
  if (D) return D[(size_t)i + (size_t)N * j];
  double s = 0.0;
  for (int d = 0; d < sdim; ++d) {
    const double diff = coords[i + (size_t)N * d] - coords[j + (size_t)N * d];
    s = __dadd_rn(s, __dmul_rn(diff, diff));
  }
  return sqrt(s);
}

// lower tile (ti, tj), ti >= tj, of a triangular launch
__device__ __forceinline__ void kg_lower_tile(int b, int& ti, int& tj) {
  ti = (int)((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
  tj = b - ti * (ti + 1) / 2;
  if (tj > ti) ++ti, tj = b - ti * (ti + 1) / 2;  // guard sqrt rounding
  if (tj < 0) --ti, tj = b - ti * (ti + 1) / 2;
}

// the sum of v over the wave, in a fixed (butterfly) order, in every lane
__device__ __forceinline__ double kg_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ---------------------------------------------------------------------------------------
// kernel matrices: one thread per entry, consecutive threads along a column
//   blockIdx.y + which0 = 0: K11 lower (np x np)   1: K12 (np x nn, the first columns of R)
//                         2: K22 lower (nn x nn, 'Full' only)
// The nn new units are the call's units unit[0 .. nn) (null: 0 .. nn - 1), rows np + unit[.] of
// the N coordinates / distances.
// ---------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void krige_kernel_matrices(const double* coords, const double* D, int np, int nn,
                                                             int N, const int* unit, int sdim, double a, int which0,
                                                             double* K11, double* K12, double* K22) {
  const int which = blockIdx.y + which0;
  const int rows = which == 2 ? nn : np, cols = which == 0 ? np : nn;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)rows * cols) return;
  const int r = (int)(idx % rows), c = (int)(idx / rows);
  if (which != 1 && r < c) return;
  const int i = which == 2 ? np + kg_unit(unit, r) : r, j = which == 0 ? c : np + kg_unit(unit, c);
  double* out = which == 0 ? K11 : which == 1 ? K12 : K22;
  out[(size_t)r + (size_t)rows * c] = exp(-kg_dist(coords, D, N, sdim, i, j) / a);
}

// E[:, j] = Eta_s[:, h] of the group's column j
__global__ __launch_bounds__(256) void krige_gather_kernel(const double* Eta, int np, int nfmax, const int* col_s,
                                                           const int* col_h, int c, double* E) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  for (int j = blockIdx.y; j < c; j += gridDim.y)
    E[(size_t)i + (size_t)np * j] = Eta[((size_t)col_s[j] * nfmax + col_h[j]) * np + i];
}

// Z[i, j] = z(unit i, h_j, s_j) ('Full'), or -- a_g = 0 -- straight into the output (ld ldo)
__global__ __launch_bounds__(256) void krige_z_kernel(Key key, uint32_t stream, int nn, const int* unit, int nfmax,
                                                      const int* col_s, const int* col_h, int c, double* Z,
                                                      double* out, size_t ldo) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nn) return;
  for (int j = blockIdx.y; j < c; j += gridDim.y) {
    const int s = col_s[j], h = col_h[j];
    const double z = normal(key, (uint32_t)kg_unit(unit, i), (uint32_t)h, stream, (uint32_t)s);
    if (Z)
      Z[(size_t)i + (size_t)nn * j] = z;
    else
      out[((size_t)s * nfmax + h) * ldo + i] = z;
  }
}

// ---------------------------------------------------------------------------------------
// R <- L^-1 R (R: n x m, ld ldr), L and the diagonal-block inverses as dense_potrf_lower left
// them.  Workgroup = 64 columns of R, block rows in order; the blocks R_j, j < b, it reads are
// the ones it wrote itself (no other workgroup touches its columns).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trsm_lower_kernel(const double* L, int ldl, int n, const double* Linv, double* R,
                                                         size_t ldr, int m) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  const int J0 = blockIdx.x * KB, cols = min(KB, m - J0), nbk = (n + KB - 1) / KB;
  double va[KU], vb[KU];
  for (int b = 0; b < nbk; ++b) {
    const int B0 = b * KB, rows = min(KB, n - B0);
    d4 acc[2][2];
    kg_zero(acc);
    if (b > 0) {
      kg_load(va, L, ldl, B0, 0, rows, KB);
      kg_load(vb, R, ldr, 0, J0, KB, cols);
    }
    for (int j = 0; j < b; ++j) {  // acc = sum_j L_bj R_j; chunk j + 1 loads during chunk j's MFMAs
      kg_store<false>(SA, va, rows, KB);  // SA[r][k] = L[B0 + r, 64 j + k]
      kg_store<true>(SB, vb, KB, cols);   // SB[c][k] = R[64 j + k, J0 + c]
      __syncthreads();
      if (j + 1 < b) {
        kg_load(va, L, ldl, B0, KB * (j + 1), rows, KB);
        kg_load(vb, R, ldr, KB * (j + 1), J0, KB, cols);
      }
      kg_mma(acc, SA, SB);
      __syncthreads();
    }
    // T = R_b - acc as the second operand (SB[c][k] = T[k][c]), Linv_b as the first
    kg_load(va, Linv + (size_t)b * KB * KB, KB, 0, 0, KB, KB);
    double rv[16];
    int e = 0;
    kg_each(acc, [&](int r, int c, double) {
      rv[e++] = R[(size_t)(B0 + min(r, rows - 1)) + ldr * (size_t)(J0 + min(c, cols - 1))];
    });
    e = 0;
    kg_each(acc, [&](int r, int c, double v) { SB[c + KLD * r] = (r < rows && c < cols) ? rv[e] - v : 0.0, ++e; });
    kg_store<false>(SA, va, KB, KB);
    __syncthreads();
    kg_zero(acc);
    kg_mma(acc, SA, SB);
    kg_each(acc, [&](int r, int c, double v) {
      if (r < rows && c < cols) R[(size_t)(B0 + r) + ldr * (size_t)(J0 + c)] = v;
    });
    __syncthreads();  // R_b written (and SA / SB free) before the next block row reads it
  }
}

// ---------------------------------------------------------------------------------------
// the kriging mean M = B^T Y (nn x c; B = L^-1 K12 and Y = L^-1 E_g, np rows, k in index order)
// and the output of the modes without a joint draw: out = M (+ sqrt(v_i) z, v from
// krige_colnorm_kernel).  out[(s nfmax + h) ldo + i]: hmsc_krige's layout at ldo = nn, a slab's
// Eta table (map.hip) at ldo = its units, out then pointing at the slab's first new unit.
// ---------------------------------------------------------------------------------------
struct MeanArgs {
  const double* R;  // B
  size_t ldr;
  const double* Y;
  size_t ldy;
  int np, nn, c, nfmax;
  const int* col_s;
  const int* col_h;
  const double* v;  // predictMeanField: 1 - colsum(B^2); else null
  const int* unit;  // the new units' indices among the call's (the counter of z), or null: i
  double* out;
  size_t ldo;
  Key key;
  uint32_t stream;
};

__global__ __launch_bounds__(256) void krige_mean_kernel(MeanArgs a) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  const int I0 = blockIdx.x * KB, J0 = blockIdx.y * KB, rowsI = min(KB, a.nn - I0), colsJ = min(KB, a.c - J0);
  const double* Y = a.Y;
  d4 acc[2][2];
  kg_zero(acc);
  double va[KU], vb[KU];
  kg_load(va, a.R, a.ldr, 0, I0, min(KB, a.np), rowsI);
  kg_load(vb, Y, a.ldy, 0, J0, min(KB, a.np), colsJ);
  for (int K0 = 0; K0 < a.np; K0 += KB) {
    const int rowsK = min(KB, a.np - K0);
    kg_store<true>(SA, va, rowsK, rowsI);  // SA[r][k] = B[K0 + k, I0 + r]
    kg_store<true>(SB, vb, rowsK, colsJ);  // SB[c][k] = Y[K0 + k, J0 + c]
    __syncthreads();
    if (K0 + KB < a.np) {
      kg_load(va, a.R, a.ldr, K0 + KB, I0, min(KB, a.np - K0 - KB), rowsI);
      kg_load(vb, Y, a.ldy, K0 + KB, J0, min(KB, a.np - K0 - KB), colsJ);
    }
    kg_mma(acc, SA, SB);
    __syncthreads();
  }
  kg_each(acc, [&](int r, int c, double m) {
    if (r < rowsI && c < colsJ) {
      const int i = I0 + r, s = a.col_s[J0 + c], h = a.col_h[J0 + c];
      if (a.v)
        m = fma(sqrt(a.v[i]), normal(a.key, (uint32_t)kg_unit(a.unit, i), (uint32_t)h, a.stream, (uint32_t)s), m);
      a.out[((size_t)s * a.nfmax + h) * a.ldo + i] = m;
    }
  });
}

// v_i = 1 - sum_k B[k, i]^2: one wave per column, lane-strided partial sums, then the butterfly
__global__ __launch_bounds__(256) void krige_colnorm_kernel(const double* B, size_t ldb, int np, int nn, double* v) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= nn) return;
  const double* col = B + ldb * (size_t)i;
  double s = 0.0;
  for (int k = lane; k < np; k += 64) s = fma(col[k], col[k], s);
  s = kg_wave_sum(s);
  if (lane == 0) v[i] = 1.0 - s;
}

// W = K22 - B^T B, lower tiles only, in place in the K22 buffer (nn x nn, ld nn)
__global__ __launch_bounds__(256) void krige_syrk_kernel(const double* B, size_t ldb, int np, int nn, double* W) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  int ti, tj;
  kg_lower_tile((int)blockIdx.x, ti, tj);
  const int I0 = KB * ti, J0 = KB * tj, rowsI = min(KB, nn - I0), rowsJ = min(KB, nn - J0);
  d4 acc[2][2];
  kg_zero(acc);
  double va[KU], vb[KU];
  kg_load(va, B, ldb, 0, I0, min(KB, np), rowsI);
  kg_load(vb, B, ldb, 0, J0, min(KB, np), rowsJ);
  for (int K0 = 0; K0 < np; K0 += KB) {
    const int rowsK = min(KB, np - K0);
    kg_store<true>(SA, va, rowsK, rowsI);
    kg_store<true>(SB, vb, rowsK, rowsJ);
    __syncthreads();
    if (K0 + KB < np) {
      kg_load(va, B, ldb, K0 + KB, I0, min(KB, np - K0 - KB), rowsI);
      kg_load(vb, B, ldb, K0 + KB, J0, min(KB, np - K0 - KB), rowsJ);
    }
    kg_mma(acc, SA, SB);
    __syncthreads();
  }
  kg_each(acc, [&](int r, int c, double v) {
    if (r < rowsI && c < rowsJ && (ti != tj || r >= c)) {
      double* w = W + (size_t)(I0 + r) + (size_t)nn * (J0 + c);
      *w = *w - v;
    }
  });
}

// A pivot of W's factor at rounding level -- L_jj^2 <= n eps against W's unit prior variance, a
// new unit on top of another unit -- is no evidence of a positive definite W, whichever sign the
// rounding gave it: reported like a non-positive one.
__global__ __launch_bounds__(256) void krige_pivot_kernel(const double* L, int n, int* info) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double l = L[(size_t)j + (size_t)n * j];
  if (!(l * l > n * 2.220446049250313e-16)) atomicExch(info, 1);
}

// out += L_W Z (L_W lower, nn x nn; Z nn x c): tile row I needs the chunks k <= I only
struct TrmmArgs {
  const double* LW;
  const double* Z;
  int nn, c, nfmax;
  const int* col_s;
  const int* col_h;
  double* out;
  size_t ldo;
};

__global__ __launch_bounds__(256) void krige_trmm_kernel(TrmmArgs a) {
  __shared__ double SA[KB * KLD];
  __shared__ double SB[KB * KLD];
  const int ib = blockIdx.x, I0 = ib * KB, J0 = blockIdx.y * KB;
  const int rowsI = min(KB, a.nn - I0), colsJ = min(KB, a.c - J0);
  d4 acc[2][2];
  kg_zero(acc);
  double va[KU], vb[KU];
  kg_load(va, a.LW, a.nn, I0, 0, rowsI, min(KB, a.nn));
  kg_load(vb, a.Z, a.nn, 0, J0, min(KB, a.nn), colsJ);
  for (int kb = 0; kb <= ib; ++kb) {
    const int rowsK = min(KB, a.nn - kb * KB);
    kg_store<false>(SA, va, rowsI, rowsK, kb == ib);  // SA[r][k] = L_W[I0 + r, K0 + k]
    kg_store<true>(SB, vb, rowsK, colsJ);             // SB[c][k] = Z[K0 + k, J0 + c]
    __syncthreads();
    if (kb < ib) {
      const int K1 = (kb + 1) * KB, rowsK1 = min(KB, a.nn - K1);
      kg_load(va, a.LW, a.nn, I0, K1, rowsI, rowsK1);
      kg_load(vb, a.Z, a.nn, K1, J0, rowsK1, colsJ);
    }
    kg_mma(acc, SA, SB);
    __syncthreads();
  }
  kg_each(acc, [&](int r, int c, double v) {
    if (r < rowsI && c < colsJ) {
      double* o = a.out + ((size_t)a.col_s[J0 + c] * a.nfmax + a.col_h[J0 + c]) * a.ldo + (I0 + r);
      *o = *o + v;
    }
  });
}

// ---------------------------------------------------------------------------------------
// NNGP (R/predictLatentFactor.R:118-160): one wave per new unit.  The k nearest fitted units
// in (distance, index) order -- ties to the lower index, FNN's / a stable argsort's order --
// then per grid index in use the k x k system in registers (lane = row, wave_la.h):
// w = K11^-1 K12, F = 1 - w K12, and m = w eta[ind, h] for the index's pairs, 64 pairs at a time.
// ---------------------------------------------------------------------------------------
struct NnArgs {
  const double* coords;  // N x sdim: the fitted units, then the call's new units
  const double* Eta;     // S x np x nfmax
  const int* unit;       // nn: the new units of this launch among the call's, or null: 0 .. nn - 1
  size_t ldo;
  int np, nn, N, sdim, nfmax, k, ngroups;
  const double* g_alpha;  // ngroups
  const int* g_off;       // ngroups + 1, into col_s / col_h
  const int* col_s;
  const int* col_h;
  double* out;
  int* info;
  Key key;
  uint32_t stream;
};

template <int NM>
__global__ __launch_bounds__(64) void krige_nn_kernel(NnArgs a) {
  __shared__ double lds[NM * (NM + 1)];
  const int i = blockIdx.x, lane = threadIdx.x, np = a.np, N = a.N, k = a.k;
  const int ui = kg_unit(a.unit, i);
  // the k nearest: round q takes the smallest (d, j) above the previous round's
  double dsel = 0.0, dl = -1.0;
  int jsel = 0, jl = -1;
  for (int q = 0; q < k; ++q) {
    double bd = INFINITY;
    int bj = 0x7fffffff;
    for (int j = lane; j < np; j += 64) {
      const double d = kg_dist(a.coords, nullptr, N, a.sdim, np + ui, j);
      const bool after = d > dl || (d == dl && j > jl);
      if (after && (d < bd || (d == bd && j < bj))) bd = d, bj = j;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd, off);
      const int oj = __shfl_xor(bj, off);
      if (od < bd || (od == bd && oj < bj)) bd = od, bj = oj;
    }
    dl = bd;
    jl = bj;
    if (lane == q) dsel = bd, jsel = bj;
  }
  if (jl == 0x7fffffff) {  // not k finite distances (NaN coordinates): report, write nothing
    if (lane == 0) atomicExch(a.info, 2);
    return;
  }
  double dd[NM];  // distances among the neighbours: lane = row
#pragma unroll
  for (int c = 0; c < NM; ++c) {
    const int jc = __shfl(jsel, c);
    dd[c] = kg_dist(a.coords, nullptr, N, a.sdim, jsel, jc);
  }
  for (int g = 0; g < a.ngroups; ++g) {
    const double alpha = a.g_alpha[g];
    double w = 0.0, sF = 1.0;
    if (alpha > 0.0) {
      double A[NM], lt[NM], dinv;
#pragma unroll
      for (int c = 0; c < NM; ++c) A[c] = (lane < k && c < k) ? exp(-dd[c] / alpha) : (lane == c ? 1.0 : 0.0);
      const bool ok = wv_chol<NM>(A, dinv);
      if (!ok && lane == 0) atomicExch(a.info, 1);
      const double K12 = lane < k ? exp(-dsel / alpha) : 0.0;
      w = K12;
      wv_forward<NM>(A, dinv, w);
      wv_transpose<NM, true>(A, lt, lds);
      wv_backward_t<NM>(lt, dinv, w);
      sF = sqrt(1.0 - kg_wave_sum(w * K12));
    }
    for (int p0 = a.g_off[g]; p0 < a.g_off[g + 1]; p0 += 64) {
      const int p = p0 + lane;
      const bool valid = p < a.g_off[g + 1];
      const int s = valid ? a.col_s[p] : 0, h = valid ? a.col_h[p] : 0;
      const double* eta = a.Eta + ((size_t)s * a.nfmax + h) * np;
      double m = 0.0;
      for (int q = 0; q < k; ++q) {
        const double wq = __shfl(w, q);
        const int jq = __shfl(jsel, q);
        m = fma(wq, eta[jq], m);
      }
      if (valid)
        a.out[((size_t)s * a.nfmax + h) * a.ldo + i] =
            fma(sF, normal(a.key, (uint32_t)ui, (uint32_t)h, a.stream, (uint32_t)s), m);
    }
  }
}

}  // namespace

// R <- L^-1 R for the n x m matrix R (ld ldr): L (n x n, ld ldl) and ws as dense_potrf_lower
// left them (ws: the 64 x 64 diagonal-block inverses)
void dense_trsm_lower(hipStream_t st, const double* L, int n, int ldl, const double* ws, double* R, size_t ldr, int m) {
  if (n <= 0 || m <= 0) return;
  trsm_lower_kernel<<<(m + KB - 1) / KB, 256, 0, st>>>(L, ldl, n, ws, R, ldr, m);
  HIP_OK(hipGetLastError());
}

static void kg_mark(hipStream_t st, hipEvent_t* ev, int k) {
  if (ev) HIP_OK(hipEventRecord(ev[k], st));
}

void krige_launch_group(hipStream_t st, const KrigeDev& d, int mode, double a, int col0, int c, int* info,
                        hipEvent_t* ev) {
  const Key key{(uint32_t)d.seed, (uint32_t)(d.seed >> 32)};
  const int np = d.np, nn = d.nn;
  const int* cs = d.col_s + col0;
  const int* ch = d.col_h + col0;
  const int gy = std::min(c, 65535);
  const dim3 gz((nn + 255) / 256, gy);
  kg_mark(st, ev, 0);
  if (!(a > 0.0)) {  // out = z; predictMean: 0 (the output starts zeroed)
    if (mode != 0)
      krige_z_kernel<<<gz, 256, 0, st>>>(key, d.stream, nn, d.unit, d.nfmax, cs, ch, c, nullptr, d.out, d.ldo);
    HIP_OK(hipGetLastError());
    for (int k = 1; k <= KRIGE_GROUP_PHASES; ++k) kg_mark(st, ev, k);
    return;
  }
  const size_t big = (size_t)std::max(np, nn) * (mode == 2 ? std::max(np, nn) : np);
  krige_kernel_matrices<<<dim3((unsigned)((big + 255) / 256), mode == 2 ? 3 : 2), 256, 0, st>>>(
      d.coords, d.dist, np, nn, d.N, d.unit, d.sdim, a, 0, d.K11, d.R, d.W);
  krige_gather_kernel<<<dim3((np + 255) / 256, gy), 256, 0, st>>>(d.Eta, np, d.nfmax, cs, ch, c, d.R + (size_t)np * nn);
  if (mode == 2) krige_z_kernel<<<gz, 256, 0, st>>>(key, d.stream, nn, d.unit, d.nfmax, cs, ch, c, d.Z, nullptr, 0);
  HIP_OK(hipGetLastError());
  kg_mark(st, ev, 1);
  dense_potrf_lower(st, d.K11, np, np, d.ws1, info, 0, d.sync);
  kg_mark(st, ev, 2);
  dense_trsm_lower(st, d.K11, np, np, d.ws1, d.R, (size_t)np, nn + c);
  kg_mark(st, ev, 3);
  if (mode == 1) krige_colnorm_kernel<<<(nn + 3) / 4, 256, 0, st>>>(d.R, (size_t)np, np, nn, d.v);
  MeanArgs ma{d.R,  (size_t)np, d.R + (size_t)np * nn, (size_t)np, np, nn, c, d.nfmax, cs, ch, mode == 1 ? d.v : nullptr,
              d.unit, d.out, d.ldo, key, d.stream};
  krige_mean_kernel<<<dim3((nn + KB - 1) / KB, (c + KB - 1) / KB), 256, 0, st>>>(ma);
  HIP_OK(hipGetLastError());
  kg_mark(st, ev, 4);
  if (mode == 2) {
    const int nbk = (nn + KB - 1) / KB;
    krige_syrk_kernel<<<nbk * (nbk + 1) / 2, 256, 0, st>>>(d.R, (size_t)np, np, nn, d.W);
    HIP_OK(hipGetLastError());
    kg_mark(st, ev, 5);
    dense_potrf_lower(st, d.W, nn, nn, d.ws2, info + 1, 0, d.sync);
    krige_pivot_kernel<<<(nn + 255) / 256, 256, 0, st>>>(d.W, nn, info + 1);
    kg_mark(st, ev, 6);
    TrmmArgs ta{d.W, d.Z, nn, c, d.nfmax, cs, ch, d.out, d.ldo};
    krige_trmm_kernel<<<dim3(nbk, (c + KB - 1) / KB), 256, 0, st>>>(ta);
    HIP_OK(hipGetLastError());
    kg_mark(st, ev, 7);
  } else {
    for (int k = 5; k <= KRIGE_GROUP_PHASES; ++k) kg_mark(st, ev, k);
  }
}

// The kriging plan of a call that walks its new units in slabs (hmsc_predict_map, map.hip):
// krige_launch_group split at what does not depend on the new units.  Per grid value a > 0, once:
// K11 (lower), its factor with the diagonal-block inverses in ws, and Y = L^-1 E_g (np x c).
void krige_plan_group(hipStream_t st, const KrigeDev& d, double a, int col0, int c, double* K11, double* ws, double* Y,
                      int* info) {
  const int np = d.np;
  krige_kernel_matrices<<<dim3((unsigned)(((size_t)np * np + 255) / 256), 1), 256, 0, st>>>(
      d.coords, d.dist, np, 0, d.N, nullptr, d.sdim, a, 0, K11, nullptr, nullptr);
  krige_gather_kernel<<<dim3((np + 255) / 256, std::min(c, 65535)), 256, 0, st>>>(d.Eta, np, d.nfmax, d.col_s + col0,
                                                                                  d.col_h + col0, c, Y);
  HIP_OK(hipGetLastError());
  dense_potrf_lower(st, K11, np, np, ws, info, 0, d.sync);
  dense_trsm_lower(st, K11, np, np, ws, Y, (size_t)np, c);
}

// ... and per slab of d.nn new units (d.unit; mode 0 or 1): the K12 slab into d.R (np x nn), B = L^-1
// K12 in place, v (mode 1) and the mean product, written to d.out with ld d.ldo.  A column of B, of v
// and of the output is the same sum over the fitted units in index order as in krige_launch_group,
// whichever slab and tile it falls in.  ev (4 events, or null): K12, trsm, mean.
void krige_slab_group(hipStream_t st, const KrigeDev& d, int mode, double a, int col0, int c, const double* K11,
                      const double* ws, const double* Y, hipEvent_t* ev) {
  const Key key{(uint32_t)d.seed, (uint32_t)(d.seed >> 32)};
  const int np = d.np, nn = d.nn;
  kg_mark(st, ev, 0);
  krige_kernel_matrices<<<dim3((unsigned)(((size_t)np * nn + 255) / 256), 1), 256, 0, st>>>(
      d.coords, d.dist, np, nn, d.N, d.unit, d.sdim, a, 1, nullptr, d.R, nullptr);
  HIP_OK(hipGetLastError());
  kg_mark(st, ev, 1);
  dense_trsm_lower(st, K11, np, np, ws, d.R, (size_t)np, nn);
  kg_mark(st, ev, 2);
  if (mode == 1) krige_colnorm_kernel<<<(nn + 3) / 4, 256, 0, st>>>(d.R, (size_t)np, np, nn, d.v);
  MeanArgs ma{d.R,  (size_t)np, Y, (size_t)np, np, nn, c, d.nfmax, d.col_s + col0, d.col_h + col0,
              mode == 1 ? d.v : nullptr, d.unit, d.out, d.ldo, key, d.stream};
  krige_mean_kernel<<<dim3((nn + KB - 1) / KB, (c + KB - 1) / KB), 256, 0, st>>>(ma);
  HIP_OK(hipGetLastError());
  kg_mark(st, ev, 3);
}

void krige_launch_nn(hipStream_t st, const KrigeDev& d, int k, int ngroups, const double* g_alpha, const int* g_off,
                     int* info) {
  NnArgs a{d.coords, d.Eta, d.unit, d.ldo, d.np, d.nn, d.N, d.sdim, d.nfmax, k, ngroups, g_alpha, g_off, d.col_s,
           d.col_h, d.out, info, Key{(uint32_t)d.seed, (uint32_t)(d.seed >> 32)}, d.stream};
  with_bucket<8, 16, 24, 32>(wv_bucket(k),
                             [&](auto nm) { krige_nn_kernel<decltype(nm)::value><<<d.nn, 64, 0, st>>>(a); });
  HIP_OK(hipGetLastError());
}

}  // namespace hmsc
