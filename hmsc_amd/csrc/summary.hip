// Posterior predictive summaries in one device pass (hmsc_predict_summary in include/hmsc_amd.h):
// per cell the posterior mean, the share of positive values and the count of non-NaN values over
// all samples of predict.Hmsc, and R's type-7 quantiles for flagged species columns -- what
// evaluateModelFit (R/evaluateModelFit.R) and plotGradient's credible intervals take from the
// ny x ns x nsamples stack of computePredictedValues, without the stack.
//
// predict_summary_kernel: grid (site tiles, species tiles), tile 64 x 32, 256 threads, 8 cells per
// thread as predict_kernel; the sample loop runs inside the workgroup, s = 0 .. S - 1 in order.
// The X columns of the site tile and its units (Pi) are staged in LDS once, each sample's Eta rows
// and its K x 32 block [Beta_s; Lambda_s] per sample; a column's family and YScalePar stay in
// registers.  Every value is predict_cell's (predict_cell.h) of the same
// fma chain, cell index and counters as predict_kernel: the double hmsc_predict would have
// written.  A cell keeps in registers sum (sequential fp64 adds in sample order, NaN skipped), n
// and pos; no atomics, nothing crosses a workgroup, so the summation order depends on the sample
// index alone.
//
// Quantiles: for flagged columns the kernel also stores each value to a slab [s][column slot][site
// of the slab] (lanes along sites: coalesced).  predict_quantile_kernel takes one cell per thread
// and finds the order statistics of rank floor(h) and ceil(h), h = (n - 1) p, by bisection over
// the order-preserving 64-bit key of the double (quantile_select.h, shared with community.hip):
// 64 counting passes fix the key of x_(floor h)
// bit by bit for all probabilities of the call at once, one more pass finds the smallest value
// above it.  Reads only, all lanes in lockstep, nothing indexed at run time (no scratch memory);
// exact and deterministic.  The host walks the sites in slabs of whole 64-row tiles that fit the
// scratch budget; a cell's results do not depend on the slab it falls in.
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "predict_cell.h"
#include "quantile_select.h"

namespace hmsc {

struct SumArgs {
  PredArgs p;
  int i_lo, rows;       // the slab: sites i_lo .. i_lo + rows - 1
  int nslot;            // flagged columns
  const int* slot;      // ns: a flagged column's slot 0 .. nslot - 1, else -1
  double* slab;         // nsamples x nslot x rows (NULL: no quantiles)
  double* mean;         // nyTotal x ns, this launch's rows from p.row0
  double* occ;          // nyTotal x ns
  int* n;               // nyTotal x ns
};

__global__ __launch_bounds__(256) void predict_summary_kernel(SumArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const PredArgs& a = g.p;
  const int t = threadIdx.x, i0 = g.i_lo + blockIdx.x * PT_I, j0 = blockIdx.y * PT_J;
  const int ny = a.ny, ns = a.ns, K = a.K, S = a.nsamples;
  const int LD = K | 1;
  double* sA = smem;
  double* sB = smem + PT_I * LD;
  const int ii = t & 63, jb = t >> 6;
  const int i = i0 + ii;
  const bool live = i < ny && i < g.i_lo + g.rows;
  int* sPi = (int*)(sB + K * PT_J);     // [level][site]: the tile's units, staged once
  double sum[8], ym[8], ysd[8];
  int cnt[8], pos[8], fam[8], slot[8];  // a column's constants stay in registers over the samples
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int j = min(j0 + jb + 4 * q, ns - 1);
    sum[q] = 0.0, cnt[q] = 0, pos[q] = 0;
    fam[q] = a.family[j], ym[q] = a.yscale[2 * j], ysd[q] = a.yscale[2 * j + 1];
    slot[q] = g.slab != nullptr ? g.slot[j] : -1;
  }
  // the X part of sA (k < nc) and the units: once
  for (int p = t; p < PT_I * a.nc; p += 256) {
    const int si = p % PT_I, k = p / PT_I;
    sA[si * LD + k] = i0 + si < ny ? a.X[(size_t)(a.row0 + i0 + si) + (size_t)a.nyTotal * k] : 0.0;
  }
  for (int p = t; p < PT_I * a.nr; p += 256) {
    const int si = p % PT_I, r = p / PT_I;
    sPi[p] = i0 + si < ny ? a.Pi[i0 + si + (size_t)ny * r] : 0;
  }
  __syncthreads();
  const size_t scell = (size_t)g.nslot * g.rows;  // cells of one sample's slab
  for (int s = 0; s < S; ++s) {
    double sg[8];  // (issued ahead of the staging, whose latency they share)
#pragma unroll
    for (int q = 0; q < 8; ++q) sg[q] = a.sigma[(size_t)s * ns + min(j0 + jb + 4 * q, ns - 1)];
    if (s > 0) __syncthreads();  // the previous sample's tiles are read out
    stage_sites(a, sA, LD, i0, s, a.nc, t, sPi);
    stage_species(a, sB, j0, s, t);
    __syncthreads();
    if (!live) continue;
    double acc[8];
    linear_predictor(sA, sB, LD, K, ii, jb, acc);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = j0 + jb + 4 * q;
      if (j >= ns) continue;
      const uint32_t cell = (uint32_t)pred_cell_index(a, i, j);
      const double z = predict_cell(a, acc[q], sg[q], fam[q], ym[q], ysd[q], cell, s);
      if (z == z) {
        sum[q] += z;
        cnt[q] += 1;
        pos[q] += z > 0.0 ? 1 : 0;
      }
      if (slot[q] >= 0) g.slab[(size_t)s * scell + (size_t)slot[q] * g.rows + (i - g.i_lo)] = z;
    }
  }
  if (!live) return;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int j = j0 + jb + 4 * q;
    if (j >= ns) continue;
    const size_t c = pred_cell_index(a, i, j);
    g.mean[c] = sum[q] / (double)cnt[q];  // 0 / 0 = NaN when every sample is NaN
    g.occ[c] = (double)pos[q] / (double)cnt[q];
    g.n[c] = cnt[q];
  }
}

struct QuantArgs {
  int ny, ns, S, i_lo, rows, nslot, nq;  // ny: the rows of n and quant (the whole call's); i_lo: the slab's first
  double probs[SUM_NQ_MAX];
  const int* cols;     // nslot: the species column of a slot
  const int* n;        // ny x ns: the summary kernel's counts
  const double* slab;  // S x nslot x rows
  double* quant;       // nq x ny x ns
};

// one cell per thread; the selection is quantile_select.h's
template <int NQ>
__global__ __launch_bounds__(256) void predict_quantile_kernel(QuantArgs a) {
  const size_t cells = (size_t)a.nslot * a.rows;
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const int sl = (int)(c / a.rows), i = a.i_lo + (int)(c % a.rows), j = a.cols[sl];
  const size_t out = (size_t)i + (size_t)a.ny * j, plane = (size_t)a.ny * a.ns;
  const int n = a.n[out];
  if (n == 0) {
    for (int q = 0; q < a.nq; ++q) a.quant[q * plane + out] = NAN;
    return;
  }
  select_quantiles<NQ>(a.slab + c, cells, a.S, n, a.probs, a.nq, a.quant + out, plane);
}

template <class QA>
static void launch_quantile_kernel(hipStream_t st, const QA& qa, int nq, size_t cells) {
  const unsigned gq = (unsigned)((cells + 255) / 256);
  if (nq <= 1) predict_quantile_kernel<1><<<gq, 256, 0, st>>>(qa);
  else if (nq <= 2) predict_quantile_kernel<2><<<gq, 256, 0, st>>>(qa);
  else if (nq <= 4) predict_quantile_kernel<4><<<gq, 256, 0, st>>>(qa);
  else predict_quantile_kernel<8><<<gq, 256, 0, st>>>(qa);
  HIP_OK(hipGetLastError());
}

// one slab of a map (predict_cell.h): the launch's own rows 0 .. a.ny - 1 are the slab
void summary_launch_slab(hipStream_t st, const PredArgs& a, const MapSummary& m) {
  SumArgs g{};
  g.p = a;
  g.i_lo = 0, g.rows = a.ny;
  g.nslot = m.nslot, g.slot = m.slot, g.slab = m.nslot > 0 ? m.slab : nullptr;
  g.mean = m.mean, g.occ = m.occ, g.n = m.n;
  const size_t lds = pred_lds_bytes(a.K) + (size_t)PT_I * a.nr * sizeof(int);
  predict_summary_kernel<<<dim3((unsigned)((a.ny + PT_I - 1) / PT_I), (unsigned)((a.ns + PT_J - 1) / PT_J)), 256, lds,
                           st>>>(g);
  HIP_OK(hipGetLastError());
}

void summary_launch_quantiles(hipStream_t st, const PredArgs& a, const MapSummary& m) {
  if (m.nslot == 0 || m.nq == 0) return;
  QuantArgs qa{};
  qa.ny = a.nyTotal, qa.ns = a.ns, qa.S = a.nsamples, qa.i_lo = a.row0, qa.rows = a.ny;
  qa.nslot = m.nslot, qa.nq = m.nq;
  for (int k = 0; k < m.nq; ++k) qa.probs[k] = m.probs[k];
  qa.cols = m.cols, qa.n = m.n, qa.slab = m.slab, qa.quant = m.quant;
  launch_quantile_kernel(st, qa, m.nq, (size_t)m.nslot * a.ny);
}

static thread_local double g_summary_ms[3] = {0.0, 0.0, 0.0};
void summary_last_timing(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_summary_ms[k];
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

constexpr uint64_t SUM_SCRATCH_DEFAULT = (uint64_t)1 << 30;

// host side: upload, then per slab of site tiles the summary kernel and the quantile kernel
// (called by hmsc_predict_summary in capi.cpp)
void run_predict_summary(const hmsc_predict_args* p, const hmsc_summary_args* q, double* mean, double* occ, int32_t* n,
                         double* quant) {
  const int K = check_pred_limits(p);
  HMSC_REQUIRE(p->ny > 0 && p->ns > 0, "predict_summary: ny and ns must be positive");
  HMSC_REQUIRE(p->nsamples >= 1, "predict_summary: nsamples must be at least 1");
  const int nq = q ? q->nq : 0;
  HMSC_REQUIRE(nq >= 0 && nq <= SUM_NQ_MAX, "predict_summary: at most 8 probabilities (nq = " + std::to_string(nq) + ")");
  HMSC_REQUIRE(nq == 0 || (q->probs != nullptr && q->qcols != nullptr && quant != nullptr),
               "predict_summary: nq > 0 needs probs, qcols and quant");
  QuantArgs qa{};
  for (int k = 0; k < nq; ++k) {
    HMSC_REQUIRE(q->probs[k] >= 0.0 && q->probs[k] <= 1.0, "predict_summary: every probability must lie in [0, 1]");
    qa.probs[k] = q->probs[k];
  }
  const size_t S = p->nsamples, ny = p->ny, ns = p->ns;
  std::vector<int> slot(ns, -1), cols;
  if (nq > 0)
    for (size_t j = 0; j < ns; ++j)
      if (q->qcols[j]) slot[j] = (int)cols.size(), cols.push_back((int)j);
  const size_t nslot = cols.size();
  const size_t ntiles = (ny + PT_I - 1) / PT_I;
  size_t slab_tiles = ntiles;
  if (nslot > 0) {
    const uint64_t budget = q->scratch_bytes ? q->scratch_bytes : SUM_SCRATCH_DEFAULT;
    const uint64_t tile_bytes = (uint64_t)S * PT_I * nslot * 8;
    HMSC_REQUIRE(tile_bytes <= budget, "predict_summary: one 64-row tile of the flagged columns needs " +
                                           std::to_string(tile_bytes) + " bytes of scratch, scratch_bytes allows " +
                                           std::to_string(budget));
    slab_tiles = std::min<uint64_t>(ntiles, budget / tile_bytes);
  }
  const size_t slab_rows = std::min(ny, slab_tiles * PT_I);

  DeviceGuard dg(p->device);
  std::vector<int> pi0;  // (source of a copy on the stream: before its owner)
  DeviceOwner own;
  const hipStream_t st = own.stream();
  auto t0 = std::chrono::steady_clock::now();
  SumArgs g{};
  g.p = upload_pred_args(p, own, st, pi0);
  g.nslot = (int)nslot;
  g.slot = own.upload(slot.data(), ns, st);
  g.mean = own.alloc<double>(ny * ns);
  g.occ = own.alloc<double>(ny * ns);
  g.n = own.alloc<int>(ny * ns);
  double* dquant = nullptr;
  if (nq > 0) {
    dquant = own.alloc<double>((size_t)nq * ny * ns);
    HIP_OK(hipMemsetAsync(dquant, 0xFF, (size_t)nq * ny * ns * 8, st));  // NaN off the flagged columns
  }
  if (nslot > 0) {
    g.slab = own.alloc<double>(S * nslot * slab_rows);
    qa.cols = own.upload(cols.data(), nslot, st);
  }
  qa.ny = p->ny, qa.ns = p->ns, qa.S = p->nsamples, qa.nslot = (int)nslot, qa.nq = nq;
  qa.n = g.n, qa.slab = g.slab, qa.quant = dquant;
  HIP_OK(hipStreamSynchronize(st));
  double up_ms = ms_since(t0), sum_ms = 0.0, q_ms = 0.0;
  const unsigned gy = (unsigned)((ns + PT_J - 1) / PT_J);
  for (size_t i_lo = 0; i_lo < ny; i_lo += slab_rows) {
    const size_t rows = std::min(slab_rows, ny - i_lo);
    t0 = std::chrono::steady_clock::now();
    g.i_lo = (int)i_lo, g.rows = (int)rows;
    const size_t lds = pred_lds_bytes(K) + (size_t)PT_I * p->nr * sizeof(int);
    predict_summary_kernel<<<dim3((unsigned)((rows + PT_I - 1) / PT_I), gy), 256, lds, st>>>(g);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    sum_ms += ms_since(t0);
    if (nslot == 0) continue;
    t0 = std::chrono::steady_clock::now();
    qa.i_lo = (int)i_lo, qa.rows = (int)rows;
    launch_quantile_kernel(st, qa, nq, nslot * rows);
    HIP_OK(hipStreamSynchronize(st));
    q_ms += ms_since(t0);
  }
  t0 = std::chrono::steady_clock::now();
  HIP_OK(hipMemcpyAsync(mean, g.mean, ny * ns * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(occ, g.occ, ny * ns * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(n, g.n, ny * ns * 4, hipMemcpyDeviceToHost, st));
  if (nq > 0) HIP_OK(hipMemcpyAsync(quant, dquant, (size_t)nq * ny * ns * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  q_ms += ms_since(t0);
  g_summary_ms[0] = up_ms, g_summary_ms[1] = sum_ms, g_summary_ms[2] = q_ms;
}

}  // namespace hmsc
