// Posterior predictive summaries in one device pass (hmsc_predict_summary in include/hmsc_amd.h):
// per cell the posterior mean, the share of positive values and the count of non-NaN values over
// all samples of predict.Hmsc, and R's type-7 quantiles for flagged species columns -- what
// evaluateModelFit (R/evaluateModelFit.R) and plotGradient's credible intervals take from the
// ny x ns x nsamples stack of computePredictedValues, without the stack.
//
// predict_summary_kernel: grid (site tiles of the launch's rows, species tiles), tile 64 x 32, 256
// threads, 8 cells per thread as predict_kernel; the sample loop runs inside the workgroup,
// s = 0 .. S - 1 in order.
// The X columns of the site tile and its units (Pi) are staged in LDS once, each sample's Eta rows
// and its K x 32 block [Beta_s; Lambda_s] per sample; a column's family and YScalePar stay in
// registers.  Every value is predict_cell's (predict_cell.h) of the same
// fma chain, cell index and counters as predict_kernel: the double hmsc_predict would have
// written.  A cell keeps in registers sum (sequential fp64 adds in sample order, NaN skipped), n
// and pos; no atomics, nothing crosses a workgroup, so the summation order depends on the sample
// index alone.
//
// Quantiles: for flagged columns the kernel also stores each value to a slab [s][column slot][row
// of the launch] (lanes along sites: coalesced).  predict_quantile_kernel takes one cell per thread
// and finds the order statistics of rank floor(h) and ceil(h), h = (n - 1) p, by bisection over
// the order-preserving 64-bit key of the double (quantile_select.h, shared with community.hip):
// 64 counting passes fix the key of x_(floor h)
// bit by bit for all probabilities of the call at once, one more pass finds the smallest value
// above it.  Reads only, all lanes in lockstep, nothing indexed at run time (no scratch memory);
// exact and deterministic.
//
// Rows: a launch serves the rows PredArgs::{row0, ny, nyTotal} name, one slab of slab_engine.h,
// whose CellBlock both kernels take as it stands.  Pi reaches the kernels through PredArgs::ldPi
// (one field; the other way, re-laying the whole call's Pi slab after slab on the host, was more
// code): this entry walks the whole call's table at row0 with ldPi = nyTotal, its Eta and np the
// whole posterior's.  The host walks the sites in slabs of whole 64-row tiles that fit the scratch
// budget; a cell's results do not depend on the slab it falls in.
#include <cmath>
#include <vector>

#include "quantile_select.h"
#include "slab_engine.h"

namespace hmsc {

__global__ __launch_bounds__(256) void predict_summary_kernel(PredArgs a, CellBlock g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x, i0 = blockIdx.x * PT_I, j0 = blockIdx.y * PT_J;
  const int ny = a.ny, ns = a.ns, K = a.K, S = a.nsamples;
  const int LD = K | 1;
  double* sA = smem;
  double* sB = smem + PT_I * LD;
  const int ii = t & 63, jb = t >> 6;
  const int i = i0 + ii;
  const bool live = i < ny;
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
    sPi[p] = i0 + si < ny ? a.Pi[i0 + si + (size_t)a.ldPi * r] : 0;
  }
  __syncthreads();
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
      // (one product by ny: the form with a per-sample stride held two more scalars over the loop
      // and measured 1 % slower)
      if (slot[q] >= 0) g.slab[((size_t)s * g.nslot + slot[q]) * ny + i] = z;
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

// one cell per thread; the selection is quantile_select.h's
template <int NQ>
__global__ __launch_bounds__(256) void predict_quantile_kernel(PredArgs a, CellBlock g) {
  const size_t cells = (size_t)g.nslot * a.ny;
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const int sl = (int)(c / a.ny), i = (int)(c % a.ny), j = g.cols[sl];
  const size_t out = pred_cell_index(a, i, j), plane = (size_t)a.nyTotal * a.ns;
  const int n = g.n[out];
  if (n == 0) {
    for (int q = 0; q < g.nq; ++q) g.quant[q * plane + out] = NAN;
    return;
  }
  select_quantiles<NQ>(g.slab + c, cells, a.nsamples, n, g.probs, g.nq, g.quant + out, plane);
}

void launch_values(hipStream_t st, const PredArgs& a, const CellBlock& g) {
  const size_t lds = pred_lds_bytes(a.K) + (size_t)PT_I * a.nr * sizeof(int);
  predict_summary_kernel<<<dim3((unsigned)((a.ny + PT_I - 1) / PT_I), (unsigned)((a.ns + PT_J - 1) / PT_J)), 256, lds,
                           st>>>(a, g);
  HIP_OK(hipGetLastError());
}

void launch_statistics(hipStream_t st, const PredArgs& a, const CellBlock& g) {
  if (g.nslot == 0) return;  // (a flagged column implies nq > 0)
  const unsigned gq = (unsigned)(((size_t)g.nslot * a.ny + 255) / 256);
  if (g.nq <= 1) predict_quantile_kernel<1><<<gq, 256, 0, st>>>(a, g);
  else if (g.nq <= 2) predict_quantile_kernel<2><<<gq, 256, 0, st>>>(a, g);
  else if (g.nq <= 4) predict_quantile_kernel<4><<<gq, 256, 0, st>>>(a, g);
  else predict_quantile_kernel<8><<<gq, 256, 0, st>>>(a, g);
  HIP_OK(hipGetLastError());
}

static thread_local double g_summary_ms[3] = {0.0, 0.0, 0.0};
void summary_last_timing(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_summary_ms[k];
}

// host side: check, plan, upload, the engine's walk, copy back (called by hmsc_predict_summary in
// capi.cpp).  Timing slots: uploads; summary kernels; quantile kernels and the copy back.
void run_predict_summary(const hmsc_predict_args* p, const hmsc_summary_args* q, double* mean, double* occ, int32_t* n,
                         double* quant) {
  check_pred_limits(p);
  HMSC_REQUIRE(p->ny > 0 && p->ns > 0, "predict_summary: ny and ns must be positive");
  HMSC_REQUIRE(p->nsamples >= 1, "predict_summary: nsamples must be at least 1");
  CellBlock g;
  std::vector<int> slot, cols, pi0;  // (sources of copies on the stream: before its owner)
  check_cells("predict_summary", q, p->ns, quant, g, slot, cols);
  const size_t slab_rows = plan_slab_rows("predict_summary", " of the flagged columns", p->ny, p->nsamples, g.nslot, 0,
                                          q ? q->scratch_bytes : 0, false);
  DeviceGuard dg(p->device);
  DeviceOwner own;
  const hipStream_t st = own.stream();
  double ms[3] = {0.0, 0.0, 0.0};
  PredArgs a{};
  timed(st, ms[0], [&] {
    a = upload_pred_args(p, own, st, pi0);
    alloc(own, st, a, slab_rows, slot, cols, g);
  });
  run_slabs(st, a, slab_rows, g, ms[1], ms[2]);
  timed(st, ms[2], [&] { copy_out(st, a, g, mean, occ, n, quant); });
  for (int k = 0; k < 3; ++k) g_summary_ms[k] = ms[k];
}

}  // namespace hmsc
