// Community-level posterior summaries in one device pass (hmsc_predict_community in
// include/hmsc_amd.h): per posterior sample and site, weighted sums over a sample's whole row of
// species -- species richness, the summed response, community-weighted trait means -- and over the
// samples their count, mean, R's type-7 quantiles and the share of samples in which one site lies
// above another: plotGradient's numbers for measures "S", "Y" and "T" (R/plotGradient.R:93-138)
// without the ny x ns x nsamples stack of predict.
//
// predict_community_kernel (kernel A): one workgroup per (64-site tile of the slab, sample), 256
// threads.  The workgroup stages its site tile [X | Eta rows] once for its sample and walks the
// species tiles of 32 in ascending order, staging [Beta_s; Lambda_s] and the tile's W rows per
// tile.  Thread (site ii = t & 63, lane l = t >> 6) forms its 8 cells per tile as predict_kernel
// does (predict_cell.h: the same fma chain, cell index i + ny j and Philox counters, so p_j is the
// double hmsc_predict writes) and folds g(p_j) into nw + 1 register accumulators.
//
// The summation order, which depends on ns alone (not on ny, the slab, the samples or the grid):
//   lane l = 0 .. 3 of a site takes the species j with j mod 4 = l, in ascending j
//     (j = 32 T + l + 4 q: tiles T ascending, q = 0 .. 7 ascending within a tile);
//   den_l = 0.0, then den_l = den_l + g(p_j) for each of them;
//   num_l,m = 0.0, then num_l,m = num_l,m + fl(g(p_j) * W[j, m]) for those with W[j, m] != 0
//     (one rounding for the product, one for the add; a zero weight is a select: no add at all);
//   den = ((den_0 + den_1) + den_2) + den_3, num_m likewise (through LDS, one fixed order);
//   C[s, i, m] = normalise[m] ? num_m / den : num_m.
// No atomics, nothing crosses a workgroup.  C goes to a device slab [s][m][site of the slab] (lanes
// along sites), to comm when asked, and the rows named in pairs to a small [s][m][pair slot] buffer.
//
// LDS: the two tiles of predict_kernel (98,816 B at K = 128) and 32 W rows of the padded column
// count (4 KB at 16); the 4 x 64 x (nw + 1) partials of the final reduction reuse the tiles' space
// once the species loop is done.
//
// community_stat_kernel: one (site, column) per thread over the slab: n and the sequential sum in
// sample order (NaN skipped), then the bisection selection of quantile_select.h, the very code
// predict_quantile_kernel runs.
//
// Rows: a launch serves the rows PredArgs::{row0, ny, nyTotal} name, one slab of slab_engine.h,
// whose CommunityBlock both kernels take as it stands; the slab is the launch's own rows, comm and
// the pairs' sites are the whole call's (row0 + i against nyTotal).  Pi: PredArgs::ldPi, as in
// summary.hip.  The host walks the sites in slabs of whole 64-row tiles that fit the scratch
// budget and counts the pairs from the pair buffer; no result depends on the slab.
#include <cmath>
#include <vector>

#include "quantile_select.h"
#include "slab_engine.h"

namespace hmsc {

// NW: the column count padded to 1, 4, 8 or 16 (the surplus columns carry zero weights)
// ntile: the launch's site tiles, workgroup b serves tile b % ntile of sample b / ntile
// work: doubles of LDS the tiles and the final reduction share; W's rows follow
template <int NW>
__global__ __launch_bounds__(256) void predict_community_kernel(PredArgs a, CommunityBlock g, int ntile, int work) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x;
  const int i0 = (int)(blockIdx.x % ntile) * PT_I, s = (int)(blockIdx.x / ntile);
  const int ny = a.ny, ns = a.ns, K = a.K;
  const int LD = K | 1;
  double* sA = smem;
  double* sB = smem + PT_I * LD;
  double* sW = smem + work;  // [column][species of the tile]
  const int ii = t & 63, jb = t >> 6;
  const int i = i0 + ii;
  const bool live = i < ny;
  double num[NW], den = 0.0;
#pragma unroll
  for (int m = 0; m < NW; ++m) num[m] = 0.0;
  stage_sites(a, sA, LD, i0, s, 0, t);
  for (int j0 = 0; j0 < ns; j0 += PT_J) {
    if (j0 > 0) __syncthreads();  // the previous species tile is read out
    stage_species(a, sB, j0, s, t);
    for (int p = t; p < NW * PT_J; p += 256) {
      const int m = p / PT_J, j = j0 + p % PT_J;
      sW[p] = m < g.nw && j < ns ? g.W[j + (size_t)ns * m] : 0.0;
    }
    __syncthreads();
    if (!live) continue;
    double acc[8];
    linear_predictor(sA, sB, LD, K, ii, jb, acc);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int jj = jb + 4 * q, j = j0 + jj;
      if (j >= ns) continue;
      const uint32_t cell = (uint32_t)pred_cell_index(a, i, j);
      const double z = predict_cell(a, acc[q], a.sigma[(size_t)s * ns + j], a.family[j], a.yscale[2 * j],
                                    a.yscale[2 * j + 1], cell, s);
      const double gz = g.transform ? exp(z) : z;
      {
#pragma clang fp contract(off)
        den = den + gz;
#pragma unroll
        for (int m = 0; m < NW; ++m) {
          const double w = sW[m * PT_J + jj];
          const double term = gz * w;
          if (w != 0.0) num[m] = num[m] + term;
        }
      }
    }
  }
  __syncthreads();  // the tiles are read out: their space takes the partials [column][lane][site]
  double* red = smem;
#pragma unroll
  for (int m = 0; m < NW; ++m) red[(m * 4 + jb) * PT_I + ii] = num[m];
  red[(NW * 4 + jb) * PT_I + ii] = den;
  __syncthreads();
  for (int p = t; p < PT_I * g.nw; p += 256) {
    const int si = p & 63, m = p >> 6, is = i0 + si;
    if (is >= ny) continue;
    const double* rn = red + m * 4 * PT_I + si;
    const double* rd = red + NW * 4 * PT_I + si;
    double c;
    {
#pragma clang fp contract(off)
      const double n4 = ((rn[0] + rn[PT_I]) + rn[2 * PT_I]) + rn[3 * PT_I];
      const double d4 = ((rd[0] + rd[PT_I]) + rd[2 * PT_I]) + rd[3 * PT_I];
      c = g.normalise[m] ? n4 / d4 : n4;
    }
    const size_t sm = (size_t)s * g.nw + m;
    g.slab[sm * ny + is] = c;
    if (g.comm) g.comm[sm * a.nyTotal + a.row0 + is] = c;
    for (int k = 0; k < g.nslots; ++k)
      if (g.pair_site[k] == a.row0 + is) g.pairbuf[sm * g.nslots + k] = c;
  }
}

template <int NQ>
__global__ __launch_bounds__(256) void community_stat_kernel(PredArgs a, CommunityBlock g) {
  const size_t cells = (size_t)g.nw * a.ny;
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const int m = (int)(c / a.ny), i = a.row0 + (int)(c % a.ny);
  const size_t out = (size_t)i + (size_t)a.nyTotal * m, plane = (size_t)a.nyTotal * g.nw;
  const double* x = g.slab + c;
  int n = 0;
  double sum = 0.0;
  for (int s = 0; s < a.nsamples; ++s) {
    const double v = x[(size_t)s * cells];
    if (v == v) sum += v, n += 1;
  }
  g.n[out] = n;
  g.mean[out] = sum / (double)n;  // 0 / 0 = NaN when every sample is NaN
  if (g.nq == 0) return;
  if (n == 0) {
    for (int q = 0; q < g.nq; ++q) g.quant[q * plane + out] = NAN;
    return;
  }
  select_quantiles<NQ>(x, cells, a.nsamples, n, g.probs, g.nq, g.quant + out, plane);
}

void launch_values(hipStream_t st, const PredArgs& a, const CommunityBlock& g) {
  const int NW = g.nw <= 1 ? 1 : g.nw <= 4 ? 4 : g.nw <= 8 ? 8 : 16;
  const int ntile = (a.ny + PT_I - 1) / PT_I;
  const int work = (int)std::max((size_t)PT_I * (a.K | 1) + (size_t)a.K * PT_J, (size_t)(NW + 1) * 4 * PT_I);
  const size_t lds = ((size_t)work + (size_t)NW * PT_J) * sizeof(double);
  HMSC_REQUIRE((uint64_t)ntile * (uint64_t)a.nsamples <= BLOCKS_MAX,
               "internal: a slab's 64-row tiles times the samples exceed 2^23 (plan_slab_rows caps them)");
  const unsigned ga = (unsigned)((size_t)ntile * a.nsamples);
  if (NW == 1) predict_community_kernel<1><<<ga, 256, lds, st>>>(a, g, ntile, work);
  else if (NW == 4) predict_community_kernel<4><<<ga, 256, lds, st>>>(a, g, ntile, work);
  else if (NW == 8) predict_community_kernel<8><<<ga, 256, lds, st>>>(a, g, ntile, work);
  else predict_community_kernel<16><<<ga, 256, lds, st>>>(a, g, ntile, work);
  HIP_OK(hipGetLastError());
}

void launch_statistics(hipStream_t st, const PredArgs& a, const CommunityBlock& g) {
  const unsigned gq = (unsigned)(((size_t)g.nw * a.ny + 255) / 256);
  if (g.nq <= 1) community_stat_kernel<1><<<gq, 256, 0, st>>>(a, g);
  else if (g.nq <= 2) community_stat_kernel<2><<<gq, 256, 0, st>>>(a, g);
  else if (g.nq <= 4) community_stat_kernel<4><<<gq, 256, 0, st>>>(a, g);
  else community_stat_kernel<8><<<gq, 256, 0, st>>>(a, g);
  HIP_OK(hipGetLastError());
}

static thread_local double g_community_ms[3] = {0.0, 0.0, 0.0};
void community_last_timing(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_community_ms[k];
}

// host side: check, plan, upload, the engine's walk, copy back; the pairs are counted here from the
// pair buffer (called by hmsc_predict_community in capi.cpp).  Timing slots: uploads; kernel A;
// statistics kernels, the copy back and the pair count.
void run_predict_community(const hmsc_predict_args* p, const hmsc_community_args* c, int32_t* n, double* mean,
                           double* quant, double* pr, double* comm) {
  check_pred_limits(p);
  HMSC_REQUIRE(p->ny > 0 && p->ns > 0, "predict_community: ny and ns must be positive");
  HMSC_REQUIRE(p->nsamples >= 1, "predict_community: nsamples must be at least 1");
  CommunityBlock g;
  check_community("predict_community", c, p->ny, false, n, mean, quant, pr, g);
  const size_t S = p->nsamples, nw = g.nw, npairs = c->npairs;
  const size_t slab_rows =
      plan_slab_rows("predict_community", " of the community columns", p->ny, S, nw, 0, c->scratch_bytes, true);
  HMSC_REQUIRE(S <= BLOCKS_MAX, "predict_community: at most 2^23 samples in one call");
  DeviceGuard dg(p->device);
  std::vector<int> pi0;  // (source of a copy on the stream: before its owner)
  std::vector<double> hpairs(S * nw * 2 * npairs);
  DeviceOwner own;
  const hipStream_t st = own.stream();
  double ms[3] = {0.0, 0.0, 0.0};
  PredArgs a{};
  timed(st, ms[0], [&] {
    a = upload_pred_args(p, own, st, pi0);
    alloc(own, st, a, slab_rows, c->W, comm != nullptr, g);
  });
  run_slabs(st, a, slab_rows, g, ms[1], ms[2]);
  const auto t0 = std::chrono::steady_clock::now();
  copy_out(st, a, g, n, mean, quant);
  if (comm) HIP_OK(hipMemcpyAsync(comm, g.comm, S * p->ny * nw * 8, hipMemcpyDeviceToHost, st));
  if (npairs > 0) HIP_OK(hipMemcpyAsync(hpairs.data(), g.pairbuf, hpairs.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  // Pr[C[, b, m] > C[, a, m]]: NaN when either value is NaN in any sample (R's mean of a logical with NA)
  for (size_t k = 0; k < npairs; ++k)
    for (size_t m = 0; m < nw; ++m) {
      size_t above = 0;
      bool nan = false;
      for (size_t s = 0; s < S; ++s) {
        const double* row = hpairs.data() + (s * nw + m) * 2 * npairs;
        const double va = row[2 * k], vb = row[2 * k + 1];
        nan = nan || va != va || vb != vb;
        above += vb > va ? 1 : 0;
      }
      pr[k + npairs * m] = nan ? NAN : (double)above / (double)S;
    }
  ms[2] += ms_since(t0);
  for (int k = 0; k < 3; ++k) g_community_ms[k] = ms[k];
}

}  // namespace hmsc
