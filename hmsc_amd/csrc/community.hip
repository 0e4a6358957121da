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
// predict_quantile_kernel runs.  The host walks the sites in slabs of whole 64-row tiles that fit
// the scratch budget and counts the pairs from the pair buffer; no result depends on the slab.
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "predict_cell.h"
#include "quantile_select.h"

namespace hmsc {

constexpr int COM_NW_MAX = 16, COM_NPAIR_MAX = 8;
constexpr uint64_t COM_SCRATCH_DEFAULT = (uint64_t)1 << 30;
constexpr uint64_t COM_BLOCKS_MAX = (uint64_t)1 << 23;  // workgroups of one launch

struct ComArgs {
  PredArgs p;
  int i_lo, rows;  // the slab: sites i_lo .. i_lo + rows - 1
  int ntile;       // its site tiles: workgroup b serves tile b % ntile of sample b / ntile
  int nw, transform, nslots;
  int work;        // doubles of LDS the tiles and the final reduction share; W's rows follow
  int pair_site[2 * COM_NPAIR_MAX];
  int normalise[COM_NW_MAX];
  const double* W;  // ns x nw
  double* slab;     // nsamples x nw x rows
  double* comm;     // nsamples x (ny x nw), or NULL
  double* pairbuf;  // nsamples x nw x nslots
};

// NW: the column count padded to 1, 4, 8 or 16 (the surplus columns carry zero weights)
template <int NW>
__global__ __launch_bounds__(256) void predict_community_kernel(ComArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const PredArgs& a = g.p;
  const int t = threadIdx.x;
  const int i0 = g.i_lo + (int)(blockIdx.x % g.ntile) * PT_I, s = (int)(blockIdx.x / g.ntile);
  const int ny = a.ny, ns = a.ns, K = a.K;
  const int LD = K | 1;
  double* sA = smem;
  double* sB = smem + PT_I * LD;
  double* sW = smem + g.work;  // [column][species of the tile]
  const int ii = t & 63, jb = t >> 6;
  const int i = i0 + ii;
  const int i_end = min(ny, g.i_lo + g.rows);
  const bool live = i < i_end;
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
    if (is >= i_end) continue;
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
    g.slab[sm * g.rows + (is - g.i_lo)] = c;
    if (g.comm) g.comm[sm * ny + is] = c;
    for (int k = 0; k < g.nslots; ++k)
      if (g.pair_site[k] == is) g.pairbuf[sm * g.nslots + k] = c;
  }
}

struct ComStatArgs {
  int ny, nw, S, i_lo, rows, nq;
  double probs[SUM_NQ_MAX];
  const double* slab;  // S x nw x rows
  int* n;              // ny x nw
  double* mean;        // ny x nw
  double* quant;       // nq x ny x nw
};

template <int NQ>
__global__ __launch_bounds__(256) void community_stat_kernel(ComStatArgs a) {
  const size_t cells = (size_t)a.nw * a.rows;
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const int m = (int)(c / a.rows), i = a.i_lo + (int)(c % a.rows);
  const size_t out = (size_t)i + (size_t)a.ny * m, plane = (size_t)a.ny * a.nw;
  const double* x = a.slab + c;
  int n = 0;
  double sum = 0.0;
  for (int s = 0; s < a.S; ++s) {
    const double v = x[(size_t)s * cells];
    if (v == v) sum += v, n += 1;
  }
  a.n[out] = n;
  a.mean[out] = sum / (double)n;  // 0 / 0 = NaN when every sample is NaN
  if (a.nq == 0) return;
  if (n == 0) {
    for (int q = 0; q < a.nq; ++q) a.quant[q * plane + out] = NAN;
    return;
  }
  select_quantiles<NQ>(x, cells, a.S, n, a.probs, a.nq, a.quant + out, plane);
}

static int com_nw_pad(int nw) { return nw <= 1 ? 1 : nw <= 4 ? 4 : nw <= 8 ? 8 : 16; }
static int com_work_doubles(int K, int NW) {
  return (int)std::max((size_t)PT_I * (K | 1) + (size_t)K * PT_J, (size_t)(NW + 1) * 4 * PT_I);
}

static void launch_community_kernel(hipStream_t st, const ComArgs& g, int NW, size_t S) {
  const size_t lds = ((size_t)g.work + (size_t)NW * PT_J) * sizeof(double);
  const unsigned ga = (unsigned)((size_t)g.ntile * S);
  if (NW == 1) predict_community_kernel<1><<<ga, 256, lds, st>>>(g);
  else if (NW == 4) predict_community_kernel<4><<<ga, 256, lds, st>>>(g);
  else if (NW == 8) predict_community_kernel<8><<<ga, 256, lds, st>>>(g);
  else predict_community_kernel<16><<<ga, 256, lds, st>>>(g);
  HIP_OK(hipGetLastError());
}

static void launch_stat_kernel(hipStream_t st, const ComStatArgs& qa, size_t cells) {
  const unsigned gq = (unsigned)((cells + 255) / 256);
  if (qa.nq <= 1) community_stat_kernel<1><<<gq, 256, 0, st>>>(qa);
  else if (qa.nq <= 2) community_stat_kernel<2><<<gq, 256, 0, st>>>(qa);
  else if (qa.nq <= 4) community_stat_kernel<4><<<gq, 256, 0, st>>>(qa);
  else community_stat_kernel<8><<<gq, 256, 0, st>>>(qa);
  HIP_OK(hipGetLastError());
}

// one slab of a map (predict_cell.h): the launch's own rows 0 .. a.ny - 1 are the slab
void community_launch_slab(hipStream_t st, const PredArgs& a, const MapCommunity& m) {
  ComArgs g{};
  g.p = a;
  g.i_lo = 0, g.rows = a.ny, g.ntile = (a.ny + PT_I - 1) / PT_I;
  g.nw = m.nw, g.transform = m.transform, g.nslots = 0;
  const int NW = com_nw_pad(m.nw);
  g.work = com_work_doubles(a.K, NW);
  for (int k = 0; k < m.nw; ++k) g.normalise[k] = m.normalise[k];
  g.W = m.W, g.slab = m.slab, g.comm = nullptr, g.pairbuf = nullptr;
  HMSC_REQUIRE((uint64_t)g.ntile * (uint64_t)a.nsamples <= COM_BLOCKS_MAX,
               "predict_map: a slab's 64-row tiles times the samples must not exceed 2^23");
  launch_community_kernel(st, g, NW, (size_t)a.nsamples);
}

void community_launch_stats(hipStream_t st, const PredArgs& a, const MapCommunity& m) {
  ComStatArgs qa{};
  qa.ny = a.nyTotal, qa.nw = m.nw, qa.S = a.nsamples, qa.i_lo = a.row0, qa.rows = a.ny, qa.nq = m.nq;
  for (int k = 0; k < m.nq; ++k) qa.probs[k] = m.probs[k];
  qa.slab = m.slab, qa.n = m.n, qa.mean = m.mean, qa.quant = m.quant;
  launch_stat_kernel(st, qa, (size_t)m.nw * a.ny);
}

static thread_local double g_community_ms[3] = {0.0, 0.0, 0.0};
void community_last_timing(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_community_ms[k];
}

static double com_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}


// host side: upload, then per slab of site tiles kernel A and the statistics kernel; the pairs
// are counted here from the pair buffer (called by hmsc_predict_community in capi.cpp)
void run_predict_community(const hmsc_predict_args* p, const hmsc_community_args* c, int32_t* n, double* mean,
                           double* quant, double* pr, double* comm) {
  const int K = check_pred_limits(p);
  HMSC_REQUIRE(p->ny > 0 && p->ns > 0, "predict_community: ny and ns must be positive");
  HMSC_REQUIRE(p->nsamples >= 1, "predict_community: nsamples must be at least 1");
  const int nw = c->nw, nq = c->nq, npairs = c->npairs;
  HMSC_REQUIRE(nw >= 1 && nw <= COM_NW_MAX,
               "predict_community: nw must lie in 1 .. 16 (nw = " + std::to_string(nw) + ")");
  HMSC_REQUIRE(c->W != nullptr && c->normalise != nullptr, "predict_community: W and normalise must not be NULL");
  HMSC_REQUIRE(nq >= 0 && nq <= SUM_NQ_MAX,
               "predict_community: at most 8 probabilities (nq = " + std::to_string(nq) + ")");
  HMSC_REQUIRE(nq == 0 || (c->probs != nullptr && quant != nullptr), "predict_community: nq > 0 needs probs and quant");
  HMSC_REQUIRE(npairs >= 0 && npairs <= COM_NPAIR_MAX,
               "predict_community: at most 8 site pairs (npairs = " + std::to_string(npairs) + ")");
  HMSC_REQUIRE(npairs == 0 || (c->pairs != nullptr && pr != nullptr), "predict_community: npairs > 0 needs pairs and pr");
  ComStatArgs qa{};
  for (int k = 0; k < nq; ++k) {
    HMSC_REQUIRE(c->probs[k] >= 0.0 && c->probs[k] <= 1.0, "predict_community: every probability must lie in [0, 1]");
    qa.probs[k] = c->probs[k];
  }
  ComArgs g{};
  for (int k = 0; k < 2 * npairs; ++k) {
    HMSC_REQUIRE(c->pairs[k] >= 0 && c->pairs[k] < p->ny,
                 "predict_community: pair index " + std::to_string(c->pairs[k]) + " outside 0 .. ny - 1");
    g.pair_site[k] = c->pairs[k];
  }
  for (int m = 0; m < nw; ++m) g.normalise[m] = c->normalise[m] ? 1 : 0;
  const size_t S = p->nsamples, ny = p->ny, ns = p->ns;
  const size_t ntiles = (ny + PT_I - 1) / PT_I;
  const uint64_t budget = c->scratch_bytes ? c->scratch_bytes : COM_SCRATCH_DEFAULT;
  const uint64_t tile_bytes = (uint64_t)S * PT_I * nw * 8;
  HMSC_REQUIRE(tile_bytes <= budget, "predict_community: one 64-row tile of the community columns needs " +
                                         std::to_string(tile_bytes) + " bytes of scratch, scratch_bytes allows " +
                                         std::to_string(budget));
  HMSC_REQUIRE(S <= COM_BLOCKS_MAX, "predict_community: at most 2^23 samples in one call");
  const size_t slab_tiles = std::min<uint64_t>(std::min<uint64_t>(ntiles, budget / tile_bytes), COM_BLOCKS_MAX / S);
  const size_t slab_rows = std::min(ny, slab_tiles * PT_I);
  const int NW = com_nw_pad(nw);

  DeviceGuard dg(p->device);
  std::vector<int> pi0;  // (source of a copy on the stream: before its owner)
  std::vector<double> hpairs;
  DeviceOwner own;
  const hipStream_t st = own.stream();
  auto t0 = std::chrono::steady_clock::now();
  g.p = upload_pred_args(p, own, st, pi0);
  g.nw = nw, g.transform = c->transform ? 1 : 0, g.nslots = 2 * npairs;
  g.work = com_work_doubles(K, NW);
  g.W = own.upload(c->W, ns * nw, st);
  g.slab = own.alloc<double>(S * nw * slab_rows);
  g.comm = comm ? own.alloc<double>(S * ny * nw) : nullptr;
  g.pairbuf = own.alloc<double>(S * nw * 2 * npairs);
  qa.ny = p->ny, qa.nw = nw, qa.S = p->nsamples, qa.nq = nq;
  qa.slab = g.slab;
  qa.n = own.alloc<int>(ny * nw);
  qa.mean = own.alloc<double>(ny * nw);
  qa.quant = nq > 0 ? own.alloc<double>((size_t)nq * ny * nw) : nullptr;
  HIP_OK(hipStreamSynchronize(st));
  double up_ms = com_ms_since(t0), a_ms = 0.0, q_ms = 0.0;
  for (size_t i_lo = 0; i_lo < ny; i_lo += slab_rows) {
    const size_t rows = std::min(slab_rows, ny - i_lo);
    t0 = std::chrono::steady_clock::now();
    g.i_lo = (int)i_lo, g.rows = (int)rows, g.ntile = (int)((rows + PT_I - 1) / PT_I);
    launch_community_kernel(st, g, NW, S);
    HIP_OK(hipStreamSynchronize(st));
    a_ms += com_ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    qa.i_lo = (int)i_lo, qa.rows = (int)rows;
    launch_stat_kernel(st, qa, (size_t)nw * rows);
    HIP_OK(hipStreamSynchronize(st));
    q_ms += com_ms_since(t0);
  }
  t0 = std::chrono::steady_clock::now();
  HIP_OK(hipMemcpyAsync(n, qa.n, ny * nw * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(mean, qa.mean, ny * nw * 8, hipMemcpyDeviceToHost, st));
  if (nq > 0) HIP_OK(hipMemcpyAsync(quant, qa.quant, (size_t)nq * ny * nw * 8, hipMemcpyDeviceToHost, st));
  if (comm) HIP_OK(hipMemcpyAsync(comm, g.comm, S * ny * nw * 8, hipMemcpyDeviceToHost, st));
  if (npairs > 0) {
    hpairs.resize(S * nw * 2 * npairs);
    HIP_OK(hipMemcpyAsync(hpairs.data(), g.pairbuf, hpairs.size() * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  // Pr[C[, b, m] > C[, a, m]]: NaN when either value is NaN in any sample (R's mean of a logical with NA)
  for (int k = 0; k < npairs; ++k)
    for (int m = 0; m < nw; ++m) {
      size_t above = 0;
      bool nan = false;
      for (size_t s = 0; s < S; ++s) {
        const double* row = hpairs.data() + (s * nw + m) * 2 * npairs;
        const double va = row[2 * k], vb = row[2 * k + 1];
        nan = nan || va != va || vb != vb;
        above += vb > va ? 1 : 0;
      }
      pr[k + (size_t)npairs * m] = nan ? NAN : (double)above / (double)S;
    }
  q_ms += com_ms_since(t0);
  g_community_ms[0] = up_ms, g_community_ms[1] = a_ms, g_community_ms[2] = q_ms;
}

}  // namespace hmsc
