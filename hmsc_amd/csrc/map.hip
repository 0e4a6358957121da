// Prediction maps (hmsc_predict_map in include/hmsc_amd.h): a pooled posterior mapped onto ny new
// rows, slab of rows by slab, the latent factors of a slab's units made and used on the device.
//
// Once per call: the uploads (X, Beta, sigma, the levels' posterior Eta, Lambda, geometry), the
// slab plan (host: per slab and level the distinct units in ascending order and the slab-local Pi)
// and per level the kriging plan (a resident KrigeLevel of krige_level.h; krige_plan_group: per grid
// value a > 0 in use K11, its factor, Y = L^-1 E).
// Per slab:
//   map_assemble_kernel   the level's Eta table T (S x units x nf, PredArgs::Eta's layout): a fitted
//                         unit's posterior rows; a new unit's z where the pair's grid value is 0
//                         (0 with predictMean), else 0 for the kriging to overwrite
//   krige_slab_group      per grid value a > 0: the K12 slab, B = L^-1 K12, the mean product written
//                         straight into T's new units (modes 0, 1); krige_launch_nn (mode 3);
//                         krige_launch_group ('Full': all new units in the slab); gpp_slab_group
//                         (mode 4: dDn and Wns C + sqrt(dDn) z from the resident iWss and C, any slab)
//   launch_values / launch_statistics (slab_engine.h) of the cell block and of each community block
//                         on a PredArgs of the slab's rows: cell = (row0 + i) + ny j, the outputs
//                         written into the whole-map buffers at row0; Pi is the slab's local table
//                         (ldPi = the slab's rows), np the slab's units
// The block descriptors, their checks, the slab sizing, the outputs' allocation and the copy back
// are the engine's; the pair grouping, the mode checks, the kriging's workspaces, launches and reports
// are the KrigeLevel's, the one hmsc_krige drives too; this file keeps the slabs' units and local Pi,
// the device-memory budget, the Eta tables and its nine phases.
// A value of T depends on (unit, factor, sample) alone: z by its counters, the kriging by sums over
// the fitted units in index order whatever slab and tile the unit falls in.  So a unit that several
// slabs refer to is the same double in each, and the outputs are those of hmsc_krige followed by
// hmsc_predict_summary / hmsc_predict_community for every slab size.
#include <algorithm>
#include <string>
#include <vector>

#include "krige_level.h"
#include "slab_engine.h"
#include "state.h"

namespace hmsc {

namespace {

constexpr int MAP_PHASES = 9;
enum MapPhase { PH_PLAN, PH_K12, PH_TRSM, PH_MEAN, PH_ASM, PH_SUM, PH_COM, PH_STAT, PH_COPY };

struct AsmArgs {
  const double* Eta;  // S x np x nf: the fitted units' posterior
  const int* units;   // U: the slab's units, 0-based; >= np: new unit units[u] - np
  const int* zflag;   // S x nf: 1 = a new unit's value is z (grid value 0, not predictMean)
  double* T;          // S x U x nf
  int U, np, nf, S;
  Key key;
  uint32_t stream;
};

__global__ __launch_bounds__(256) void map_assemble_kernel(AsmArgs a) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= a.U) return;
  const int unit = a.units[u];
  for (int p = blockIdx.y; p < a.S * a.nf; p += gridDim.y) {
    const int s = p / a.nf, h = p % a.nf;
    double v = 0.0;
    if (unit < a.np)
      v = a.Eta[(size_t)p * a.np + unit];
    else if (a.zflag[p])
      v = normal(a.key, (uint32_t)(unit - a.np), (uint32_t)h, a.stream, (uint32_t)s);
    a.T[(size_t)p * a.U + u] = v;
  }
}

// what the host keeps of a level: its kriging plan and the slab bookkeeping
struct LevelPlan {
  KrigeLevel k;
  bool full = false;                   // a 'Full' level with a grid value > 0 in use: the joint draw
  std::vector<size_t> off{0};          // per slab: its units' range in units
  std::vector<int> units, unew, nknown;  // the slabs' units; units - np; fitted units per slab
  size_t Umax = 0, mmax = 0;           // most units / new units of a slab
  // device
  const int* d_units = nullptr;
  const int* d_unew = nullptr;
  const int* d_zflag = nullptr;
  double* T = nullptr;
};

}  // namespace

static thread_local double g_map_ms[MAP_PHASES] = {0};
void map_last_timing(double out[MAP_PHASES]) {
  for (int k = 0; k < MAP_PHASES; ++k) out[k] = g_map_ms[k];
}

void run_predict_map(const hmsc_map_args* p, const hmsc_map_out* o) {
  HMSC_REQUIRE(p->nr >= 0 && p->nr <= HMSC_MAX_LEVELS, "predict_map: bad nr");
  HMSC_REQUIRE(p->ny > 0 && p->ns > 0, "predict_map: ny and ns must be positive");
  HMSC_REQUIRE(p->nsamples >= 1, "predict_map: nsamples must be at least 1");
  HMSC_REQUIRE(p->X != nullptr && p->Beta != nullptr && p->sigma != nullptr && p->family != nullptr &&
                   p->YScalePar != nullptr,
               "predict_map: NULL X / Beta / sigma / family / YScalePar");
  const int nr = p->nr;
  int K = p->nc;
  for (int r = 0; r < nr; ++r) {
    HMSC_REQUIRE(p->level[r].nf > 0 && p->level[r].np > 0 && p->level[r].nn >= 0,
                 "predict_map: a level's np and nf must be positive");
    K += p->level[r].nf;
  }
  HMSC_REQUIRE(K <= PK_MAX, "predict_map: nc + sum(nf) must be <= 128");
  HMSC_REQUIRE((size_t)p->ny * p->ns < ((size_t)1 << 32),
               "predict_map: nyTotal * ns must fit 32-bit cell counters (ny = " + std::to_string(p->ny) +
                   ", ns = " + std::to_string(p->ns) + ")");
  const size_t S = p->nsamples, ny = p->ny, ns = p->ns, nc = p->nc;
  HMSC_REQUIRE(S <= BLOCKS_MAX, "predict_map: at most 2^23 samples in one call");
  HMSC_REQUIRE(p->cells || p->ncomm > 0, "predict_map: neither cells nor a community block is asked for");
  HMSC_REQUIRE(p->ncomm >= 0 && p->ncomm <= 2, "predict_map: ncomm must be 0, 1 or 2");

  // the blocks
  CellBlock ms{};
  std::vector<int> slot, cols;
  if (p->cells) {
    HMSC_REQUIRE(o->mean != nullptr && o->occ != nullptr && o->n != nullptr, "predict_map: cells needs mean, occ and n");
    check_cells("predict_map", &p->summary, ns, o->quant, ms, slot, cols);
  }
  const size_t nslot = ms.nslot, nq = ms.nq;
  CommunityBlock mc[2] = {};
  size_t nw_all = 0;
  for (int b = 0; b < p->ncomm; ++b) {
    check_community("predict_map", &p->community[b], p->ny, true, o->cn[b], o->cmean[b], o->cquant[b], nullptr, mc[b]);
    nw_all += mc[b].nw;
  }

  // the slabs: every block's slab columns and the levels' Eta tables against the scratch budget
  size_t nf_all = 0;
  for (int r = 0; r < nr; ++r) nf_all += p->level[r].nf;
  const size_t slab_rows = plan_slab_rows("predict_map", "", ny, S, nslot + nw_all + nf_all,
                                          p->slab_rows > 0 ? (size_t)p->slab_rows : 0, p->scratch_bytes, true);
  const size_t nslab = (ny + slab_rows - 1) / slab_rows;

  // per level: the kriging plan's (s, h) pairs by grid value, the slabs' units and local Pi
  std::vector<LevelPlan> lv(nr);
  std::vector<int> piloc(ny * std::max(1, nr), 0);  // slab after slab, each rows x nr column-major
  std::vector<int> pos;
  for (int r = 0; r < nr; ++r) {
    const hmsc_map_level& l = p->level[r];
    LevelPlan& P = lv[r];
    const std::string nm = "predict_map: level " + std::to_string(r) + ": ";
    HMSC_REQUIRE(l.unit != nullptr && l.Eta != nullptr && l.Lambda != nullptr && l.alphas != nullptr &&
                     l.alpha != nullptr && l.G > 0,
                 nm + "NULL unit / Eta / Lambda / alphas / alpha, or G = 0");
    HMSC_REQUIRE(l.mode >= 0 && l.mode <= 4,
                 nm + "mode must be 0 (predictMean), 1 (predictMeanField), 2 (Full), 3 (NNGP) or 4 (GPP)");
    HMSC_REQUIRE(l.coords == nullptr || l.sDim > 0, nm + "coords needs sDim > 0");
    P.k.q = KrigeSpec{l.mode, l.np, l.nn, l.sDim, l.nK, l.nNeighbours, l.G, p->nsamples, l.nf, r,
                      l.coords, l.dist, l.knots, l.alphas, l.Eta, l.alpha, p->seed};
    P.k.g = krige_group_pairs(P.k.q, false, nm);
    if (P.k.g.size() > 0) krige_check_mode(P.k.q, nm);
    P.full = l.mode == 2 && P.k.g.cmax > 0;
    // slabs
    const int Nu = l.np + l.nn;
    pos.assign(Nu, -1);
    size_t base = 0;
    for (size_t b = 0; b < nslab; ++b) {
      const size_t row0 = b * slab_rows, m = std::min(slab_rows, ny - row0);
      const size_t u0 = P.units.size();
      for (size_t i = 0; i < m; ++i) {
        const int u = l.unit[row0 + i] - 1;
        HMSC_REQUIRE(u >= 0 && u < Nu, nm + "unit " + std::to_string(u + 1) + " of row " + std::to_string(row0 + i) +
                                           " is outside 1 .. np + nn");
        P.units.push_back(u);
      }
      std::sort(P.units.begin() + u0, P.units.end());
      P.units.erase(std::unique(P.units.begin() + u0, P.units.end()), P.units.end());
      const size_t U = P.units.size() - u0;
      size_t known = 0;
      for (size_t k = 0; k < U; ++k) pos[P.units[u0 + k]] = (int)k, known += P.units[u0 + k] < l.np ? 1 : 0;
      for (size_t i = 0; i < m; ++i) piloc[base + i + m * r] = pos[l.unit[row0 + i] - 1];
      P.off.push_back(P.units.size());
      P.nknown.push_back((int)known);
      P.Umax = std::max(P.Umax, U), P.mmax = std::max(P.mmax, U - known);
      HMSC_REQUIRE(!P.full || U == known || U - known == (size_t)l.nn,
                   nm + "a 'Full' joint draw needs all " + std::to_string(l.nn) + " new units in one slab (slab " +
                       std::to_string(b) + " of " + std::to_string(slab_rows) + " rows holds " + std::to_string(U - known) +
                       "); use predictEtaMean or predictEtaMeanField");
      base += m * (size_t)std::max(1, nr);
    }
    P.unew = P.units;
    for (int& u : P.unew) u -= l.np;
  }

  // device memory: the kriging's share against its budget
  DeviceGuard dg(p->device);
  uint64_t fixed = (ny * nc + S * nc * ns + S * ns + 2 * ns) * 8 + ns * 4 + piloc.size() * 4;  // X, Beta, sigma, ...
  fixed += (uint64_t)slab_rows * S * 8 * (nslot + nw_all);
  if (p->cells) fixed += ny * ns * (8 + 8 + 4) + (uint64_t)nq * ny * ns * 8;
  for (int b = 0; b < p->ncomm; ++b) fixed += ny * mc[b].nw * (uint64_t)(12 + 8 * mc[b].nq) + ns * mc[b].nw * 8;
  uint64_t need = 0;
  for (int r = 0; r < nr; ++r) {
    const hmsc_map_level& l = p->level[r];
    const LevelPlan& P = lv[r];
    const uint64_t nf = l.nf;
    need += krige_need_bytes(P.k.q, P.k.g, true, P.mmax);
    need += (S * nf * ns + S * P.Umax * nf) * 8 + (2 * P.units.size() + S * nf) * 4;  // Lambda, the table; the units, zflag
  }
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t budget = p->factor_bytes ? p->factor_bytes : (free_b > fixed ? free_b - fixed : 0);
  HMSC_REQUIRE(need <= budget, "predict_map: the kriging plan (resident factors, Y, posterior Eta) and one slab's workspace "
                                   "need " + std::to_string(need) + " bytes of device memory, the budget (factor_bytes) is " +
                                   std::to_string(budget) + " bytes");

  DeviceOwner own;
  const hipStream_t st = own.stream();
  double ph[MAP_PHASES] = {0};
  auto t0 = std::chrono::steady_clock::now();
  auto up = [&](const auto* src, size_t n) { return own.upload(src, n, st); };
  PredArgs a{};
  a.ns = p->ns, a.nc = p->nc, a.nr = nr, a.nsamples = p->nsamples, a.K = K, a.expected = p->expected;
  a.nyTotal = p->ny;
  a.X = up(p->X, ny * nc);
  a.Beta = up(p->Beta, S * nc * ns);
  a.sigma = up(p->sigma, S * ns);
  a.family = up(p->family, ns);
  a.yscale = up(p->YScalePar, 2 * ns);
  a.key = Key{(uint32_t)p->seed, (uint32_t)(p->seed >> 32)};
  const int* d_piloc = up(piloc.data(), piloc.size());
  if (p->cells) alloc(own, st, a, slab_rows, slot, cols, ms);
  for (int b = 0; b < p->ncomm; ++b) alloc(own, st, a, slab_rows, p->community[b].W, false, mc[b]);
  for (int r = 0; r < nr; ++r) {
    const hmsc_map_level& l = p->level[r];
    LevelPlan& P = lv[r];
    const size_t nf = l.nf;
    a.nf[r] = l.nf;
    a.Lambda[r] = up(l.Lambda, S * nf * ns);
    P.d_units = up(P.units.data(), P.units.size());
    P.d_unew = up(P.unew.data(), P.unew.size());
    P.d_zflag = up(P.k.g.zflag.data(), P.k.g.zflag.size());
    P.T = own.alloc<double>(S * P.Umax * nf);
    a.Eta[r] = P.T;
    P.k.prepare(own, st, true, P.mmax, true);
  }
  HIP_OK(hipStreamSynchronize(st));
  ph[PH_PLAN] = ms_since(t0);

  size_t base = 0;
  for (size_t b = 0; b < nslab; ++b) {
    const size_t row0 = b * slab_rows, m = std::min(slab_rows, ny - row0);
    a.ny = a.ldPi = (int)m, a.row0 = (int)row0;
    a.Pi = d_piloc + base;
    base += m * (size_t)std::max(1, nr);
    // the Eta tables
    timed(st, ph[PH_ASM], [&] {
      for (int r = 0; r < nr; ++r) {
        const LevelPlan& P = lv[r];
        const int U = (int)(P.off[b + 1] - P.off[b]);
        a.np[r] = U;
        const KrigeDev& d = P.k.dev();
        AsmArgs g{d.Eta, P.d_units + P.off[b], P.d_zflag, P.T, U, d.np, d.nfmax, (int)S, a.key, d.stream};
        const unsigned gy = (unsigned)std::min<size_t>(S * d.nfmax, 65535);
        map_assemble_kernel<<<dim3((unsigned)((U + 255) / 256), gy), 256, 0, st>>>(g);
        HIP_OK(hipGetLastError());
      }
    });
    // the kriging of the slab's new units
    std::vector<int> ran;
    for (int r = 0; r < nr; ++r) {
      LevelPlan& P = lv[r];
      const int U = (int)(P.off[b + 1] - P.off[b]), known = P.nknown[b];
      if (P.k.run(st, P.d_unew + P.off[b] + known, U - known, P.T + known, (size_t)U)) ran.push_back(r);
    }
    if (!ran.empty()) HIP_OK(hipStreamSynchronize(st));
    for (int r : ran)  // 'GPP': the dDn pass, then the slab product
      lv[r].k.each_elapsed([&](int grp, int w, double e) {
        ph[grp < 0 || (p->level[r].mode == 4 && w == 1) ? PH_MEAN : PH_K12 + w] += e;
      });
    // the summaries of the slab's rows
    if (p->cells) timed(st, ph[PH_SUM], [&] { launch_values(st, a, ms); });
    for (int c = 0; c < p->ncomm; ++c) timed(st, ph[PH_COM], [&] { launch_values(st, a, mc[c]); });
    timed(st, ph[PH_STAT], [&] {
      if (p->cells) launch_statistics(st, a, ms);
      for (int c = 0; c < p->ncomm; ++c) launch_statistics(st, a, mc[c]);
    });
  }

  t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < nr; ++r) lv[r].k.collect(st);
  if (p->cells) copy_out(st, a, ms, o->mean, o->occ, o->n, o->quant);
  for (int b = 0; b < p->ncomm; ++b) copy_out(st, a, mc[b], o->cn[b], o->cmean[b], o->cquant[b]);
  HIP_OK(hipStreamSynchronize(st));
  ph[PH_COPY] = ms_since(t0);
  for (int k = 0; k < MAP_PHASES; ++k) g_map_ms[k] = ph[k];
  for (int r = 0; r < nr; ++r) lv[r].k.report("predict_map: level " + std::to_string(r) + ": ");
}

}  // namespace hmsc
