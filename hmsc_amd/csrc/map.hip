// Prediction maps (hmsc_predict_map in include/hmsc_amd.h): a pooled posterior mapped onto ny new
// rows, slab of rows by slab, the latent factors of a slab's units made and used on the device.
//
// Once per call: the uploads (X, Beta, sigma, the levels' posterior Eta, Lambda, geometry), the
// slab plan (host: per slab and level the distinct units in ascending order and the slab-local Pi)
// and the kriging plan (krige_plan_group: per grid value a > 0 in use K11, its factor, Y = L^-1 E).
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
// are the engine's; this file keeps the level plan, the device-memory budget, the Eta tables and
// its nine phases.
// A value of T depends on (unit, factor, sample) alone: z by its counters, the kriging by sums over
// the fitted units in index order whatever slab and tile the unit falls in.  So a unit that several
// slabs refer to is the same double in each, and the outputs are those of hmsc_krige followed by
// hmsc_predict_summary / hmsc_predict_community for every slab size.
#include <algorithm>
#include <string>
#include <vector>

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

// what the host keeps of a level
struct LevelPlan {
  bool spatial = false, dense = false, full = false, gpp = false;
  int ipg = 2;                         // info words per group (4: 'GPP')
  std::vector<int> col_s, col_h, g_idx, g_off{0};
  std::vector<double> g_alpha;
  std::vector<int> zflag;
  size_t cmax = 0;                     // most pairs of a grid value > 0
  std::vector<size_t> off{0};          // per slab: its units' range in units
  std::vector<int> units, unew, nknown;  // the slabs' units; units - np; fitted units per slab
  size_t Umax = 0, mmax = 0;           // most units / new units of a slab
  // device
  KrigeDev d{};
  const int* d_units = nullptr;
  const int* d_unew = nullptr;
  const int* d_zflag = nullptr;
  const double* d_galpha = nullptr;
  const int* d_goff = nullptr;
  double* T = nullptr;
  std::vector<double*> K11, ws, Y;     // per group (null at a = 0)
  std::vector<double*> iWss, Cm;       // 'GPP', per group (null at a = 0)
  int* info = nullptr;                 // 2 per group, then the NNGP kernel's
  std::vector<hipEvent_t> ev;          // 4 per group (modes 0, 1), 2 otherwise
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

  // per level: the (s, h) pairs by grid value (hmsc_krige's grouping), the slabs' units and local Pi
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
    P.spatial = l.coords != nullptr || l.dist != nullptr;
    HMSC_REQUIRE(l.coords == nullptr || l.sDim > 0, nm + "coords needs sDim > 0");
    const size_t nf = l.nf;
    std::vector<std::vector<int>> by_g(l.G + 1);
    P.zflag.assign(S * nf, 0);
    for (size_t s = 0; s < S; ++s) {
      int glast = 0;
      for (size_t h = 0; h < nf; ++h) {
        const int g = l.alpha[s * nf + h];
        HMSC_REQUIRE(g >= 0 && g <= l.G, nm + "grid index " + std::to_string(g) + " of sample " + std::to_string(s) +
                                             ", factor " + std::to_string(h) + " is outside the alphapw grid 1.." +
                                             std::to_string(l.G));
        if (g > 0) glast = g;
      }
      for (size_t h = 0; h < nf; ++h) {  // 'GPP': the sample's last factor decides for all (R's ag = alpha[nf])
        const int g = l.alpha[s * nf + h] > 0 ? (l.mode == 4 ? glast : l.alpha[s * nf + h]) : 0;
        if (g > 0) by_g[g].push_back((int)(s * nf + h));
        if (g > 0 && !(l.alphas[g - 1] > 0.0) && l.mode != 0) P.zflag[s * nf + h] = 1;
      }
    }
    for (int g = 1; g <= l.G; ++g) {
      if (by_g[g].empty()) continue;
      const bool pos_a = l.alphas[g - 1] > 0.0;
      if (!pos_a && l.mode != 3) continue;  // z: the assembly's
      HMSC_REQUIRE(!pos_a || P.spatial, nm + "a grid value > 0 needs coords or dist");
      for (int pr : by_g[g]) P.col_s.push_back(pr / (int)nf), P.col_h.push_back(pr % (int)nf);
      P.g_idx.push_back(g);
      P.g_alpha.push_back(l.alphas[g - 1]);
      P.g_off.push_back((int)P.col_s.size());
      if (pos_a) P.cmax = std::max(P.cmax, by_g[g].size());
    }
    if (l.nn == 0) P.g_idx.clear(), P.g_alpha.clear(), P.g_off.assign(1, 0), P.col_s.clear(), P.col_h.clear(), P.cmax = 0;
    if (l.mode == 3) {
      for (size_t k = 0; k < P.zflag.size(); ++k) P.zflag[k] = 0;  // the NNGP kernel writes z itself
      if (!P.g_idx.empty()) {
        HMSC_REQUIRE(l.coords != nullptr, nm + "NNGP kriging needs coordinates; a distMat level predicts with 'Full'");
        HMSC_REQUIRE(l.nNeighbours >= 1, nm + "nNeighbours must be positive");
        HMSC_REQUIRE(l.nNeighbours <= 32, nm + "NNGP kriging on the device takes nNeighbours <= 32 (got " +
                                              std::to_string(l.nNeighbours) + ")");
        HMSC_REQUIRE(l.nNeighbours <= l.np, nm + "nNeighbours exceeds the number of fitted units");
      }
    }
    if (l.mode == 4 && P.cmax > 0) {
      HMSC_REQUIRE(l.coords != nullptr && l.dist == nullptr,
                   nm + "GPP kriging needs coordinates; a distMat level predicts with 'Full'");
      HMSC_REQUIRE(l.knots != nullptr && l.nK > 0, nm + "GPP kriging needs knots (knots with nK > 0)");
      P.gpp = true, P.ipg = 4;
    }
    P.dense = l.mode != 3 && l.mode != 4 && P.cmax > 0;
    P.full = P.dense && l.mode == 2;
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
    const uint64_t np = l.np, N = np + l.nn, nf = l.nf;
    uint64_t dbl = S * np * nf + S * nf * ns + S * P.Umax * nf;  // Eta, Lambda, the table
    if (!P.g_idx.empty()) dbl += l.coords ? N * l.sDim : N * N;
    if (P.dense && !P.full) {
      uint64_t ngpos = 0, cs = 0;
      for (size_t k = 0; k < P.g_idx.size(); ++k)
        if (P.g_alpha[k] > 0.0) ++ngpos, cs += P.g_off[k + 1] - P.g_off[k];
      dbl += ngpos * (np * np + dense_ws_doubles(l.np)) + np * cs;  // the resident factors and Y
      dbl += np * P.mmax + P.mmax;                                  // one slab: K12, v
    }
    if (P.gpp) {
      const uint64_t nK = l.nK;
      dbl += nK * l.sDim + gpp_plan_doubles(l.np, l.nK, (int)P.cmax) + P.mmax;  // the plan's workspace; one slab: dDn
      for (size_t k = 0; k < P.g_idx.size(); ++k)
        if (P.g_alpha[k] > 0.0) dbl += nK * nK + nK * (uint64_t)(P.g_off[k + 1] - P.g_off[k]);  // resident: iWss, C
    }
    if (P.full) {
      const uint64_t nn = l.nn;
      dbl += np * np + np * (nn + P.cmax) + dense_ws_doubles(l.np) + nn * nn + nn * P.cmax + dense_ws_doubles(l.nn);
    }
    need += dbl * 8 + (2 * P.units.size() + 2 * P.col_s.size() + S * nf + 6 * P.g_idx.size() + 2 + DENSE_SYNC_INTS) * 4;
  }
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t budget = p->factor_bytes ? p->factor_bytes : (free_b > fixed ? free_b - fixed : 0);
  HMSC_REQUIRE(need <= budget, "predict_map: the kriging plan (resident factors, Y, posterior Eta) and one slab's workspace "
                                   "need " + std::to_string(need) + " bytes of device memory, the budget (factor_bytes) is " +
                                   std::to_string(budget) + " bytes");

  std::vector<std::vector<int>> infos(nr);  // (host targets of the stream's copies: before the stream)
  std::vector<int> hs(nr, 0);
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
    const size_t np = l.np, N = np + l.nn, nf = l.nf, ng = P.g_idx.size();
    a.nf[r] = l.nf;
    a.Lambda[r] = up(l.Lambda, S * nf * ns);
    KrigeDev& d = P.d;
    d.np = l.np, d.sdim = l.coords ? l.sDim : 0, d.S = p->nsamples, d.nfmax = l.nf, d.N = (int)N;
    d.seed = p->seed;
    d.stream = S_KRIGE + LEVEL_STRIDE * (uint32_t)r;
    d.Eta = up(l.Eta, S * np * nf);
    P.d_units = up(P.units.data(), P.units.size());
    P.d_unew = up(P.unew.data(), P.unew.size());
    P.d_zflag = up(P.zflag.data(), P.zflag.size());
    P.T = own.alloc<double>(S * P.Umax * nf);
    a.Eta[r] = P.T;
    infos[r].assign(P.ipg * ng + 1, 0);
    P.info = own.alloc<int>(P.ipg * ng + 1);
    if (ng == 0) continue;
    double* geo = l.coords ? up(l.coords, N * l.sDim) : up(l.dist, N * N);
    d.coords = l.coords ? geo : nullptr;
    d.dist = l.coords ? nullptr : geo;
    d.col_s = up(P.col_s.data(), P.col_s.size());
    d.col_h = up(P.col_h.data(), P.col_h.size());
    if (l.mode == 3) {
      P.d_galpha = up(P.g_alpha.data(), ng);
      P.d_goff = up(P.g_off.data(), ng + 1);
      P.ev = {own.event(), own.event()};
      continue;
    }
    d.sync = own.alloc<int>(DENSE_SYNC_INTS);
    if (l.mode == 4) {
      for (size_t k = 0; k < 4 * ng; ++k) P.ev.push_back(own.event());
      if (!P.gpp) continue;
      const size_t nK = l.nK;
      d.knots = up(l.knots, nK * l.sDim);
      d.nK = l.nK;
      d.v = own.alloc<double>(P.mmax);
      const GppWork gw = gpp_carve(own.alloc<double>(gpp_plan_doubles(l.np, l.nK, (int)P.cmax)), l.np, l.nK, (int)P.cmax);
      P.iWss.assign(ng, nullptr), P.Cm.assign(ng, nullptr);
      for (size_t k = 0; k < ng; ++k) {
        if (!(P.g_alpha[k] > 0.0)) continue;
        const int c = P.g_off[k + 1] - P.g_off[k];
        P.iWss[k] = own.alloc<double>(nK * nK);
        P.Cm[k] = own.alloc<double>(nK * (size_t)c);
        gpp_plan_group(st, d, gw, P.g_alpha[k], P.g_off[k], c, P.iWss[k], P.Cm[k], P.info + 4 * k, nullptr);
      }
      continue;
    }
    if (P.full) {
      const size_t nn = l.nn;
      d.K11 = own.alloc<double>(np * np);
      d.R = own.alloc<double>(np * (nn + P.cmax));
      d.ws1 = own.alloc<double>(dense_ws_doubles(l.np));
      d.W = own.alloc<double>(nn * nn);
      d.Z = own.alloc<double>(nn * P.cmax);
      d.ws2 = own.alloc<double>(dense_ws_doubles(l.nn));
      P.ev = {own.event(), own.event()};
      continue;
    }
    d.R = own.alloc<double>(np * P.mmax);
    if (l.mode == 1) d.v = own.alloc<double>(P.mmax);
    P.K11.assign(ng, nullptr), P.ws.assign(ng, nullptr), P.Y.assign(ng, nullptr);
    for (size_t k = 0; k < ng; ++k) {
      for (int e = 0; e < 4; ++e) P.ev.push_back(own.event());
      if (!(P.g_alpha[k] > 0.0)) continue;
      const int c = P.g_off[k + 1] - P.g_off[k];
      P.K11[k] = own.alloc<double>(np * np);
      P.ws[k] = own.alloc<double>(dense_ws_doubles(l.np));
      P.Y[k] = own.alloc<double>(np * (size_t)c);
      krige_plan_group(st, d, P.g_alpha[k], P.g_off[k], c, P.K11[k], P.ws[k], P.Y[k], P.info + 2 * k);
    }
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
        AsmArgs g{P.d.Eta, P.d_units + P.off[b], P.d_zflag, P.T, U, P.d.np, P.d.nfmax, (int)S, a.key, P.d.stream};
        const unsigned gy = (unsigned)std::min<size_t>(S * P.d.nfmax, 65535);
        map_assemble_kernel<<<dim3((unsigned)((U + 255) / 256), gy), 256, 0, st>>>(g);
        HIP_OK(hipGetLastError());
      }
    });
    // the kriging of the slab's new units
    bool kriged = false;
    for (int r = 0; r < nr; ++r) {
      const hmsc_map_level& l = p->level[r];
      LevelPlan& P = lv[r];
      const int U = (int)(P.off[b + 1] - P.off[b]), known = P.nknown[b], mnew = U - known;
      const int ng = (int)P.g_idx.size();
      if (mnew == 0 || ng == 0) continue;
      kriged = true;
      KrigeDev d = P.d;
      d.nn = mnew, d.unit = P.d_unew + P.off[b] + known, d.out = P.T + known, d.ldo = (size_t)U;
      if (l.mode == 3) {
        HIP_OK(hipEventRecord(P.ev[0], st));
        krige_launch_nn(st, d, l.nNeighbours, ng, P.d_galpha, P.d_goff, P.info + 2 * ng);
        HIP_OK(hipEventRecord(P.ev[1], st));
      } else if (P.full) {
        HIP_OK(hipEventRecord(P.ev[0], st));
        for (int k = 0; k < ng; ++k)
          krige_launch_group(st, d, 2, P.g_alpha[k], P.g_off[k], P.g_off[k + 1] - P.g_off[k], P.info + 2 * k, nullptr);
        HIP_OK(hipEventRecord(P.ev[1], st));
      } else if (l.mode == 4) {
        for (int k = 0; k < ng; ++k)
          if (P.g_alpha[k] > 0.0)
            gpp_slab_group(st, d, P.g_alpha[k], P.g_off[k], P.g_off[k + 1] - P.g_off[k], P.iWss[k], P.Cm[k],
                           P.ev.data() + 4 * k);
      } else {
        for (int k = 0; k < ng; ++k)
          if (P.g_alpha[k] > 0.0)
            krige_slab_group(st, d, l.mode, P.g_alpha[k], P.g_off[k], P.g_off[k + 1] - P.g_off[k], P.K11[k], P.ws[k],
                             P.Y[k], P.ev.data() + 4 * k);
      }
    }
    if (kriged) {
      HIP_OK(hipStreamSynchronize(st));
      for (int r = 0; r < nr; ++r) {
        const LevelPlan& P = lv[r];
        const int ng = (int)P.g_idx.size();
        if (P.off[b + 1] - P.off[b] == (size_t)P.nknown[b] || ng == 0) continue;
        float e = 0.f;
        if (p->level[r].mode == 3 || P.full) {
          HIP_OK(hipEventElapsedTime(&e, P.ev[0], P.ev[1]));
          ph[PH_MEAN] += e;
          continue;
        }
        for (int k = 0; k < ng; ++k) {
          if (!(P.g_alpha[k] > 0.0)) continue;
          for (int w = 0; w < (P.gpp ? 2 : 3); ++w) {  // 'GPP': the dDn pass, then the slab product
            HIP_OK(hipEventElapsedTime(&e, P.ev[4 * k + w], P.ev[4 * k + w + 1]));
            ph[P.gpp && w == 1 ? PH_MEAN : PH_K12 + w] += e;
          }
        }
      }
    }
    // the summaries of the slab's rows
    if (p->cells) timed(st, ph[PH_SUM], [&] { launch_values(st, a, ms); });
    for (int c = 0; c < p->ncomm; ++c) timed(st, ph[PH_COM], [&] { launch_values(st, a, mc[c]); });
    timed(st, ph[PH_STAT], [&] {
      if (p->cells) launch_statistics(st, a, ms);
      for (int c = 0; c < p->ncomm; ++c) launch_statistics(st, a, mc[c]);
    });
  }

  t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < nr; ++r) {
    HIP_OK(hipMemcpyAsync(infos[r].data(), lv[r].info, infos[r].size() * sizeof(int), hipMemcpyDeviceToHost, st));
    if (lv[r].d.sync)
      HIP_OK(hipMemcpyAsync(&hs[r], lv[r].d.sync + DENSE_SYNC_ERR, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (p->cells) copy_out(st, a, ms, o->mean, o->occ, o->n, o->quant);
  for (int b = 0; b < p->ncomm; ++b) copy_out(st, a, mc[b], o->cn[b], o->cmean[b], o->cquant[b]);
  HIP_OK(hipStreamSynchronize(st));
  ph[PH_COPY] = ms_since(t0);
  for (int k = 0; k < MAP_PHASES; ++k) g_map_ms[k] = ph[k];
  for (int r = 0; r < nr; ++r) {
    const LevelPlan& P = lv[r];
    const std::string nm = "predict_map: level " + std::to_string(r) + ": ";
    if (hs[r] != 0)
      throw HmscError(-5, "internal: an in-launch handshake of the blocked dense solver timed out (error bits " +
                              std::to_string(hs[r]) + "); the result is invalid");
    const size_t ng = P.g_idx.size();
    for (size_t k = 0; P.gpp && k < ng; ++k) {
      const std::string at = " at grid index " + std::to_string(P.g_idx[k]) + " (alpha = " + std::to_string(P.g_alpha[k]) + ")";
      HMSC_REQUIRE(infos[r][4 * k] == 0, nm + "GPP: Wss of the knots is not positive definite" + at);
      HMSC_REQUIRE(infos[r][4 * k + 3] == 0, nm + "GPP: fitted unit " + std::to_string(P.d.np - infos[r][4 * k + 3]) +
                                                 " (0-based) lies on a knot or has dD <= 0" + at +
                                                 ": its predictive-process variance 1 / dD is not finite");
      HMSC_REQUIRE(infos[r][4 * k + 1] == 0, nm + "GPP: F = Wss + W12' diag(1 / dD) W12 is not positive definite" + at);
      HMSC_REQUIRE(infos[r][4 * k + 2] == 0, nm + "GPP: iF = F^-1 is not positive definite" + at);
    }
    for (size_t k = 0; !P.gpp && k < ng; ++k) {
      HMSC_REQUIRE(infos[r][2 * k] == 0, nm + "K11 of the fitted units is not positive definite at grid index " +
                                             std::to_string(P.g_idx[k]) + " (alpha = " + std::to_string(P.g_alpha[k]) + ")");
      HMSC_REQUIRE(infos[r][2 * k + 1] == 0,
                   nm + "the conditional covariance W = K22 - K12' K11^-1 K12 of the new units is not positive definite "
                        "at grid index " + std::to_string(P.g_idx[k]) + " (alpha = " + std::to_string(P.g_alpha[k]) +
                       "): coincident new units?");
    }
    HMSC_REQUIRE(infos[r][P.ipg * ng] != 2, nm + "non-finite coordinates");
    HMSC_REQUIRE(infos[r][P.ipg * ng] == 0, nm + "a neighbour kernel matrix K11 is not positive definite");
  }
}

}  // namespace hmsc
