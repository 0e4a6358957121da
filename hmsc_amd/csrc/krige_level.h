// The kriging of one spatial level on the host side: what hmsc_krige (all new units in one call) and
// hmsc_predict_map (new units slab by slab) share around the group launchers of krige.hip / gpp.hip.
// Both describe a level as a KrigeSpec, group its (sample, factor) pairs with krige_group_pairs, check
// the mode's arguments with krige_check_mode, size the plan with krige_need_bytes and drive a
// KrigeLevel (krige_level.hip): prepare, run per set of new units, collect, report.  The grouping,
// the checks and the byte counts are plain host functions (no device call): tests/capi/krige_plan_check.cpp
// runs them on a machine without a GPU.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "state.h"

namespace hmsc {

// what a caller describes of a level: hmsc_krige_args' and hmsc_map_level's fields
struct KrigeSpec {
  int mode, np, nn, sDim, nK, nNeighbours, G, S, nf, level;
  const double *coords, *dist, *knots, *alphas, *Eta;
  const int32_t* alpha;  // S x nf, 1-based grid indices, 0: no such factor
  uint64_t seed;
};

// the (s, h) pairs by grid index, the distinct indices in ascending order
struct KrigeGroups {
  std::vector<int> col_s, col_h, g_idx, g_off{0};
  std::vector<double> g_alpha;
  std::vector<int> zflag;  // S x nf: 1 = a new unit's value is z, written by the map's assembly kernel
  size_t cmax = 0;         // most pairs of a grid value > 0
  size_t size() const { return g_idx.size(); }
  int cols(size_t k) const { return g_off[k + 1] - g_off[k]; }
};

// 'GPP' files every factor of a sample under the index of its last one (R's ag = alpha[nf]).
// keep_zero: the groups at a = 0 stay (hmsc_krige: its launcher writes z).  Otherwise (the map) they
// are left to the assembly kernel through zflag -- except mode 3, whose kernel writes z itself -- and a
// level without new units has no groups at all.
inline KrigeGroups krige_group_pairs(const KrigeSpec& q, bool keep_zero, const std::string& nm) {
  const size_t S = q.S, nf = q.nf;
  KrigeGroups o;
  std::vector<std::vector<int>> by_g(q.G + 1);
  o.zflag.assign(S * nf, 0);
  for (size_t s = 0; s < S; ++s) {
    int glast = 0;
    for (size_t h = 0; h < nf; ++h) {
      const int g = q.alpha[s * nf + h];
      HMSC_REQUIRE(g >= 0 && g <= q.G, nm + "grid index " + std::to_string(g) + " of sample " + std::to_string(s) +
                                           ", factor " + std::to_string(h) + " is outside the alphapw grid 1.." +
                                           std::to_string(q.G));
      if (g > 0) glast = g;
    }
    for (size_t h = 0; h < nf; ++h) {
      const int g = q.alpha[s * nf + h] > 0 ? (q.mode == 4 ? glast : q.alpha[s * nf + h]) : 0;
      if (g > 0) by_g[g].push_back((int)(s * nf + h));
      if (g > 0 && !(q.alphas[g - 1] > 0.0) && q.mode != 0 && q.mode != 3) o.zflag[s * nf + h] = 1;
    }
  }
  for (int g = 1; g <= q.G; ++g) {
    if (by_g[g].empty()) continue;
    const bool pos_a = q.alphas[g - 1] > 0.0;
    if (!pos_a && !keep_zero && q.mode != 3) continue;
    HMSC_REQUIRE(!pos_a || q.coords || q.dist, nm + "a grid value > 0 needs coords or dist");
    for (int pr : by_g[g]) o.col_s.push_back(pr / (int)nf), o.col_h.push_back(pr % (int)nf);
    o.g_idx.push_back(g);
    o.g_alpha.push_back(q.alphas[g - 1]);
    o.g_off.push_back((int)o.col_s.size());
    if (pos_a) o.cmax = std::max(o.cmax, by_g[g].size());
  }
  if (!keep_zero && q.nn == 0) o.g_idx.clear(), o.g_alpha.clear(), o.g_off.assign(1, 0), o.col_s.clear(), o.col_h.clear(), o.cmax = 0;
  return o;
}

// the arguments modes 3 and 4 need (hmsc_krige: whenever the mode is given; the map: when a group needs them)
inline void krige_check_mode(const KrigeSpec& q, const std::string& nm) {
  if (q.mode == 3) {
    HMSC_REQUIRE(q.coords != nullptr, nm + "NNGP kriging needs coordinates; a distMat level predicts with 'Full'");
    HMSC_REQUIRE(q.nNeighbours >= 1, nm + "nNeighbours must be positive");
    HMSC_REQUIRE(q.nNeighbours <= 32, nm + "NNGP kriging on the device takes nNeighbours <= 32 (got " +
                                          std::to_string(q.nNeighbours) + ")");
    HMSC_REQUIRE(q.nNeighbours <= q.np, nm + "nNeighbours exceeds the number of fitted units");
  }
  if (q.mode == 4) {
    HMSC_REQUIRE(q.coords != nullptr && q.dist == nullptr,
                 nm + "GPP kriging needs coordinates; a distMat level predicts with 'Full'");
    HMSC_REQUIRE(q.knots != nullptr && q.nK > 0, nm + "GPP kriging needs knots (knots with nK > 0)");
  }
}

// Device bytes of a level's kriging: the posterior Eta, the geometry, the pair tables, the info and
// handshake words and the workspaces by mode.
//   one-shot (hmsc_krige): the output, and one workspace shared by the grid values for all nn new units;
//   resident (a map level): per grid value K11, its factor's workspace and Y, or iWss and C, plus one
//   slab's K12 and v for at most `slab` new units ('Full': the one-shot workspace).
// The map adds its own share (Lambda, the Eta table, the unit lists, zflag).
inline uint64_t krige_need_bytes(const KrigeSpec& q, const KrigeGroups& g, bool resident, size_t slab) {
  const uint64_t np = q.np, nn = q.nn, N = np + nn, S = q.S, nf = q.nf, nK = q.nK, ng = g.size(), cmax = g.cmax;
  const uint64_t ncols = g.col_s.size();
  const bool gpp = q.mode == 4, dense = q.mode != 3 && !gpp && cmax > 0, full = dense && q.mode == 2;
  uint64_t dbl = S * np * nf;
  if (!resident) dbl += S * nn * nf;
  if (!resident || ng > 0) dbl += q.coords ? N * q.sDim : N * N;
  if (dense && (full || !resident)) {
    dbl += np * np + np * (nn + cmax) + dense_ws_doubles(q.np);
    if (q.mode == 1) dbl += nn;
    if (full) dbl += nn * nn + nn * cmax + dense_ws_doubles(q.nn);
  } else if (dense) {
    dbl += ng * (np * np + dense_ws_doubles(q.np)) + np * ncols + np * slab + slab;
  }
  if (gpp && (!resident || cmax > 0)) dbl += nK * q.sDim;
  if (gpp && cmax > 0) {
    dbl += gpp_plan_doubles(q.np, q.nK, (int)cmax);
    dbl += resident ? ng * nK * nK + nK * ncols + slab : nK * nK + nK * cmax + nn;
  }
  const uint64_t words = resident ? 6 * ng : ((gpp ? 4 : 2) + 1) * ng;
  return dbl * sizeof(double) + (2 * ncols + words + 2 + DENSE_SYNC_INTS) * sizeof(int);
}

// The plan of one level.  Host targets of the stream's copies live here: declare it before the
// DeviceOwner whose stream it uses.
class KrigeLevel {
 public:
  KrigeSpec q{};
  KrigeGroups g;

  // Uploads and allocations by mode.  resident: the map's plan -- per grid value what the fitted units
  // alone decide is made here, once (krige_plan_group, gpp_plan_group), and run() serves slabs of at
  // most `slab` new units; otherwise run() is hmsc_krige's single pass over slab = nn units.
  // timed: events around the phases (each_elapsed); a resident plan always has them.
  void prepare(DeviceOwner& own, hipStream_t st, bool resident, size_t slab, bool timed);
  // the launches for the nn new units `unit` (null: 0 .. nn - 1), written to out with ld ldo;
  // false: nothing to launch
  bool run(hipStream_t st, const int* unit, int nn, double* out, size_t ldo);
  // the info words and the handshake word, copied back on st; report() after st has drained
  void collect(hipStream_t st);
  void report(const std::string& nm) const;
  // f(group, phase, ms) for every interval the last run() recorded; group -1: one interval around the
  // whole run (mode 3, a resident 'Full' level)
  template <class F>
  void each_elapsed(F&& f) const {
    if (ev_.empty()) return;
    float ms = 0.f;
    if (epg_ == 0) {
      HIP_OK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
      f(-1, 0, (double)ms);
      return;
    }
    for (size_t k = 0; k < g.size(); ++k)
      for (int ph = 0; ph + 1 < epg_; ++ph) {
        HIP_OK(hipEventElapsedTime(&ms, ev_[k * epg_ + ph], ev_[k * epg_ + ph + 1]));
        f((int)k, ph, (double)ms);
      }
  }
  const KrigeDev& dev() const { return d_; }

 private:
  void events(DeviceOwner& own, size_t n) {
    ev_.resize(n);
    for (auto& e : ev_) e = own.event();
  }
  KrigeDev d_{};
  bool resident_ = false;
  int ipg_ = 2;                           // info words per group (4: 'GPP')
  int* info_ = nullptr;                   // ipg_ per group, then the NNGP kernel's
  const double* d_galpha_ = nullptr;      // mode 3
  const int* d_goff_ = nullptr;
  GppWork gw_{};
  std::vector<double*> K11_, ws_, Y_;     // resident, per group
  std::vector<double*> iWss_, Cm_;        // 'GPP': per group (resident) or one for all
  std::vector<hipEvent_t> ev_;
  int epg_ = 0;                           // events per group; 0: one pair around the run
  std::vector<int> info_h_;
  int hs_ = 0;
};

void run_krige(const hmsc_krige_args* args, double* out);

}  // namespace hmsc
