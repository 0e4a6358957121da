// The kriging level plan (krige_level.h) and hmsc_krige on top of it.  Host code only: the kernels and
// the group launchers are krige.hip's and gpp.hip's.
#include "krige_level.h"

namespace hmsc {

void KrigeLevel::prepare(DeviceOwner& own, hipStream_t st, bool resident, size_t slab, bool timed) {
  const size_t np = q.np, nn = q.nn, N = np + nn, S = q.S, nf = q.nf, nK = q.nK, ng = g.size(), cmax = g.cmax;
  auto up = [&](const auto* src, size_t n) { return own.upload(src, n, st); };
  resident_ = resident;
  timed = timed || resident;
  d_.np = q.np, d_.sdim = q.coords ? q.sDim : 0, d_.S = q.S, d_.nfmax = q.nf, d_.N = (int)N;
  d_.seed = q.seed;
  d_.stream = S_KRIGE + LEVEL_STRIDE * (uint32_t)q.level;
  d_.Eta = up(q.Eta, S * np * nf);
  ipg_ = q.mode == 4 ? 4 : 2;
  info_h_.assign(ipg_ * ng + 1, 0);
  info_ = own.alloc<int>(ipg_ * ng + 1);
  if (ng == 0) return;
  double* geo = q.coords ? up(q.coords, N * q.sDim) : up(q.dist, N * N);
  d_.coords = q.coords ? geo : nullptr;
  d_.dist = q.coords ? nullptr : geo;
  d_.col_s = up(g.col_s.data(), g.col_s.size());
  d_.col_h = up(g.col_h.data(), g.col_h.size());
  if (q.mode == 3) {
    d_galpha_ = up(g.g_alpha.data(), ng);
    d_goff_ = up(g.g_off.data(), ng + 1);
    if (timed) events(own, 2);
    return;
  }
  // one pass: krige_launch_group's KRIGE_GROUP_PHASES, 'GPP' its plan's and its slab's in their place
  if (timed && !resident) epg_ = KRIGE_GROUP_PHASES + 1, events(own, ng * epg_);
  if (q.mode == 4) {
    d_.knots = up(q.knots, nK * q.sDim);
    d_.nK = q.nK;
  }
  if (cmax == 0) return;  // every group at a = 0: z
  d_.sync = own.alloc<int>(DENSE_SYNC_INTS);
  if (q.mode == 4) {
    if (resident) epg_ = 3, events(own, ng * epg_);  // per slab: the dDn pass, the slab product
    d_.v = own.alloc<double>(slab);
    gw_ = gpp_carve(own.alloc<double>(gpp_plan_doubles(q.np, q.nK, (int)cmax)), q.np, q.nK, (int)cmax);
    for (size_t k = 0; k < (resident ? ng : 1); ++k) {
      iWss_.push_back(own.alloc<double>(nK * nK));
      Cm_.push_back(own.alloc<double>(nK * (resident ? (size_t)g.cols(k) : cmax)));
      if (resident)
        gpp_plan_group(st, d_, gw_, g.g_alpha[k], g.g_off[k], g.cols(k), iWss_[k], Cm_[k], info_ + 4 * k, nullptr);
    }
    return;
  }
  if (!resident || q.mode == 2) {  // krige_launch_group's workspace, shared by the grid values
    d_.K11 = own.alloc<double>(np * np);
    d_.R = own.alloc<double>(np * (nn + cmax));
    d_.ws1 = own.alloc<double>(dense_ws_doubles(q.np));
    if (q.mode == 1) d_.v = own.alloc<double>(nn);
    if (q.mode == 2) {
      d_.W = own.alloc<double>(nn * nn);
      d_.Z = own.alloc<double>(nn * cmax);
      d_.ws2 = own.alloc<double>(dense_ws_doubles(q.nn));
    }
    if (resident) events(own, 2);  // around a slab's groups
    return;
  }
  d_.R = own.alloc<double>(np * slab);
  if (q.mode == 1) d_.v = own.alloc<double>(slab);
  epg_ = 4, events(own, ng * epg_);  // per slab: K12, trsm, mean
  for (size_t k = 0; k < ng; ++k) {
    K11_.push_back(own.alloc<double>(np * np));
    ws_.push_back(own.alloc<double>(dense_ws_doubles(q.np)));
    Y_.push_back(own.alloc<double>(np * (size_t)g.cols(k)));
    krige_plan_group(st, d_, g.g_alpha[k], g.g_off[k], g.cols(k), K11_[k], ws_[k], Y_[k], info_ + 2 * k);
  }
}

bool KrigeLevel::run(hipStream_t st, const int* unit, int nn, double* out, size_t ldo) {
  const int ng = (int)g.size();
  if (nn == 0 || ng == 0) return false;
  KrigeDev d = d_;
  d.nn = nn, d.unit = unit, d.out = out, d.ldo = ldo;
  const bool whole = !ev_.empty() && epg_ == 0;
  if (whole) HIP_OK(hipEventRecord(ev_[0], st));
  if (q.mode == 3) krige_launch_nn(st, d, q.nNeighbours, ng, d_galpha_, d_goff_, info_ + 2 * ng);
  for (int k = 0; q.mode != 3 && k < ng; ++k) {
    const double a = g.g_alpha[k];
    const int col0 = g.g_off[k], c = g.cols(k);
    hipEvent_t* ev = epg_ ? ev_.data() + (size_t)k * epg_ : nullptr;
    if (resident_ && q.mode == 4) {
      gpp_slab_group(st, d, a, col0, c, iWss_[k], Cm_[k], ev);
    } else if (resident_ && q.mode != 2) {
      krige_slab_group(st, d, q.mode, a, col0, c, K11_[k], ws_[k], Y_[k], ev);
    } else if (q.mode == 4 && a > 0.0) {
      gpp_plan_group(st, d, gw_, a, col0, c, iWss_[0], Cm_[0], info_ + 4 * k, ev);
      gpp_slab_group(st, d, a, col0, c, iWss_[0], Cm_[0], ev ? ev + GPP_PLAN_PHASES : nullptr);
    } else {  // 'GPP' at a = 0: out = z
      krige_launch_group(st, d, q.mode == 4 ? 2 : q.mode, a, col0, c, info_ + ipg_ * k, ev);
    }
  }
  if (whole) HIP_OK(hipEventRecord(ev_[1], st));
  return true;
}

void KrigeLevel::collect(hipStream_t st) {
  HIP_OK(hipMemcpyAsync(info_h_.data(), info_, info_h_.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  if (d_.sync) HIP_OK(hipMemcpyAsync(&hs_, d_.sync + DENSE_SYNC_ERR, sizeof(int), hipMemcpyDeviceToHost, st));
}

void KrigeLevel::report(const std::string& nm) const {
  dense_handshake_check(hs_);
  const std::vector<int>& info = info_h_;
  for (size_t k = 0; k < g.size(); ++k) {
    const std::string at = " at grid index " + std::to_string(g.g_idx[k]) + " (alpha = " + std::to_string(g.g_alpha[k]) + ")";
    if (q.mode == 4) {
      HMSC_REQUIRE(info[4 * k] == 0, nm + "GPP: Wss of the knots is not positive definite" + at);
      HMSC_REQUIRE(info[4 * k + 3] == 0, nm + "GPP: fitted unit " + std::to_string(q.np - info[4 * k + 3]) +
                                             " (0-based) lies on a knot or has dD <= 0" + at +
                                             ": its predictive-process variance 1 / dD is not finite");
      HMSC_REQUIRE(info[4 * k + 1] == 0, nm + "GPP: F = Wss + W12' diag(1 / dD) W12 is not positive definite" + at);
      HMSC_REQUIRE(info[4 * k + 2] == 0, nm + "GPP: iF = F^-1 is not positive definite" + at);
    } else {
      HMSC_REQUIRE(info[2 * k] == 0, nm + "K11 of the fitted units is not positive definite" + at);
      HMSC_REQUIRE(info[2 * k + 1] == 0, nm + "the conditional covariance W = K22 - K12' K11^-1 K12 of the new units is "
                                                  "not positive definite" + at + ": coincident new units?");
    }
  }
  HMSC_REQUIRE(info[ipg_ * g.size()] != 2, nm + "non-finite coordinates");
  HMSC_REQUIRE(info[ipg_ * g.size()] == 0, nm + "a neighbour kernel matrix K11 is not positive definite");
}

void run_krige(const hmsc_krige_args* args, double* out) {
  HMSC_REQUIRE(args != nullptr && out != nullptr, "hmsc_krige: NULL argument");
  const hmsc_krige_args& p = *args;
  const std::string nm = "hmsc_krige: ";
  HMSC_REQUIRE(p.np > 0 && p.nn > 0 && p.S > 0 && p.nfmax > 0 && p.G > 0, nm + "np, nn, S, nfmax and G must be positive");
  HMSC_REQUIRE(p.mode >= 0 && p.mode <= 4,
               nm + "mode must be 0 (predictMean), 1 (predictMeanField), 2 (Full), 3 (NNGP) or 4 (GPP)");
  HMSC_REQUIRE(p.alphas != nullptr && p.Eta != nullptr && p.alpha != nullptr, nm + "NULL alphas / Eta / alpha");
  HMSC_REQUIRE((p.coords != nullptr && p.sDim > 0) || p.dist != nullptr, nm + "coords (with sDim > 0) or dist is needed");
  HMSC_REQUIRE(p.level >= 0 && p.level < HMSC_MAX_LEVELS, nm + "bad level");
  KrigeLevel L;  // (host targets of the stream's copies: before the stream's owner)
  L.q = KrigeSpec{p.mode, p.np, p.nn, p.sDim, p.mode == 4 ? p.nK : 0, p.nNeighbours, p.G, p.S, p.nfmax, p.level,
                  p.coords, p.dist, p.knots, p.alphas, p.Eta, p.alpha, p.seed};
  krige_check_mode(L.q, nm);
  L.g = krige_group_pairs(L.q, true, nm);
  const size_t nn = p.nn, nout = (size_t)p.S * nn * p.nfmax;
  std::fill(out, out + nout, 0.0);
  if (p.kernel_ms) std::fill(p.kernel_ms, p.kernel_ms + KRIGE_GROUP_PHASES + 1, 0.0);
  if (L.g.size() == 0) return;
  DeviceGuard dg(p.device);
  // device memory, taken once: refuse by name what the device cannot hold
  const uint64_t need = krige_need_bytes(L.q, L.g, false, nn);
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  HMSC_REQUIRE(need <= free_b, nm + "the call needs " + std::to_string(need) + " bytes of device memory (np = " +
                                   std::to_string(p.np) + ", nn = " + std::to_string(nn) +
                                   (p.mode == 4 ? ", nK = " + std::to_string(p.nK) : std::string()) + "), the device has " +
                                   std::to_string(free_b) + " bytes free");
  DeviceOwner own;
  const hipStream_t st = own.stream();
  L.prepare(own, st, false, nn, p.kernel_ms != nullptr);
  double* dout = own.alloc<double>(nout);  // zeroed
  L.run(st, nullptr, p.nn, dout, nn);
  L.collect(st);
  HIP_OK(hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  L.report(nm);
  // 'GPP' records its plan's five phases, then the dDn pass and the slab product
  static const int gpp_slot[KRIGE_GROUP_PHASES] = {0, 1, 4, 5, 6, 2, 3};
  L.each_elapsed([&](int k, int ph, double ms) {
    if (k < 0)
      p.kernel_ms[KRIGE_GROUP_PHASES] = ms;
    else
      p.kernel_ms[p.mode == 4 && L.g.g_alpha[k] > 0.0 ? gpp_slot[ph] : ph] += ms;
  });
}

}  // namespace hmsc
