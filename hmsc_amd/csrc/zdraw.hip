// updateZ launcher (R/updateZ.R:4-94): the fused z kernel of z_kernel.h and its slab
// reductions.  Its own translation unit: it is compiled with MachineLICM off (build.py), so
// the ~60 polynomial constants of the inlined truncated-normal draws are materialised where
// they are used inside the site loop instead of being hoisted into (and spilled from) the
// register file.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "rng.h"
#include "state.h"
#include "z_kernel.h"

namespace hmsc {

PackArgs record_pack_args(State& s, int part);  // kernels.hip

#ifdef HMSC_STAMPS
__device__ unsigned long long g_zstamps[Z_NSTAMP];
#endif

// the z kernel's phase stamps (z_kernel.h Z_STAMP), diagnostic build only
void read_zstamps(double* out, int n) {
#ifdef HMSC_STAMPS
  unsigned long long h[Z_NSTAMP];
  HMSC_REQUIRE(n <= Z_NSTAMP, "zstamps: at most 64 slots");
  HIP_OK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_zstamps), sizeof(h)));
  for (int i = 0; i < n; ++i) out[i] = (double)h[i];
#else
  (void)out;
  (void)n;
  throw HmscError(-1, "zstamps: this library was built without --stamps");
#endif
}

// Z Tr is only consumed with NA (updateGamma2 forms X^T Z Tr from XZ otherwise, and a
// sharded chain all-reduces that), so the no-NA kernels skip the ZTr contraction
template <bool HAS_NA>
constexpr int z_mode() { return HAS_NA ? Z_ALL : (Z_ALL & ~8); }

template <bool DRAW, bool HAS_NA, bool POIS, bool NORMAL, bool LEAN = false>
static void z_dispatch_k(const State& s, dim3 grid, size_t smem, const ZArgs& a) {
  constexpr int M = z_mode<HAS_NA>();
  with_bucket<1, 2, 3, 4, 8>(z_nkb(s.K), [&](auto nkb) {
    z_wave_kernel<DRAW, HAS_NA, decltype(nkb)::value, M, POIS, NORMAL, LEAN><<<grid, 256, smem, s.stream>>>(a);
  });
}

// lean: the trimmed pair draw of an all-probit chain without NA cells at unit scale (z_kernel.h LEAN)
template <bool DRAW, bool HAS_NA, bool POIS = false>
static void z_dispatch(const State& s, dim3 grid, size_t smem, const ZArgs& a, bool lean = false) {
  if constexpr (DRAW && !HAS_NA && !POIS) {
    if (lean) return z_dispatch_k<DRAW, HAS_NA, POIS, false, true>(s, grid, smem, a);
  }
  if (!DRAW || POIS || s.any_normal)
    z_dispatch_k<DRAW, HAS_NA, POIS, true>(s, grid, smem, a);
  else
    z_dispatch_k<DRAW, HAS_NA, POIS, false>(s, grid, smem, a);
}

template <bool HAS_NA>
static int z_occupancy(int nkb, size_t smem) {
  int nb = 0;
  with_bucket<1, 2, 3, 4, 8>(nkb, [&](auto b) {
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &nb, z_wave_kernel<true, HAS_NA, decltype(b)::value, z_mode<HAS_NA>()>, 256, smem));
  });
  return nb;
}

int z_xeta_cols_for(int Kmax) { return z_xeta_cols(Kmax); }

// Workgroups of the drawing z kernel resident on the whole device at once (occupancy x CUs):
// one round of the (species block x site chunk) grid, which the schedule below is sized by.
int z_resident_slots(const State& s) {
  const size_t smem = z_smem_bytes(s.Kmax, s.nt);
  const int nkb = z_nkb(s.Kmax);
  int ncu = 0;
  const int nb = s.has_na ? z_occupancy<true>(nkb, smem) : z_occupancy<false>(nkb, smem);
  HIP_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s.device));
  return std::max(1, nb) * std::max(1, ncu);
}

// The z kernel draws a species quad from one Philox block, indexed (sp0 + j) >> 2: a shard that
// started elsewhere would draw other uniforms than the unsharded chain.
void z_require_shard_start(int sp0) {
  HMSC_REQUIRE((sp0 & 3) == 0,
               "updateZ: species shards must start at a multiple of 4 species (one Philox block per species quad)");
}

// Tiles per chunk of the default schedule's last round.  Config 4 (R = 32 rows to a round, 157
// tiles), same-box 1000-step medians in sweeps/s: 32x4 + 29x1 7,516; 32x3 + 31x2 7,356; 32x3 +
// 32x1 + 29x1 7,295; 64x2 + 29x1 7,221; uniform 2 (the rule before) 7,221; uniform 3 7,130
// (profiles/zsched_ab_parts.txt).
constexpr int Z_LAST_T = 1;

// The site-chunk schedule of the z grid, fixed when the chain is created (the rule: capi.cpp
// setup_workspaces).  Chunk rows are dispatched in order, species blocks fastest, so the long
// chunks of the first segment fill the first round and the short ones the last.  The list is
// normalised against the tile count: a segment is cut where the tiles end, the last one extended
// to cover them, so no chunk is empty.  Draws do not depend on it (one Philox block per site
// and species quad); XZ only by the grouping of its partial sums.
void z_schedule_setup(State& s) {
  const int n_tiles = (s.ny + ZT_I - 1) / ZT_I;
  constexpr int NIN = 8;
  int in_n[NIN], in_t[NIN], nin = 0;
  bool uniform = false;
  if (!s.knobs.z_sched.empty()) {  // "n1xt1,n2xt2,..." (a bare number: one chunk of that many tiles)
    const char* p = s.knobs.z_sched.c_str();
    while (*p) {
      char* q = nullptr;
      long n = std::strtol(p, &q, 10), t = 0;
      HMSC_REQUIRE(q != p && nin < NIN, "HMSC_Z_SCHED: expected n1xt1,n2xt2,... (at most 8 segments)");
      if (*q == 'x' || *q == 'X') {
        p = q + 1;
        t = std::strtol(p, &q, 10);
        HMSC_REQUIRE(q != p, "HMSC_Z_SCHED: expected n1xt1,n2xt2,... (at most 8 segments)");
      } else {
        t = n;
        n = 1;
      }
      HMSC_REQUIRE(n >= 1 && t >= 1 && n <= (1 << 20) && t <= (1 << 20), "HMSC_Z_SCHED: counts must be positive");
      HMSC_REQUIRE(nin == 0 || t <= in_t[nin - 1], "HMSC_Z_SCHED: tiles per chunk must not increase");
      HMSC_REQUIRE(*q == ',' || *q == 0, "HMSC_Z_SCHED: expected n1xt1,n2xt2,... (at most 8 segments)");
      in_n[nin] = (int)n;
      in_t[nin++] = (int)t;
      p = *q ? q + 1 : q;
    }
    HMSC_REQUIRE(nin > 0, "HMSC_Z_SCHED: empty schedule");
  } else if (s.nchunk > 0) {  // HMSC_Z_CHUNKS: a uniform split
    uniform = true;
    s.nchunk = std::max(1, std::min(n_tiles, s.nchunk));
    in_t[0] = (n_tiles + s.nchunk - 1) / s.nchunk;
    in_n[0] = (n_tiles + in_t[0] - 1) / in_t[0];
    nin = 1;
  } else {
    const int R = std::max(1, z_resident_slots(s) / std::max(1, s.ntile_j));  // chunk rows to a round
    if (n_tiles <= R) {
      in_n[0] = n_tiles, in_t[0] = 1, nin = 1;
    } else {
      in_n[0] = R, in_t[0] = std::max(Z_LAST_T, (n_tiles - Z_LAST_T * R + R - 1) / R);
      in_n[1] = 1, in_t[1] = Z_LAST_T;  // (extended below to the remaining tiles)
      nin = 2;
    }
  }
  int nseg = 0, rem = n_tiles, chunks = 0;
  for (int g = 0; g < Z_NSEG; ++g) s.z_seg_n[g] = s.z_seg_t[g] = 0;
  for (int g = 0; g < nin && rem > 0; ++g) {
    const int need = (rem + in_t[g] - 1) / in_t[g];
    const int n = (g == nin - 1 || in_n[g] >= need) ? need : in_n[g];
    if (nseg > 0 && s.z_seg_t[nseg - 1] == in_t[g]) {
      s.z_seg_n[nseg - 1] += n;
    } else {
      HMSC_REQUIRE(nseg < Z_NSEG, "HMSC_Z_SCHED: more than 4 segments are in use");
      s.z_seg_n[nseg] = n;
      s.z_seg_t[nseg++] = in_t[g];
    }
    chunks += n;
    rem -= std::min((long long)rem, (long long)n * in_t[g]);
  }
  s.z_chunks = chunks;
  if (!uniform) s.nchunk = chunks;
}

static void run_z_fused(State& s, bool draw, uint32_t iter, bool use_raw_y) {
  HMSC_REQUIRE(s.K <= KMAX_Z, "updateZ: K = nc + sum(nf) must be <= 128 in this build");
  z_require_shard_start(s.sp0);
  if (!s.xeta_valid) launch_xeta(s);
  ZArgs a{};
  a.XEta = s.XEta;
  a.ny = s.ny;
  a.K = s.K;
  a.ns_loc = s.nsl;
  a.sp0 = s.sp0;
  a.nt = s.nt;
  for (int g = 0; g < Z_NSEG; ++g) a.seg[g] = ZSeg{s.z_seg_n[g], s.z_seg_t[g]};
  const int nchunk = s.z_chunks;
#ifdef HMSC_STAMPS
  a.stamp_by = std::min(s.knobs.z_stamp_by, s.ntile_j - 1);
  a.stamp_chunk = std::min(s.knobs.z_stamp_chunk, nchunk - 1);
#endif
  // (the initial Z is drawn from the unmasked X, R/computeInitialParameters.R:34-50,229-254)
  a.BL = use_raw_y ? s.BL : s.BLx;
  a.iSigma = s.iSigma;
  a.Ycode = s.Ycode;
  a.Ybits = s.Ybits;
  a.logtab = s.logtab;
  a.ztab = s.logtab + ZLOG_W * ZLOG_N;
  a.Yval = use_raw_y ? s.Yraw : s.Yval;
  a.fam = s.fam;
  a.Tr = s.Tr;
  a.Z = s.Z;
  a.XZ_part = s.XZ_part;
  a.ZTr_part = s.ZTr_part;
  a.key = s.key;
  a.iter = iter;
  a.iter_dev = iter_src(s);
  a.noise_zero = s.noise_mode;
  a.zprev_is_e = use_raw_y;  // only the init draw reads hM$Y (R/computeInitialParameters.R:254)
  a.mask_na = s.phylo ? 0 : 1;
  a.kt = kt_slot(s, KT_Z);
  dim3 grid(s.ntile_j, nchunk);  // species blocks fastest (z_kernel.h)
  size_t smem = z_smem_bytes(s.K, s.nt);
  // The record pack is this launch's last grid row, so the slab launch after z sums XZ only:
  // its ntile_j pack workgroups dispatch last and overlap z's final round (1000-step config 4:
  // 6,852 sweeps/s against 6,761 with the pack in the slab launch, three same-box rounds,
  // profiles/r06_packrow_ab.txt).  Leaving XZ as chunk partials for the fused Gamma2 +
  // BetaLambda launch to sum where it reads them lost to the reduction launch (6,601-6,688
  // against 6,677-6,713 sweeps/s: ~15 MB of partial loads land on the BetaLambda prologue,
  // profiles/r05_fold_ab2.txt) and is gone.
  a.pack_row = 0;
  if (draw && !s.sharded && s.pack_req && s.side_fused && s.capturing) {
    a.pack_row = 1;
    a.pack = record_pack_args(s, 1);
    grid.y += 1;
    s.pack_req = false;
    s.pack_done = true;
  }
  if (draw && s.g_pending) {  // G's Eta rows reduced on an extra first grid row
    a.gred_y0 = 1;
    a.gred_ntile = s.g_ntile;
    a.gred_nf = s.g_nf;
    a.gred_Kmax = s.Kmax;
    a.gred_groups = (s.K * s.g_nf + 63) / 64;
    a.gred_part = s.G_part;
    a.gred_XX = s.XX;
    a.gred_G = s.G;
    grid.y += 1;
    smem = std::max(smem, (size_t)256 * sizeof(double));
    s.g_pending = false;
  }
  // The lean pair draw (z_kernel.h LEAN) holds no NA handling and no scale.  It needs "no code
  // is -1" in Ycode / Ybits: that is what has_na == false says -- setup_species_data (capi.cpp)
  // sets has_na in the very loop that writes code -1, over this rank's species, which are the
  // launch's; the padding of Ybits past the last species and site holds code 0.  And it needs
  // sd = isd = 1.0 exactly for every species: all probit, whose iSigma updateInvSigma leaves at
  // its initial 1, and no iSigma set from outside since (hmsc_set_state clears isigma_fixed_one)
  // -- the condition updateGamma2 already relies on (kernels.hip check_isigma).  HMSC_Z_GENERAL
  // (read at create) keeps such a chain on the general draw, so one build can be compared with
  // itself.
  const bool lean = draw && !s.any_poisson && !s.has_na && s.all_probit && s.isigma_fixed_one && !s.knobs.z_general;
  if (draw) s.z_lean_last = lean ? 1 : 0;
  {
    ProfScope ps(s, PROF_Z);
    if (draw && s.any_poisson) {
      if (s.has_na)
        z_dispatch<true, true, true>(s, grid, smem, a);
      else
        z_dispatch<true, false, true>(s, grid, smem, a);
    } else if (draw) {
      if (s.has_na)
        z_dispatch<true, true>(s, grid, smem, a);
      else
        z_dispatch<true, false>(s, grid, smem, a, lean);
    } else {
      if (s.has_na)
        z_dispatch<false, true>(s, grid, smem, a);
      else
        z_dispatch<false, false>(s, grid, smem, a);
    }
    HIP_OK(hipGetLastError());
  }
  // XZ and ZTr from their partials, one launch
  const int64_t nXZ = (int64_t)s.K * s.nsl, nZT = s.has_na ? (int64_t)s.ny * s.nt : 0;
  const SideGate gate = draw ? side_gate_next(s, iter) : SideGate{};
  if (draw && s.pack_req && (s.side_fused || sharded_pack_split(s)) && s.capturing) {
    launch_slab_sum2_pack(s, s.XZ_part, s.XZ, nXZ, nchunk, s.ZTr_part, s.ZTr, nZT, s.ntile_j, gate);
    s.pack_req = false;
    s.pack_done = true;
  } else {
    launch_slab_sum2(s.XZ_part, s.XZ, nXZ, nchunk, s.ZTr_part, s.ZTr, nZT, s.ntile_j, s.stream, gate);
  }
}

// the z kernel's tables in one device buffer: the log table, then z_draw_tables
int z_log_table_doubles() { return ZLOG_W * ZLOG_N + ZT_DOUBLES; }
void z_log_table_fill(double* t) {
  z_log_table(t);
  z_draw_tables(t + ZLOG_W * ZLOG_N);
}

// hmsc_debug_eval "trunc_normal_tab" / "trunc_normal_poly": the z kernel's pair draws on arrays a
// test supplies.  Elements 2k and 2k + 1 are one pair (a cell with alpha > 25 takes its partner
// onto the scalar path with it); e = -alpha, sd = isd = 1, code 1, or code -1 for alpha = -inf,
// so x = z - e.  The LDS tables are staged from z_log_table_fill's buffer as z_wave_kernel
// stages them.
template <bool TAB>
__global__ __launch_bounds__(256) void z_pair_eval_kernel(int64_t n, const double* alpha, const double* u, double* x,
                                                          const double* logtab, const double* ztab) {
  __shared__ __attribute__((aligned(16))) double sLog[ZLOG_W * ZLOG_N];
  __shared__ __attribute__((aligned(16))) double sZT[ZT_DOUBLES];
  const int t = threadIdx.x;
  constexpr int NZT = (ZT_DOUBLES + 255) / 256;
  if (t < ZLOG_W * ZLOG_N) sLog[t] = logtab[t];
#pragma unroll
  for (int k = 0; k < NZT; ++k)
    if (t + 256 * k < ZT_DOUBLES) sZT[t + 256 * k] = ztab[t + 256 * k];
  __syncthreads();
  const int64_t npair = (n + 1) / 2;
  for (int64_t p = (int64_t)blockIdx.x * 256 + t; p < npair; p += (int64_t)gridDim.x * 256) {
    const int64_t i0 = 2 * p, i1 = 2 * p + 1;
    const bool two = i1 < n;
    const double al0 = alpha[i0], al1 = two ? alpha[i1] : 0.0;
    const double u0 = u[i0], u1 = two ? u[i1] : 0.5;
    const int c0 = al0 == -INFINITY ? -1 : 1, c1 = al1 == -INFINITY ? -1 : 1;
    const double e0 = c0 < 0 ? 0.0 : -al0, e1 = c1 < 0 ? 0.0 : -al1;
    const ZPair z = TAB ? z_probit_pair_tab(e0, e1, 1.0, 1.0, 1.0, 1.0, c0, c1, u0, u1, 0, sLog, sZT)
                        : z_probit_pair(e0, e1, 1.0, 1.0, 1.0, 1.0, c0, c1, u0, u1, 0, sLog);
    x[i0] = z.z0 - e0;
    if (two) x[i1] = z.z1 - e1;
  }
}

// tab: the z kernel's buffer (z_log_table_doubles() doubles, z_log_table_fill) on the device
void launch_z_pair_eval(hipStream_t st, bool tab_draw, int64_t n, const double* alpha, const double* u, double* x,
                        const double* tab) {
  const int grid = (int)std::min<int64_t>(1024, ((n + 1) / 2 + 255) / 256);
  if (tab_draw)
    z_pair_eval_kernel<true><<<grid, 256, 0, st>>>(n, alpha, u, x, tab, tab + ZLOG_W * ZLOG_N);
  else
    z_pair_eval_kernel<false><<<grid, 256, 0, st>>>(n, alpha, u, x, tab, tab + ZLOG_W * ZLOG_N);
  HIP_OK(hipGetLastError());
}

void launch_update_z(State& s, uint32_t iter, bool use_raw_y) {
  run_z_fused(s, true, iter, use_raw_y);
  s.zt_valid = true;
}

void launch_zt_refresh(State& s) {
  run_z_fused(s, false, 0, false);
  s.zt_valid = true;
}

}  // namespace hmsc
