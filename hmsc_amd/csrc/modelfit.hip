// evaluateModelFit on the device (R/evaluateModelFit.R:53-169; the host function in
// hmsc_amd/predict.py is the specification): RMSE, R2, AUC, TjurR2, SR2, O.AUC, O.TjurR2, O.RMSE,
// C.SR2 and C.RMSE of every species in one call, from Y, the per-cell mean (the median in Poisson
// columns) m and the share of positive draws pO.
//
// One workgroup of 1024 threads per species does everything the species needs, one step after
// the other; no workgroup waits for another and there are no atomics.
//
// Ranks by counting.  A rank job takes a column x and a row mask and gives every kept row its
// average rank (#kept < x) + (#kept == x + 1) / 2.  The kept rows' order-preserving 64-bit keys
// (quantile_select.h order_key, -0.0 canonicalised to +0.0) are sorted chunk by chunk in LDS with
// a key-only bitonic network; rows that are not kept and the padding to the power of two hold the
// all-ones key, which lies above order_key(+inf), so they sort behind every kept value.  Each
// thread then finds, by binary search in every sorted chunk, how many keys lie below its row's key
// and how many are not above it; the two counts summed over the chunks are the two terms of the
// rank.  The counts are integers, so no merge of the chunks is needed, a tie run may span chunks,
// and the rank does not depend on the chunk size.  A column that fits one chunk is searched in LDS;
// otherwise the sorted chunks go to the species' scratch in global memory and are searched there.
//
// Sums.  Every sum is in fp64 in one fixed order: thread t adds its rows t, t + 1024, ... in
// ascending order, the 64 lanes of a wave combine in a fixed shuffle tree, and the 16 wave sums are
// added in ascending order.  Nothing in that order depends on chunk_rows, scratch_bytes, the
// slab or the grid, so every output repeats bit for bit.  Rank sums are sums of half-integers and
// exact.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../include/hmsc_amd.h"
#include "common.h"
#include "devmem.h"
#include "quantile_select.h"

namespace hmsc {

#pragma clang fp contract(off)  // the sums as written: no fused multiply-add changes a rounding

constexpr int MF_NT = 1024, MF_NW = MF_NT / WAVE;
constexpr int MF_CAP = 16384;   // keys of the large sort bucket: 128 KiB of the CU's 160 KiB LDS
constexpr int MF_SMALL = 1024;  // ... and of the small one
constexpr int MF_OUT = 10;
enum MfOut { MF_RMSE = 0, MF_R2, MF_AUC, MF_TJUR, MF_SR2, MF_OAUC, MF_OTJUR, MF_ORMSE, MF_CSR2, MF_CRMSE };

struct MfArgs {
  int ny, ns, nsl, j0, chunk;  // nsl species of the slab, the first is species j0; chunk rows per sort
  const double *Y, *m, *pO;    // the slab's columns (pO null: no Poisson column in the call)
  const int* family;           // ns
  double* scratch;             // nsl x 3 ny: sorted keys, two rank columns
  double* out;                 // MF_OUT x ns
};

// K sums at once in the fixed order of the header; every thread gets all of them
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red) {
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, WAVE);
    if (lane == 0) red[k * MF_NW + w] = v[k];
  }
  __syncthreads();
  if (t < K) {
    double s = red[t * MF_NW];
    for (int q = 1; q < MF_NW; ++q) s += red[t * MF_NW + q];
    red[K * MF_NW + t] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = red[K * MF_NW + k];
  __syncthreads();
}

__device__ __forceinline__ uint64_t rank_key(double x) {
  const uint64_t k = order_key(x);
  return k == 0x7FFFFFFFFFFFFFFFull ? 0x8000000000000000ull : k;  // -0.0 ties with +0.0
}

// ascending key-only bitonic sort of s[0 .. P), P a power of two; all threads of the workgroup
__device__ __forceinline__ void bitonic_sort(uint64_t* s, int P) {
  const int t = threadIdx.x;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = t; q < (P >> 1); q += MF_NT) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
        const uint64_t a = s[i], b = s[l];
        if ((a > b) == ((i & k) == 0)) s[i] = b, s[l] = a;
      }
      __syncthreads();
    }
}

// number of keys of the ascending s[0 .. n) below x (lo) and not above x (hi)
__device__ __forceinline__ void count_bounds(const uint64_t* s, int n, uint64_t x, int& lo, int& hi) {
  int a = 0, b = n;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (s[mid] < x) a = mid + 1; else b = mid;
  }
  lo += a;
  b = n;  // the first key above x is not before the first key that is not below it
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (s[mid] <= x) a = mid + 1; else b = mid;
  }
  hi += a;
}

// The average ranks of val(i) among the rows with keep(i), into rk[i] for those rows.
// skey: LDS for one chunk's keys; gkeys: the species' ny sorted keys when there are several chunks.
template <class V, class M>
__device__ __forceinline__ void rank_job(int ny, int chunk, V val, M keep, uint64_t* skey, uint64_t* gkeys, double* rk) {
  const int t = threadIdx.x;
  const int nch = (ny + chunk - 1) / chunk;
  for (int c = 0; c < nch; ++c) {
    const int r0 = c * chunk, L = min(chunk, ny - r0);
    int P = 2;
    while (P < L) P <<= 1;
    for (int i = t; i < P; i += MF_NT) skey[i] = (i < L && keep(r0 + i)) ? rank_key(val(r0 + i)) : ~0ull;
    __syncthreads();
    bitonic_sort(skey, P);
    if (nch > 1) {
      for (int i = t; i < L; i += MF_NT) gkeys[r0 + i] = skey[i];
      __syncthreads();  // the chunk is in global memory, for this workgroup, before LDS is reused or it is read
    }
  }
  for (int i = t; i < ny; i += MF_NT) {
    if (!keep(i)) continue;
    const uint64_t x = rank_key(val(i));
    int lo = 0, hi = 0;
    if (nch == 1)
      count_bounds(skey, ny, x, lo, hi);
    else
      for (int c = 0; c < nch; ++c) count_bounds(gkeys + (size_t)c * chunk, min(chunk, ny - c * chunk), x, lo, hi);
    rk[i] = (double)lo + 0.5 * (double)(hi - lo + 1);
  }
  __syncthreads();
}

// sqrt of the mean of (a - b)^2 over the rows where that term is not NaN
template <class A, class B>
__device__ __forceinline__ double rmse_of(int ny, A a, B b, double* red) {
  double v[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < ny; i += MF_NT) {
    const double d = a(i) - b(i), q = d * d;
    if (q == q) v[0] += q, v[1] += 1.0;
  }
  block_sum(v, red);
  return sqrt(v[0] / v[1]);  // no row: 0 / 0
}

// sign(co) co^2 of the two-pass Pearson correlation over the rows where neither value is NaN
template <class A, class B>
__device__ __forceinline__ double corr_of(int ny, A a, B b, double* red) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < ny; i += MF_NT) {
    const double x = a(i), y = b(i);
    if (x == x && y == y) s[0] += 1.0, s[1] += x, s[2] += y;
  }
  block_sum(s, red);
  if (s[0] < 2.0) return nan;
  const double ma = s[1] / s[0], mb = s[2] / s[0];
  double c[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < ny; i += MF_NT) {
    const double x = a(i), y = b(i);
    if (x == x && y == y) {
      const double dx = x - ma, dy = y - mb;
      c[0] += dx * dy, c[1] += dx * dx, c[2] += dy * dy;
    }
  }
  block_sum(c, red);
  double co = c[0] / sqrt(c[1] * c[2]);
  co = co > 1.0 ? 1.0 : co < -1.0 ? -1.0 : co;  // (as np.corrcoef clips; NaN stays)
  return co < 0.0 ? -(co * co) : co * co;
}

// Spearman: Pearson on the average ranks over the pairwise-complete rows
template <class A, class B>
__device__ __forceinline__ double spearman_of(int ny, int chunk, A a, B b, uint64_t* skey, double* scr, double* red) {
  uint64_t* gkeys = (uint64_t*)scr;
  double *ra = scr + ny, *rb = scr + 2 * (size_t)ny;
  auto ok = [&](int i) {
    const double x = a(i), y = b(i);
    return x == x && y == y;
  };
  rank_job(ny, chunk, a, ok, skey, gkeys, ra);
  rank_job(ny, chunk, b, ok, skey, gkeys, rb);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  return corr_of(ny, [&](int i) { return ok(i) ? ra[i] : nan; }, [&](int i) { return ok(i) ? rb[i] : nan; }, red);
}

// _auc of predict.py over the rows with y not NaN, classes 1[y > 0]
template <class Yv, class P>
__device__ __forceinline__ double auc_of(int ny, int chunk, Yv y, P p, uint64_t* skey, double* scr, double* red) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double v[3] = {0.0, 0.0, 0.0};  // rows, positives, NaN predictions
  for (int i = threadIdx.x; i < ny; i += MF_NT) {
    const double yi = y(i), pi = p(i);
    if (yi == yi) v[0] += 1.0, v[1] += yi > 0.0 ? 1.0 : 0.0, v[2] += pi != pi ? 1.0 : 0.0;
  }
  block_sum(v, red);
  const double n1 = v[1], n0 = v[0] - v[1];
  if (n1 == 0.0 || n0 == 0.0 || v[2] > 0.0) return nan;
  double* rk = scr + ny;
  rank_job(ny, chunk, p, [&](int i) { const double yi = y(i); return yi == yi; }, skey, (uint64_t*)scr, rk);
  double r[1] = {0.0};
  for (int i = threadIdx.x; i < ny; i += MF_NT)
    if (y(i) > 0.0) r[0] += rk[i];
  block_sum(r, red);
  return (r[0] - n1 * (n1 + 1.0) / 2.0) / (n1 * n0);
}

// mean of p over class 1 minus its mean over class 0
template <class C1, class C0, class P>
__device__ __forceinline__ double tjur_of(int ny, C1 one, C0 zero, P p, double* red) {
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < ny; i += MF_NT) {
    if (one(i)) v[0] += p(i), v[1] += 1.0;
    if (zero(i)) v[2] += p(i), v[3] += 1.0;
  }
  block_sum(v, red);
  return v[0] / v[1] - v[2] / v[3];  // an empty class: 0 / 0
}

template <int NKEY>
__global__ __launch_bounds__(MF_NT) void model_fit_kernel(MfArgs a) {
  __shared__ uint64_t skey[NKEY];
  __shared__ double red[5 * MF_NW];
  const int sl = blockIdx.x, ny = a.ny, chunk = a.chunk;
  const int fam = a.family[a.j0 + sl];
  const double* Y = a.Y + (size_t)sl * ny;
  const double* M = a.m + (size_t)sl * ny;
  const double* O = a.pO ? a.pO + (size_t)sl * ny : nullptr;
  double* scr = a.scratch + (size_t)sl * 3 * ny;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double res[MF_OUT];
#pragma unroll
  for (int k = 0; k < MF_OUT; ++k) res[k] = nan;
  auto y = [&](int i) { return Y[i]; };
  auto m = [&](int i) { return M[i]; };
  res[MF_RMSE] = rmse_of(ny, y, m, red);
  if (fam == 1) {
    res[MF_R2] = corr_of(ny, y, m, red);
  } else if (fam == 2) {
    res[MF_AUC] = auc_of(ny, chunk, y, m, skey, scr, red);
    res[MF_TJUR] = tjur_of(ny, [&](int i) { return Y[i] == 1.0; }, [&](int i) { return Y[i] == 0.0; }, m, red);
  } else {
    auto o = [&](int i) { return O[i]; };
    auto yo = [&](int i) { const double v = Y[i]; return v != v ? v : v > 0.0 ? 1.0 : 0.0; };  // 1[Y > 0], NA kept
    auto yc = [&](int i) { const double v = Y[i]; return v == 0.0 ? nan : v; };                // Y with 0 -> NA
    auto mc = [&](int i) { return M[i] / O[i]; };
    res[MF_SR2] = spearman_of(ny, chunk, y, m, skey, scr, red);
    res[MF_OAUC] = auc_of(ny, chunk, y, o, skey, scr, red);
    res[MF_OTJUR] = tjur_of(ny, [&](int i) { return Y[i] > 0.0; }, [&](int i) { const double v = Y[i]; return v == v && !(v > 0.0); }, o, red);
    res[MF_ORMSE] = rmse_of(ny, yo, o, red);
    res[MF_CSR2] = spearman_of(ny, chunk, yc, mc, skey, scr, red);
    res[MF_CRMSE] = rmse_of(ny, yc, mc, red);
  }
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < MF_OUT; ++k) a.out[(size_t)k * a.ns + a.j0 + sl] = res[k];
}

// whole call (host clock), uploads, kernels (device events summed over the slabs; -1 for a call
// of more slabs than are timed) of this thread's last run_model_fit, ms
static thread_local double g_model_fit_ms[3] = {0.0, 0.0, 0.0};
void model_fit_last_timing(double out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_model_fit_ms[k];
}

void run_model_fit(const hmsc_model_fit_args* p, double* out) {
  const auto t_start = std::chrono::steady_clock::now();
  HMSC_REQUIRE(p && out, "hmsc_model_fit: NULL argument (args, out)");
  HMSC_REQUIRE(p->Y && p->m && p->family, "hmsc_model_fit: NULL argument (Y, m, family)");
  HMSC_REQUIRE(p->ny >= 1 && p->ns >= 1, "hmsc_model_fit: ny = " + std::to_string(p->ny) + ", ns = " +
                                             std::to_string(p->ns) + ": both must be at least 1");
  HMSC_REQUIRE(p->chunk_rows >= 0, "hmsc_model_fit: chunk_rows = " + std::to_string(p->chunk_rows) + " is negative");
  const int ny = p->ny, ns = p->ns;
  bool poisson = false;
  for (int j = 0; j < ns; ++j) {
    HMSC_REQUIRE(p->family[j] >= 1 && p->family[j] <= 3, "hmsc_model_fit: family = " + std::to_string(p->family[j]) +
                                                           " of species " + std::to_string(j) + " is outside 1..3");
    poisson = poisson || p->family[j] == 3;
  }
  HMSC_REQUIRE(!poisson || p->pO, "hmsc_model_fit: pO is NULL while a Poisson column exists");
  const bool with_o = p->pO != nullptr;
  // slabs of whole species within scratch_bytes: the inputs' columns and 3 ny doubles of scratch each
  const uint64_t scratch = p->scratch_bytes ? p->scratch_bytes : (uint64_t)1 << 30;
  const size_t col_bytes = (size_t)ny * sizeof(double), sp_bytes = ((with_o ? 3 : 2) + 3) * col_bytes;
  HMSC_REQUIRE(scratch >= sp_bytes, "hmsc_model_fit: scratch_bytes = " + std::to_string(scratch) +
                                        " is below one species' need (ny = " + std::to_string(ny) + ": " +
                                        std::to_string(sp_bytes) + " bytes)");
  const int nsl = (int)std::min<uint64_t>((uint64_t)ns, scratch / sp_bytes);
  const int nslab = (ns + nsl - 1) / nsl;
  const int chunk = std::min(ny, p->chunk_rows ? std::min(p->chunk_rows, MF_CAP) : MF_CAP);
  DeviceGuard dg(p->device);
  const size_t need = (size_t)nsl * sp_bytes + (size_t)ns * (sizeof(int) + MF_OUT * sizeof(double));
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  HMSC_REQUIRE(need <= free_b, "hmsc_model_fit: the call needs " + std::to_string(need) +
                                   " bytes of device memory (ny = " + std::to_string(ny) + ", " + std::to_string(nsl) +
                                   " species per slab), the device has " + std::to_string(free_b) + " bytes free");
  DeviceOwner b;
  const hipStream_t st = b.stream();
  MfArgs a{};
  a.ny = ny, a.ns = ns, a.chunk = chunk;
  a.family = b.upload(p->family, ns, st);
  double* dY = b.alloc<double>((size_t)nsl * ny);
  double* dM = b.alloc<double>((size_t)nsl * ny);
  double* dO = with_o ? b.alloc<double>((size_t)nsl * ny) : nullptr;
  a.Y = dY, a.m = dM, a.pO = dO;
  a.scratch = b.alloc<double>((size_t)nsl * 3 * ny);
  a.out = b.alloc<double>((size_t)MF_OUT * ns);
  constexpr int TIMED_SLABS = 256;
  const bool timed = nslab <= TIMED_SLABS;
  std::vector<hipEvent_t> ev;
  if (timed)
    for (int k = 0; k < 3 * nslab; ++k) ev.push_back(b.event());
  for (int k = 0; k < nslab; ++k) {
    a.j0 = k * nsl, a.nsl = std::min(nsl, ns - a.j0);
    const size_t off = (size_t)a.j0 * ny, bytes = (size_t)a.nsl * col_bytes;
    hipEvent_t* e = timed ? &ev[3 * (size_t)k] : nullptr;
    if (e) HIP_OK(hipEventRecord(e[0], st));
    HIP_OK(hipMemcpyAsync(dY, p->Y + off, bytes, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(dM, p->m + off, bytes, hipMemcpyHostToDevice, st));
    if (with_o) HIP_OK(hipMemcpyAsync(dO, p->pO + off, bytes, hipMemcpyHostToDevice, st));
    if (e) HIP_OK(hipEventRecord(e[1], st));
    if (chunk <= MF_SMALL)
      model_fit_kernel<MF_SMALL><<<a.nsl, MF_NT, 0, st>>>(a);
    else
      model_fit_kernel<MF_CAP><<<a.nsl, MF_NT, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    if (e) HIP_OK(hipEventRecord(e[2], st));
  }
  HIP_OK(hipMemcpyAsync(out, a.out, (size_t)MF_OUT * ns * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  double up = timed ? 0.0 : -1.0, kn = up;
  for (size_t k = 0; timed && k + 2 < ev.size(); k += 3) {
    float u_ms = 0.f, k_ms = 0.f;
    HIP_OK(hipEventElapsedTime(&u_ms, ev[k], ev[k + 1]));
    HIP_OK(hipEventElapsedTime(&k_ms, ev[k + 1], ev[k + 2]));
    up += u_ms, kn += k_ms;
  }
  g_model_fit_ms[0] = ms_since(t_start), g_model_fit_ms[1] = up, g_model_fit_ms[2] = kn;
}

}  // namespace hmsc
