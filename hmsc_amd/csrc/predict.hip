// predict.Hmsc on the device (R/predict.R:143-229): for every posterior
// sample s,
//   L_s = X Beta_s + sum_r Eta_r,s[Pi_r,] Lambda_r,s                               (:154-189)
//   expected:  probit pnorm(L), Poisson exp(L + sigma/2), normal L                  (:203-218)
//   draws:     Z = L + sqrt(sigma) N(0,1); probit 1[Z > 0], Poisson rpois(exp(Z))   (:198-218)
//              rpois (:216) of a NaN or infinite rate is NaN, as in R: Z = NaN, or exp(Z)
//              overflowing past Z = 709.78 where a new X extrapolates a Poisson species
//   then the YScalePar back-transform Z s + m                                       (:222-227)
// out[s] is ny x ns column-major, as R's pred[[s]].
//
// One launch covers all samples: grid (site tiles, species tiles, samples); a workgroup
// stages the 64-site rows of [X | Eta_1[Pi_1,] | ...] and the K x 32 coefficient block
// [Beta_s; Lambda_1,s; ...] in LDS and writes a 64 x 32 output tile with coalesced
// 512-B site runs.  K = nc + sum nf is small (<= 128), so the kernel streams its output:
// the HBM bound is nsamples * ny * ns * 8 B of writes.  The two tiles take
// (64 (K | 1) + 32 K) 8 B of dynamic LDS: past 64 KB from K = 86 on, 98,816 B at K = 128, which
// a gfx950 workgroup is granted as it stands (160 KB per CU; tests/test_gpu_predict_cells.py
// launches K = 86, 127 and 128).
// Randomness: normal = inversion of the first uniform of (cell, 0, S_PREDICT, s), Poisson
// PTRS trial t uses (cell, 1 + t, S_PREDICT, s); cell = i + ny j (oracle predict_oracle).
// The staging, the fma chain and the per-cell epilogue are predict_cell.h's, shared with the
// summary kernel (summary.hip).
#include <vector>

#include "predict_cell.h"

namespace hmsc {

__global__ __launch_bounds__(256) void predict_kernel(PredArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x, i0 = blockIdx.x * PT_I, j0 = blockIdx.y * PT_J, s = blockIdx.z;
  const int ny = a.ny, ns = a.ns, K = a.K;
  const int LD = K | 1;                 // odd: conflict-free column reads
  double* sA = smem;                    // [site][k], padded
  double* sB = smem + PT_I * LD;        // [k][species]
  stage_sites(a, sA, LD, i0, s, 0, t);
  stage_species(a, sB, j0, s, t);
  __syncthreads();
  const int ii = t & 63, jb = t >> 6;  // thread: site ii, species jb, jb+4, ..., jb+28
  const int i = i0 + ii;
  if (i >= ny) return;
  double acc[8];
  linear_predictor(sA, sB, LD, K, ii, jb, acc);
  double* out = a.out + (size_t)s * ny * ns;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int j = j0 + jb + 4 * q;
    if (j >= ns) continue;
    const uint32_t cell = (uint32_t)((size_t)i + (size_t)ny * j);
    out[i + (size_t)ny * j] = predict_cell(a, acc[q], a.sigma[(size_t)s * ns + j], a.family[j], a.yscale[2 * j],
                                           a.yscale[2 * j + 1], cell, s);
  }
}

// host side: upload, one launch, download (called by hmsc_predict in capi.cpp)
void run_predict(const hmsc_predict_args* p, double* out) {
  const int K = check_pred_limits(p);
  DeviceGuard dg(p->device);
  const size_t S = p->nsamples, ny = p->ny, ns = p->ns;
  std::vector<int> pi0;  // (source of a copy on the stream: before its owner)
  DeviceOwner own;  // drains the stream and frees the uploads on every exit
  const hipStream_t st = own.stream();
  PredArgs a = upload_pred_args(p, own, st, pi0);
  a.out = own.alloc<double>(S * ny * ns);
  if (S > 0) {
    dim3 grid((p->ny + PT_I - 1) / PT_I, (p->ns + PT_J - 1) / PT_J, p->nsamples);
    predict_kernel<<<grid, 256, pred_lds_bytes(K), st>>>(a);
    HIP_OK(hipGetLastError());
    copy_sync(out, a.out, S * ny * ns * 8, hipMemcpyDeviceToHost, st);
  }
}

}  // namespace hmsc
