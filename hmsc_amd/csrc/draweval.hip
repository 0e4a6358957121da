// hmsc_debug_eval (include/hmsc_amd.h): the device halves of rng.h's scalar functions, evaluated
// elementwise on arrays a test supplies.  Compiled with the flags of the sweep's kernels, so the
// device-only code under __HIP_DEVICE_COMPILE__ (rcp_pos, exp_small, fma_sc, log_fast) is held to
// a reference as the updaters run it (log_pnorm of waic_math.h: as waic.hip, built with the same flags, runs it).  The table draw of the z kernel is evaluated by zdraw.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "rng.h"
#include "waic_math.h"

namespace hmsc {

enum DrawEval { EV_TRUNC_NORMAL = 0, EV_QNORM, EV_ERFC, EV_LOG, EV_EXP_SMALL, EV_PG_MOMENTS, EV_LOG_PNORM, EV_RNG_COUNT };

__global__ __launch_bounds__(256) void draw_eval_kernel(int what, int64_t n, const double* in0, const double* in1,
                                                        double* out0, double* out1) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double a = in0[i];
    switch (what) {
      case EV_TRUNC_NORMAL: out0[i] = trunc_normal_lower(a, in1[i]); break;
      case EV_QNORM: out0[i] = qnorm_fast(a); break;
      case EV_ERFC: out0[i] = erfc_fast(a); break;
      case EV_LOG: out0[i] = log_fast(a); break;
      case EV_EXP_SMALL: out0[i] = exp_small(a); break;
      case EV_LOG_PNORM: out0[i] = log_pnorm(a); break;
      default: {
        double m, v;
        pg_moments(a, in1[i], &m, &v);
        out0[i] = m;
        out1[i] = v;
      }
    }
  }
}

// what: a DrawEval; in1 / out1 are read / written by the two-argument / two-result entries only
void launch_draw_eval(hipStream_t st, int what, int64_t n, const double* in0, const double* in1, double* out0,
                      double* out1) {
  HMSC_REQUIRE(what >= 0 && what < EV_RNG_COUNT, "internal: draw_eval selector");
  const int grid = (int)std::min<int64_t>(1024, (n + 255) / 256);
  draw_eval_kernel<<<grid, 256, 0, st>>>(what, n, in0, in1, out0, out1);
  HIP_OK(hipGetLastError());
}

}  // namespace hmsc
