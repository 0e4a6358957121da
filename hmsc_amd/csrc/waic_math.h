// Scalar functions of computeWAIC's cell terms (waic.hip; hmsc_debug_eval "log_pnorm" in
// draweval.hip evaluates the same code with the same flags).
#pragma once
#include "rng.h"

namespace hmsc {

// log(erfc(a / sqrt 2) / 2) = log Phi(-a) for a >= 0, on the whole half line.  erfc_fast has the
// form t exp(-z^2 + g(t)), t = 2 / (2 + z), with g fitted on all of t in (0, 1] (scripts/
// fit_erfc.py), so the logarithm is log t - z^2 + g(t) - log 2 and never sees erfc's underflow.
// z^2 = a^2 / 2 is taken exactly as hi + lo (one product, one fma); t and g are smooth in z, so
// the rounding of z = a / sqrt 2 moves them by ~1e-16 relative.  An a^2 / 2 beyond the double
// range gives -inf.
__host__ __device__ __forceinline__ double log_pnorm_lower(double a) {
  const double z = a * 0.7071067811865476;
  const double t = 2.0 / (2.0 + z);
  const double x = 2.0 * t - 1.0;
  double g = kErfcPoly[0];
#pragma unroll
  for (int k = 1; k < ERFC_NC; ++k) g = fma_sc(g, x, kErfcPoly[k]);
  const double h = 0.5 * a;  // exact
  const double hi = h * a;
  if (hi > 1.7976931348623157e308) return -hi;
  const double lo = fma(h, a, -hi);
  const double lt = t < 1.0 ? log_fast(fmax(t, 2.3e-308)) : 0.0;
  return ((lt + g - 0.6931471805599453) - lo) - hi;
}

// log Phi(x).  x <= 0: log_pnorm_lower(-x).  x > 0: log1p(-p), p = Phi(-x) = exp(log_pnorm_lower(x))
// in (0, 1/2), with log1p(-p) = log u + ((1 - u) - p) / u, u = fl(1 - p): 1 - u is exact (u in
// [1/2, 1]), so the quotient restores what the rounding of u lost and the result keeps its
// relative accuracy down to p -> 0, where it is -p.
__host__ __device__ __forceinline__ double log_pnorm(double x) {
  const double lower = log_pnorm_lower(fabs(x));
  if (!(x > 0.0)) return lower;
  const double p = exp(lower);
  const double u = 1.0 - p;
  const double c = (1.0 - u) - p;
  const double lu = u < 1.0 ? log_fast(u) : 0.0;
  return lu + c / u;
}

}  // namespace hmsc
