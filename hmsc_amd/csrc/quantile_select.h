// What summary.hip and community.hip share: R's type-7 quantiles of one thread's strided column of
// a sample slab, by exact bisection selection over the order-preserving 64-bit key of the double.
// 64 counting passes fix the key of x_(floor h), h = (n - 1) p, bit by bit for all probabilities of
// the call at once, one more pass finds the smallest value above it.  Reads only, all lanes in
// lockstep, nothing indexed at run time (no scratch memory); exact and deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace hmsc {

// the order-preserving key of a double: negative values reversed below the positive ones
__device__ __forceinline__ uint64_t order_key(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double key_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k;
  return __longlong_as_double((long long)u);
}

// The values x[s * stride], s = 0 .. S - 1, n >= 1 of them not NaN; quant[q * plane] for q < nq gets
// the quantile at probs[q].  NQ probabilities at once (nq <= NQ; the surplus repeats the last and
// is not stored).
template <int NQ>
__device__ __forceinline__ void select_quantiles(const double* x, size_t stride, int S, int n, const double* probs,
                                                 int nq, double* quant, size_t plane) {
  int rank[NQ];      // floor(h)
  double frac[NQ];   // h - floor(h)
  uint64_t key[NQ];  // the key of x_(rank), fixed from the top bit down
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double h = (double)(n - 1) * probs[q < nq ? q : nq - 1];
    const double fl = floor(h);
    rank[q] = (int)fl;
    frac[q] = h - fl;
    key[q] = 0;
  }
  for (int b = 63; b >= 0; --b) {
    // bit b stays 0 if at least rank + 1 values have a key <= prefix | (all ones below b)
    const uint64_t low = b ? (~0ull >> (64 - b)) : 0ull;
    int le[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) le[q] = 0;
    for (int s = 0; s < S; ++s) {
      const double v = x[(size_t)s * stride];
      if (v != v) continue;
      const uint64_t kv = order_key(v);
#pragma unroll
      for (int q = 0; q < NQ; ++q) le[q] += kv <= (key[q] | low) ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (le[q] < rank[q] + 1) key[q] |= 1ull << b;
  }
  // ties at x_(rank) reach the next rank; otherwise the next order statistic is the smallest value above
  int le[NQ];
  uint64_t above[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) le[q] = 0, above[q] = ~0ull;
  for (int s = 0; s < S; ++s) {
    const double v = x[(size_t)s * stride];
    if (v != v) continue;
    const uint64_t kv = order_key(v);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      le[q] += kv <= key[q] ? 1 : 0;
      above[q] = kv > key[q] && kv < above[q] ? kv : above[q];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (q >= nq) continue;
    const double lo = key_value(key[q]);
    double r = lo;
    if (frac[q] > 0.0) {
      const double hi = le[q] >= rank[q] + 2 ? lo : key_value(above[q]);
      if (hi != lo) {
#pragma clang fp contract(off)
        const double d = hi - lo;
        const double m = frac[q] * d;
        r = lo + m;  // one rounding each: the type-7 formula as the host writes it
      }
    }
    quant[q * plane] = r;
  }
}

}  // namespace hmsc
